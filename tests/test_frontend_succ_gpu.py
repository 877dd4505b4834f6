"""The resident front-end map, its yaw-free table and the batched successor test (svsdf_frontend_set_map,
svsdf_frontend_yaw_free, svsdf_astar_successors) against the reference's four steps of AstarPathSearcher::AstarGetSucc
(front_end_Astar.hpp:192-241).

The map-side integer code -- generateMapKernel2D (PCSmap_manager.h:81-108), kernelConv<true> byte for byte with its
shifts (sw_manager.hpp:1033-1099), the yaw search (test_frontend_succ.bfs_ref), getPointsInAABB2D
(PCSmap_manager.h:137-158) -- is restated here in plain Python; the SDF side (byte kernels, checkSubSWCollision) is
the oracle's.  Booleans, stages and the bits of the yaws must be equal."""
import functools
import json
import math
import os

import numpy as np
import pytest

from oracle import orc
from test_frontend_succ import bfs_ref, handout_yaws

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
ASSETS = json.load(open(os.path.join(HERE, "golden", "reference_assets.json")))


# ---------------------------------------------------------------- restatement of the map side
def grid_from_cloud(cloud, res, sta_threshold=1):
    """PCSmapManager::rcvGlobalMapHandler (PCSmap_manager.cpp:116-178) -> (occ [X, Y, Z] bool, bmin, bmax)."""
    c = np.asarray(cloud, dtype=np.float32).astype(np.float64)
    bmin, bmax = c.min(0), c.max(0)
    dims = np.ceil((bmax - bmin) / res).astype(int)
    idx = np.floor((c - bmin) / res).astype(int)
    idx = np.minimum(np.maximum(idx, 0), dims - 1)
    cnt = np.zeros(dims, dtype=int)
    np.add.at(cnt, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    return cnt >= sta_threshold, bmin, bmax


def generate_map_kernel_2d(occ0, ks):
    """generateMapKernel2D: the inflated byte map, bit 0x80 >> (y % 8), row-major in x.  One more byte than the
    reference allocates stands for what it reads past the array on the last row; it is 0xFF here: those bits only meet
    kernel columns >= kernel_size."""
    X, Y = occ0.shape
    side = (ks - 1) // 2
    bpl = (Y + 2 * side + 7) // 8
    mk = np.zeros((X + 2 * side) * bpl + 1, dtype=np.uint8)
    for x, y in zip(*np.nonzero(occ0)):
        fx, fy = x + side, y + side
        mk[fx * bpl + fy // 8] |= 0x80 >> (fy % 8)
    mk[-1] = 0xFF
    return mk, bpl


def yaw_free_ref(occ0, kbytes, ks):
    """bit k of [ix, iy] = kernelConv<true>(k, (ix, iy, 0)), all cells at once; kbytes: the oracle's byte kernels
    [count, ks, (ks + 7) // 8]."""
    X, Y = occ0.shape
    count, kbpl = kbytes.shape[0], (ks + 7) // 8
    mk, bpl = generate_map_kernel_2d(occ0, ks)
    ix, iy = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    off = (iy % 8).astype(np.uint16)
    hit = np.zeros((count, X, Y), dtype=bool)
    for i in range(ks):
        start = (ix + i) * bpl + iy // 8
        for j in range(kbpl):
            a = mk[start + j].astype(np.uint16)
            b = mk[start + j + 1].astype(np.uint16)
            block = (((a << off) | (b >> (8 - off))) & 0xFF).astype(np.uint8)
            hit |= (kbytes[:, i, j][:, None, None] & block[None]) != 0
    free = np.zeros((X, Y), dtype=np.uint64)
    for k in range(count):
        free |= (~hit[k]).astype(np.uint64) << np.uint64(k)
    return free


def box_ids(c, half, bmin, bmax, res, size):
    """projInMap (PCSmap_manager.h:128-135) + getGridIndex (Gridmap3D.cpp:137-177) of centre -+ half, one axis."""
    out = []
    for a in (c - half, c + half):
        a = min(max(a, bmin), bmax)
        i = int(math.floor((a - bmin) / res))
        out.append(min(max(i, 0), size - 1))
    return out


def successors_ref(o, occ, bmin, bmax, res, free, ks, count, parents, yaws):
    """The four steps per (parent, neighbour) -> ok [n, 9], child yaw [n, 9], stage [n, 9]."""
    X, Y = occ.shape[:2]
    occ0 = occ[:, :, 0]
    half = float(ks // 2 + 1)
    n = len(parents)
    ok = np.zeros((n, 9), dtype=bool)
    cyaw = np.full((n, 9), np.nan)
    stage = np.zeros((n, 9), dtype=np.uint8)
    centre = lambda i, d: (i + 0.5) * res + bmin[d]
    for p, ((pi, pj), fy) in enumerate(zip(parents, yaws)):
        father = [centre(pi, 0), centre(pj, 1), fy]
        for s in range(9):
            vi, vj = pi + s // 3 - 1, pj + s % 3 - 1
            if not (0 <= vi < X and 0 <= vj < Y):
                stage[p, s] = 1
                continue
            if occ0[vi, vj]:
                stage[p, s] = 2
                continue
            r = bfs_ref(int(free[vi, vj]), count, fy)
            assert r != "error"
            if r is None:
                stage[p, s] = 3
                continue
            cy = r[0]
            cx, cyy = centre(vi, 0), centre(vj, 1)
            i1, i2 = box_ids(cx, half, bmin[0], bmax[0], res, X)
            j1, j2 = box_ids(cyy, half, bmin[1], bmax[1], res, Y)
            sub = occ0[i1:i2 + 1, j1:j2 + 1]
            ii, jj = np.nonzero(sub)
            pts = np.column_stack([(ii + i1 + 0.5) * res + bmin[0], (jj + j1 + 0.5) * res + bmin[1]])
            cyaw[p, s] = cy
            if o.check_sub_sw_collision(father, [cx, cyy, cy], pts):
                ok[p, s] = True
            else:
                stage[p, s] = 4
    return ok, cyaw, stage


# ---------------------------------------------------------------- synthetic maps
GRIDS = [(5, 11), (13, 70), (65, 129)]
KERNELS = [(3, 2), (9, 8), (17, 18), (63, 64)]
LAYOUTS = ["none", "all", "border", "one", "random"]


def layout(name, X, Y, seed):
    g = np.zeros((X, Y), dtype=bool)
    if name == "all":
        g[:] = True
    elif name == "border":      # the four corners and the border
        g[0, :] = g[-1, :] = True
        g[:, 0] = g[:, -1] = True
    elif name == "one":         # meets kernel row / column 0 and kernel_size - 1 of the cells `side` away, where the grid has them
        g[X // 2, Y // 2] = True
    elif name == "random":
        g = np.random.default_rng(seed).random((X, Y)) < 0.3
    return g


def cloud_of(g, res):
    """A cloud whose grid at `res` with sta_threshold = 2 is g in layer 0: two corner points fix the bounds (one point
    each: below the threshold), two points at the centre of every occupied cell."""
    X, Y = g.shape
    ii, jj = np.nonzero(g)
    c = np.column_stack([(ii + 0.5) * res, (jj + 0.5) * res, np.full(len(ii), 0.5 * res)])
    return np.vstack([[[0.0, 0.0, 0.0], [X * res, Y * res, res]], c, c]).astype(np.float32)


# A table that is all ones or all zeros compares nothing but one constant.  Outside the "none" and "all" layouts every case
# must therefore have a mixed table -- except where the geometry leaves no room for one, which is a property of the inputs
# (worked out with yaw_free_ref and the oracle's kernels alone, before any device code ran): a grid much smaller than the
# robot (5 x 11 cells of 0.25 m hold a star of radius 2.8 m nowhere once any cell is occupied), 30 % random occupancy under
# a kernel of 9 cells and more, and the 3 x 3 kernel of the hollow horseshoe at 0.25 m, which is empty at margin 0.5.
# (X, Y, res, shape, kernel_size, layout) -> what the expected table is there.
DEGENERATE = {
    (5, 11, 1.0, 'star', 9, 'border'): 'zeros',
    (5, 11, 1.0, 'star', 17, 'border'): 'zeros',
    (5, 11, 1.0, 'star', 17, 'random'): 'zeros',
    (5, 11, 1.0, 'star', 63, 'border'): 'zeros',
    (5, 11, 1.0, 'star', 63, 'random'): 'zeros',
    (5, 11, 1.0, 'sdHorseshoe', 9, 'border'): 'zeros',
    (5, 11, 1.0, 'sdHorseshoe', 17, 'border'): 'zeros',
    (5, 11, 1.0, 'sdHorseshoe', 63, 'border'): 'zeros',
    (5, 11, 0.25, 'star', 9, 'border'): 'zeros',
    (5, 11, 0.25, 'star', 9, 'random'): 'zeros',
    (5, 11, 0.25, 'star', 17, 'border'): 'zeros',
    (5, 11, 0.25, 'star', 17, 'one'): 'zeros',
    (5, 11, 0.25, 'star', 17, 'random'): 'zeros',
    (5, 11, 0.25, 'star', 63, 'border'): 'zeros',
    (5, 11, 0.25, 'star', 63, 'one'): 'zeros',
    (5, 11, 0.25, 'star', 63, 'random'): 'zeros',
    (5, 11, 0.25, 'sdHorseshoe', 3, 'border'): 'ones',
    (5, 11, 0.25, 'sdHorseshoe', 3, 'one'): 'ones',
    (5, 11, 0.25, 'sdHorseshoe', 3, 'random'): 'ones',
    (13, 70, 1.0, 'star', 9, 'random'): 'zeros',
    (13, 70, 0.25, 'star', 9, 'random'): 'zeros',
    (13, 70, 0.25, 'star', 17, 'border'): 'zeros',
    (13, 70, 0.25, 'star', 17, 'random'): 'zeros',
    (13, 70, 0.25, 'star', 63, 'border'): 'zeros',
    (13, 70, 0.25, 'star', 63, 'random'): 'zeros',
    (13, 70, 0.25, 'sdHorseshoe', 3, 'border'): 'ones',
    (13, 70, 0.25, 'sdHorseshoe', 3, 'one'): 'ones',
    (13, 70, 0.25, 'sdHorseshoe', 3, 'random'): 'ones',
    (13, 70, 0.25, 'sdHorseshoe', 17, 'border'): 'zeros',
    (13, 70, 0.25, 'sdHorseshoe', 17, 'random'): 'zeros',
    (13, 70, 0.25, 'sdHorseshoe', 63, 'border'): 'zeros',
    (13, 70, 0.25, 'sdHorseshoe', 63, 'random'): 'zeros',
    (65, 129, 0.25, 'star', 9, 'random'): 'zeros',
    (65, 129, 0.25, 'star', 17, 'random'): 'zeros',
    (65, 129, 0.25, 'star', 63, 'random'): 'zeros',
    (65, 129, 0.25, 'sdHorseshoe', 3, 'border'): 'ones',
    (65, 129, 0.25, 'sdHorseshoe', 3, 'one'): 'ones',
    (65, 129, 0.25, 'sdHorseshoe', 3, 'random'): 'ones',
    (65, 129, 0.25, 'sdHorseshoe', 63, 'random'): 'zeros',
}


@functools.lru_cache(maxsize=None)
def oracle_bytes(shape, ks, count, res, margin):
    m, b, yaws, n = orc.Oracle(shape).shape_kernels(ks, count, res, margin)
    return b


@pytest.fixture(scope="module")
def ctxs(built):
    import svsdf_amd
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = svsdf_amd.SvsdfContext(shape=shape, device=0)
        return made[shape]
    return get


@pytest.mark.parametrize("ks,count", KERNELS)
@pytest.mark.parametrize("shape", ["star", "sdHorseshoe"])
@pytest.mark.parametrize("res", [1.0, 0.25])
@pytest.mark.parametrize("X,Y", GRIDS)
def test_yaw_free_table_synthetic(ctxs, X, Y, res, shape, ks, count):
    import svsdf_amd
    ctx = ctxs(shape)
    margin = 0.5
    kb = oracle_bytes(shape, ks, count, res, margin)
    full = np.uint64((1 << count) - 1)
    for name in LAYOUTS:
        g = layout(name, X, Y, seed=X * 1000 + Y + ks)
        om = svsdf_amd.OccupancyMap(cloud_of(g, res), resolution=res, sta_threshold=2)
        assert om.info()["dims"] == (X, Y, 1)
        ctx.frontend_set_map(om, ks, count, margin)
        got = ctx.yaw_free()
        want = yaw_free_ref(g, kb, ks)
        assert got.shape == (X, Y) and got.dtype == np.uint64
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {X}x{Y} res {res} {shape} {ks}/{count}")
        kind = "ones" if (want == full).all() else "mixed" if want.any() else "zeros"
        if name == "none":
            assert kind == "ones"
        elif name != "all":
            assert kind == DEGENERATE.get((X, Y, res, shape, ks, name), "mixed"), (name, kind)


# ---------------------------------------------------------------- reference maps
KS, KC, MARGIN = 17, 18, 0.5


@functools.lru_cache(maxsize=None)
def reference_case(name):
    """Map `name` at resolution 1 with its own shape: grid, expected table, parents and the expected successors."""
    cloud = np.array(ASSETS["maps"][name], dtype=np.float32)
    occ, bmin, bmax = grid_from_cloud(cloud, 1.0)
    o = orc.Oracle(name)
    free = yaw_free_ref(occ[:, :, 0], oracle_bytes(name, KS, KC, 1.0, MARGIN), KS)
    X, Y = occ.shape[:2]
    cells = [(i, j) for i in range(0, X, 2) for j in range(0, Y, 3) if not occ[i, j, 0]]
    hy = handout_yaws(KC)
    parents = [c for c in cells for _ in (2, 9, 14)]
    yaws = [hy[k] for _ in cells for k in (2, 9, 14)]
    ok, cyaw, stage = successors_ref(o, occ, bmin, bmax, 1.0, free, KS, KC, parents, yaws)
    for a in (free, ok, cyaw, stage):
        a.setflags(write=False)
    return dict(cloud=cloud, occ=occ, bmin=bmin, bmax=bmax, free=free, parents=np.array(parents, dtype=np.int32),
                yaws=np.array(yaws), ok=ok, cyaw=cyaw, stage=stage)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("name", sorted(ASSETS["maps"]))
def test_table_and_successors_on_reference_maps(ctxs, name):
    import svsdf_amd
    case = reference_case(name)
    om = svsdf_amd.OccupancyMap(case["cloud"], resolution=1.0)
    info = om.info()
    assert info["dims"] == case["occ"].shape
    np.testing.assert_array_equal(info["bmin"], case["bmin"])
    np.testing.assert_array_equal(info["bmax"], case["bmax"])
    ctx = ctxs(name)
    ctx.frontend_set_map(om, KS, KC, MARGIN)
    np.testing.assert_array_equal(ctx.yaw_free(), case["free"])
    ok, cyaw, stage = ctx.astar_successors(case["parents"], case["yaws"])
    counts = np.bincount(case["stage"].ravel(), minlength=5)
    print(name, "stages 0..4:", counts.tolist())
    assert (counts > 0).all()                  # all five stages occur on every map
    np.testing.assert_array_equal(stage, case["stage"])
    np.testing.assert_array_equal(ok, case["ok"])
    np.testing.assert_array_equal(ok, stage == 0)
    assert _same_bits(cyaw, case["cyaw"])       # NaN where no yaw was chosen, on both sides
    assert np.isnan(cyaw[(stage != 0) & (stage != 4)]).all() and not np.isnan(cyaw[(stage == 0) | (stage == 4)]).any()


def test_successors_agree_with_check_sub_sw_collision(ctxs):
    """The accepted and the stage-4 slots of one map through the shipped path: svsdf_check_sub_sw_collision fed with
    the returned child yaws and host-gathered points."""
    import svsdf_amd
    case = reference_case("star")
    om = svsdf_amd.OccupancyMap(case["cloud"], resolution=1.0)
    ctx = ctxs("star")
    ctx.frontend_set_map(om, KS, KC, MARGIN)
    ok, cyaw, stage = ctx.astar_successors(case["parents"], case["yaws"])
    bmin, half = case["bmin"], float(KS // 2 + 1)
    fs, cs, pts, want = [], [], [], []
    for p, s in zip(*np.nonzero((stage == 0) | (stage == 4))):
        pi, pj = case["parents"][p]
        vi, vj = pi + s // 3 - 1, pj + s % 3 - 1
        centre = np.array([vi + 0.5 + bmin[0], vj + 0.5 + bmin[1], 0.0])
        g = om.gather(centre[None], [half, half, 0.0])
        fs.append([pi + 0.5 + bmin[0], pj + 0.5 + bmin[1], case["yaws"][p]])
        cs.append([centre[0], centre[1], cyaw[p, s]])
        pts.append(g[np.abs(g[:, 2] - (0.5 + bmin[2])) < 1e-9][:, :2])     # the box is one layer thick: layer 0
        want.append(ok[p, s])
    got = ctx.check_sub_sw_collision(np.array(fs), np.array(cs), pts)
    np.testing.assert_array_equal(got, np.array(want))
    assert any(want) and not all(want)


# ---------------------------------------------------------------- plumbing
def test_plumbing(built):
    import svsdf_amd
    case = reference_case("star")
    om = svsdf_amd.OccupancyMap(case["cloud"], resolution=1.0)
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0)
    with pytest.raises(svsdf_amd.SvsdfError, match="no map"):     # before any frontend_set_map
        ctx.astar_successors([[3, 3]], [0.0])
    with pytest.raises(svsdf_amd.SvsdfError, match="no map"):
        ctx.yaw_free()
    ctx.frontend_set_map(om, KS, KC, MARGIN)
    ok, cyaw, stage = ctx.astar_successors(np.zeros((0, 2), dtype=np.int32), np.zeros(0))     # n = 0
    assert ok.shape == (0, 9) and cyaw.shape == (0, 9) and stage.shape == (0, 9)
    # one parent alone and inside a batch of 5000
    reps = -(-5000 // len(case["parents"]))
    ij = np.tile(case["parents"], (reps, 1))[:5000]
    yw = np.tile(case["yaws"], reps)[:5000]
    okb, cyb, stb = ctx.astar_successors(ij, yw)
    np.testing.assert_array_equal(stb[:len(case["stage"])], case["stage"][:5000])
    for p in (0, 2503, 4999):
        ok1, cy1, st1 = ctx.astar_successors(ij[p:p + 1], yw[p:p + 1])
        assert ok1.tobytes() == okb[p:p + 1].tobytes() and cy1.tobytes() == cyb[p:p + 1].tobytes() \
            and st1.tobytes() == stb[p:p + 1].tobytes()
    # a parent outside the map, a yaw the search rejects: an error that names the parent; the context stays usable
    with pytest.raises(svsdf_amd.SvsdfError, match="parent 1 is outside the map"):
        ctx.astar_successors([[3, 3], [case["occ"].shape[0], 3]], [0.0, 0.0])
    with pytest.raises(svsdf_amd.SvsdfError, match="parent 0 is outside the map"):
        ctx.astar_successors([[3, -1]], [0.0])
    with pytest.raises(svsdf_amd.SvsdfError, match="yaw of parent 2"):
        ctx.astar_successors([[3, 3]] * 3, [0.0, 1.0, 3.1415926536])
    ok1, cy1, st1 = ctx.astar_successors(ij[:1], yw[:1])
    assert st1.tobytes() == stb[:1].tobytes() and cy1.tobytes() == cyb[:1].tobytes()
    # bad kernel geometry
    for ks, kc in ((16, 18), (0, 18), (-3, 18), (65, 18), (17, 65), (17, 0)):
        with pytest.raises(svsdf_amd.SvsdfError):
            ctx.frontend_set_map(om, ks, kc, MARGIN)
    np.testing.assert_array_equal(ctx.yaw_free(), case["free"])        # a refused call leaves the resident map alone
    # a second map replaces the first
    g = layout("random", 13, 70, seed=7)
    om2 = svsdf_amd.OccupancyMap(cloud_of(g, 1.0), resolution=1.0, sta_threshold=2)
    ctx.frontend_set_map(om2, 9, 8, MARGIN)
    np.testing.assert_array_equal(ctx.yaw_free(), yaw_free_ref(g, oracle_bytes("star", 9, 8, 1.0, MARGIN), 9))
    with pytest.raises(svsdf_amd.SvsdfError, match="outside the map"):
        ctx.astar_successors([[20, 3]], [0.0])      # inside the first map, outside the second
    # Polygon: no yaw kernels
    from svsdf_amd import workload
    with pytest.raises(svsdf_amd.SvsdfError, match="Polygon"):
        svsdf_amd.SvsdfContext(shape="Polygon", polygon=workload.star_outline(), device=0).frontend_set_map(om, KS, KC, MARGIN)
    # a multi-device context gives the same bytes as the single one
    multi = svsdf_amd.SvsdfContext(shape="star", devices=[0, 0])
    multi.frontend_set_map(om, KS, KC, MARGIN)
    np.testing.assert_array_equal(multi.yaw_free(), case["free"])
    okm, cym, stm = multi.astar_successors(ij, yw)
    assert okm.tobytes() == okb.tobytes() and cym.tobytes() == cyb.tobytes() and stm.tobytes() == stb.tobytes()


# ---------------------------------------------------------------- entries reached through a group; the chunk loop
@pytest.fixture(scope="module")
def small_map(built):
    """The 13 x 70 random map of test_plumbing (kernels 9 / 8 on it)."""
    import svsdf_amd
    g = layout("random", 13, 70, seed=7)
    return g, svsdf_amd.OccupancyMap(cloud_of(g, 1.0), resolution=1.0, sta_threshold=2)


def test_entries_through_a_group(ctxs, small_map):
    """svsdf_check_sub_sw_collision and svsdf_shape_kernels on a multi-device context run on its first stripe: the same
    bytes as a single-device context.  An entry that fails there hands the stripe's error text to the group."""
    import svsdf_amd
    g, om = small_map
    single = ctxs("star")
    multi = svsdf_amd.SvsdfContext(shape="star", devices=[0, 0])
    with pytest.raises(svsdf_amd.SvsdfError, match="no map"):      # before any frontend_set_map on the group
        multi.astar_search([0.5, 0.5, 0.5], [12.5, 69.5, 0.5])
    # three edges with 0, 1 and 70 obstacle points: the occupied cells' centres, nearest to the father first
    ii, jj = np.nonzero(g)
    cen = np.column_stack([ii + 0.5, jj + 0.5])
    father = np.array([6.5, 30.5, 0.0])
    near = cen[np.argsort(np.hypot(cen[:, 0] - father[0], cen[:, 1] - father[1]), kind="stable")]
    assert len(near) >= 70
    fs = np.tile(father, (3, 1))
    cs = np.array([[7.5, 31.5, 0.4], [7.5, 30.5, -0.8], [5.5, 29.5, 2.0]])
    pts = [np.zeros((0, 2)), near[-1:], near[:70]]
    want = single.check_sub_sw_collision(fs, cs, pts)
    got = multi.check_sub_sw_collision(fs, cs, pts)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert want[0]                                                 # no point: nothing to collide with
    ms, bs, ys, ns = single.shape_kernels(9, 8, 1.0, 0.5)
    mm, bm, ym, nm = multi.shape_kernels(9, 8, 1.0, 0.5)
    assert mm.tobytes() == ms.tobytes() and bm.tobytes() == bs.tobytes() and ym.tobytes() == ys.tobytes() and nm == ns
    assert ms.any() and not ms.all()
    multi.frontend_set_map(om, 9, 8, MARGIN)
    assert multi.astar_search([0.5, 0.5, 0.5], [12.5, 69.5, 0.5])["status"] in ("FOUND", "EXHAUSTED")
    multi.close()


def test_successors_chunk_loop(ctxs, small_map):
    """More than 2^18 parents in one call go to the device in chunks of 2^18: the same bytes as the chunks sent as calls
    of their own, and as the parents at both sides of the boundary sent alone."""
    g, om = small_map
    ctx = ctxs("star")
    ctx.frontend_set_map(om, 9, 8, MARGIN)
    chunk = 1 << 18
    n = chunk + 3
    free = np.argwhere(~g).astype(np.int32)
    reps = -(-n // len(free))
    ij = np.tile(free, (reps, 1))[:n]
    hy = handout_yaws(8)
    yw = np.array([hy[k % 8] for k in range(5)] * (n // 5 + 1))[:n]          # period 5 against the cells' period
    ok, cy, st = ctx.astar_successors(ij, yw)
    assert ok.shape == (n, 9) and cy.shape == (n, 9) and st.shape == (n, 9)
    ok0, cy0, st0 = ctx.astar_successors(ij[:chunk], yw[:chunk])
    ok1, cy1, st1 = ctx.astar_successors(ij[chunk:], yw[chunk:])
    assert ok.tobytes() == ok0.tobytes() + ok1.tobytes()
    assert cy.tobytes() == cy0.tobytes() + cy1.tobytes()
    assert st.tobytes() == st0.tobytes() + st1.tobytes()
    for p in (0, chunk - 1, chunk, chunk + 2):
        okp, cyp, stp = ctx.astar_successors(ij[p:p + 1], yw[p:p + 1])
        assert okp.tobytes() == ok[p:p + 1].tobytes() and cyp.tobytes() == cy[p:p + 1].tobytes() \
            and stp.tobytes() == st[p:p + 1].tobytes()
    print("stages 0..4:", np.bincount(st.ravel(), minlength=5).tolist())
