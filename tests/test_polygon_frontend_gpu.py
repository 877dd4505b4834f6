"""The front end on a Polygon context created with SVSDF_FLAG_POLYGON_YAW_KERNELS: svsdf_shape_kernels, the yaw-free
table, svsdf_astar_successors and svsdf_astar_search / svsdf_astar_nodes against the expected values composed in
tests/polygon_frontend.py from the oracle's one-argument Polygon::getonlySDF and the existing restatements.  Bytes, words,
stages, booleans, counters and the bits of every yaw, g and f must be equal.  Every test first re-asserts, from the oracle
alone, that its inputs are admissible (polygon_frontend: no kernel cell within 1e-9 of the margin, the same expected result
with libm and with device-library trig, mixed tables, all five stages or a named exception)."""
import math

import numpy as np
import pytest

import astar_restatement as ar
import polygon_frontend as pf

pytestmark = pytest.mark.gpu

REFUSALS = {
    "shape_kernels": "svsdf_shape_kernels: Polygon has no getonlySDF(pos_rel, Matrix3d) in the reference (Shape.hpp:1477)",
    "frontend_set_map": "svsdf_frontend_set_map: Polygon has no getonlySDF(pos_rel, Matrix3d) in the reference "
                        "(Shape.hpp:1477), so no yaw kernels",
}


@pytest.fixture(scope="module")
def resident(built):
    """One flagged context per robot; a case's map is made resident only when the context holds another one."""
    import svsdf_amd
    ctxs, held = {}, {}

    def get(name, case=None):
        if name not in ctxs:
            ctxs[name] = pf.robot(name).context(svsdf_amd, device=0)
        ctx = ctxs[name]
        if case is not None and held.get(name) is not case:
            ctx.frontend_set_map(case.device_map(svsdf_amd), case.ks, case.count, case.margin)
            held[name] = case
        return ctx
    return get


# ---------------------------------------------------------------- svsdf_shape_kernels
@pytest.mark.parametrize("name,ks,count,res,margin", pf.KERNEL_CASES)
def test_shape_kernels(resident, name, ks, count, res, margin):
    occ, by, yaws, n, gap = pf.expected_kernels(name, ks, count, res, margin)
    assert gap >= pf.MIN_GAP and occ.any() and not occ.all()
    m, b, y, loops = resident(name).shape_kernels(ks, count, res, margin)
    assert m.shape == occ.shape and b.shape == by.shape
    bad = np.argwhere(m != occ)
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert b.tobytes() == by.tobytes()
    assert pf.same_bits(y, yaws) and loops == n


# ---------------------------------------------------------------- the yaw-free table
@pytest.mark.parametrize("name", ["bar", "L"])
@pytest.mark.parametrize("ks,count", pf.GRID_KERNELS)
@pytest.mark.parametrize("X,Y", pf.GRIDS)
def test_yaw_free_table_synthetic(resident, X, Y, ks, count, name):
    for lay in pf.LAYOUTS:
        c = pf.grid_table_case(name, X, Y, ks, count, lay)
        assert c.gap >= pf.MIN_GAP
        assert c.table_kind() == pf.expected_table_kind(name, X, Y, ks, lay), (lay, c.table_kind())
        got = resident(name, c).yaw_free()
        assert got.shape == (X, Y) and got.dtype == np.uint64
        np.testing.assert_array_equal(got, c.free, err_msg=f"{lay} {X}x{Y} {name} {ks}/{count}")


@pytest.mark.parametrize("name,map_name", pf.SUCCESSOR_CASES + [("mesh", "star"), ("ring", "star")])
def test_yaw_free_table_on_reference_maps(resident, name, map_name):
    import svsdf_amd
    c = pf.demo_case(name, map_name)
    assert c.gap >= pf.MIN_GAP and c.table_kind() == "mixed"
    info = c.device_map(svsdf_amd).info()
    assert info["dims"] == c.occ.shape
    np.testing.assert_array_equal(resident(name, c).yaw_free(), c.free)


# ---------------------------------------------------------------- svsdf_astar_successors
@pytest.mark.parametrize("name,map_name", pf.SUCCESSOR_CASES)
def test_successors_on_reference_maps(resident, name, map_name):
    c, s = pf.assert_successors_admissible(name, map_name)
    ok, cyaw, stage = resident(name, c).astar_successors(s["parents"], s["yaws"])
    print(name, map_name, "stages 0..4:", np.bincount(s["stage"].ravel(), minlength=5).tolist())
    np.testing.assert_array_equal(stage, s["stage"])
    np.testing.assert_array_equal(ok, s["ok"])
    np.testing.assert_array_equal(ok, stage == 0)
    assert pf.same_bits(cyaw, s["cyaw"])        # NaN where no yaw was chosen, on both sides
    assert np.isnan(cyaw[(stage != 0) & (stage != 4)]).all() and not np.isnan(cyaw[(stage == 0) | (stage == 4)]).any()


@pytest.mark.parametrize("name", ["bar", "L"])
def test_successors_agree_with_check_sub_sw_collision(resident, name):
    """The accepted and the stage-4 slots of map `star` through the other shipped path: svsdf_check_sub_sw_collision
    (k_subsw<Polygon>) fed with the returned child yaws and host-gathered points."""
    import svsdf_amd
    c, s = pf.assert_successors_admissible(name, "star")
    om = c.device_map(svsdf_amd)
    ctx = resident(name, c)
    ok, cyaw, stage = ctx.astar_successors(s["parents"], s["yaws"])
    bmin, half = c.bmin, float(c.ks // 2 + 1)
    fs, cs, pts, want = [], [], [], []
    for p, sl in zip(*np.nonzero((stage == 0) | (stage == 4))):
        pi, pj = s["parents"][p]
        vi, vj = pi + sl // 3 - 1, pj + sl % 3 - 1
        centre = np.array([vi + 0.5 + bmin[0], vj + 0.5 + bmin[1], 0.0])
        g = om.gather(centre[None], [half, half, 0.0])
        fs.append([pi + 0.5 + bmin[0], pj + 0.5 + bmin[1], s["yaws"][p]])
        cs.append([centre[0], centre[1], cyaw[p, sl]])
        pts.append(g[np.abs(g[:, 2] - (0.5 + bmin[2])) < 1e-9][:, :2])     # the box is one layer thick: layer 0
        want.append(ok[p, sl])
    got = ctx.check_sub_sw_collision(np.array(fs), np.array(cs), pts)
    np.testing.assert_array_equal(got, np.array(want))
    assert any(want) and not all(want)


# ---------------------------------------------------------------- svsdf_astar_search / svsdf_astar_nodes
def _device(ctx, start, end, **kw):
    r = ctx.astar_search(start, end, **kw)
    r.update(ctx.astar_nodes())
    return r


def _equal(dev, ref, what, slice_=256):
    assert ar.same_search(dev, ref) == [], (what, {k: (dev[k], ref[k]) for k in ("status", "path_len") + ar.COUNTERS})
    pops = ref["expansions"] + (1 if ref["status"] == "FOUND" else 0)
    assert dev["launches"] == math.ceil(pops / slice_), (what, dev["launches"], pops, slice_)
    assert dev["path"].shape == (ref["path_len"], 3)
    assert int(dev["stage_counts"].sum()) == 9 * dev["expansions"]


@pytest.mark.parametrize("key", sorted(pf.SEARCH_CASES))
def test_search(resident, key):
    c, start, end, kw, ref = pf.search_case(key)
    want = pf.SEARCH_CASES[key]
    assert (ref["status"], ref["path_len"]) == (want["status"], want["path_len"])
    dev = _device(resident(c.shape, c), start, end, **kw)
    print(key, {k: dev[k] for k in ("status", "path_len", "launches") + ar.COUNTERS}, dev["stage_counts"].tolist())
    _equal(dev, ref, key)
    if "max_expansions" in kw:
        assert dev["expansions"] == kw["max_expansions"]
        c2, s2, e2, _, ref2 = pf.search_case(key.replace(" limit %d" % kw["max_expansions"], " forward"))
        _equal(_device(resident(c.shape, c), s2, e2), ref2, "unlimited after limited")      # the state is reset per search


def test_slices_give_identical_bytes(resident):
    c, start, end, kw, ref = pf.search_case("bar star forward")
    ctx = resident("bar", c)
    base = _device(ctx, start, end, slice=256)
    _equal(base, ref, 256)
    for sl in (1, 7):
        dev = _device(ctx, start, end, slice=sl)
        _equal(dev, ref, sl, sl)
        for k in ("path", "cells", "stage_counts") + ar.NODE_KEYS:
            assert dev[k].tobytes() == base[k].tobytes(), (sl, k)


# ---------------------------------------------------------------- plumbing
def test_without_the_flag_the_polygon_is_refused(built):
    import svsdf_amd
    c = pf.demo_case("bar", "star")
    ctx = pf.robot("bar").context(svsdf_amd, flags=0, device=0)
    with pytest.raises(svsdf_amd.SvsdfError) as e:
        ctx.shape_kernels(17, 18, 1.0, 0.5)
    assert REFUSALS["shape_kernels"] in str(e.value)
    with pytest.raises(svsdf_amd.SvsdfError) as e:
        ctx.frontend_set_map(c.device_map(svsdf_amd), 17, 18, 0.5)
    assert REFUSALS["frontend_set_map"] in str(e.value)
    for call in (lambda: ctx.yaw_free(), lambda: ctx.astar_successors([[3, 3]], [0.0]), lambda: ctx.astar_search(c.start, c.end)):
        with pytest.raises(svsdf_amd.SvsdfError, match="no map"):
            call()
    ctx.close()


def test_the_flag_changes_nothing_for_an_analytic_shape(built):
    import svsdf_amd
    c = ar.demo_case("star")
    out = []
    for flags in (0, svsdf_amd.FLAG_POLYGON_YAW_KERNELS):
        ctx = svsdf_amd.SvsdfContext(shape="star", device=0, flags=flags)
        k = ctx.shape_kernels(17, 18, 1.0, 0.5)
        ctx.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, ar.MARGIN)
        r = _device(ctx, c.start, c.end)
        out.append([np.asarray(a).tobytes() for a in k[:3]] + [k[3], ctx.yaw_free().tobytes(), r["status"], r["expansions"]] +
                   [r[key].tobytes() for key in ("path", "cells", "stage_counts") + ar.NODE_KEYS])
        ctx.close()
    assert out[0] == out[1] and out[0][5] == "FOUND"


def test_group_context_and_allocations(resident):
    """devices=[0, 0] gives the bytes of one device; a closed flagged Polygon context returns every allocation."""
    import svsdf_amd
    c, start, end, kw, ref = pf.search_case("bar star forward")
    s = pf.demo_successors("bar", "star")
    single = resident("bar", c)
    want = [a.tobytes() for a in single.astar_successors(s["parents"], s["yaws"])]
    base = _device(single, start, end)
    before = svsdf_amd.live_allocations()
    multi = pf.robot("bar").context(svsdf_amd, devices=[0, 0])
    assert [np.asarray(a).tobytes() for a in multi.shape_kernels(17, 18, 1.0, 0.5)[:3]] == \
        [np.asarray(a).tobytes() for a in single.shape_kernels(17, 18, 1.0, 0.5)[:3]]
    multi.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, c.margin)
    assert multi.yaw_free().tobytes() == c.free.tobytes()
    assert [a.tobytes() for a in multi.astar_successors(s["parents"], s["yaws"])] == want
    m = _device(multi, start, end)
    for k in ("path", "cells", "stage_counts") + ar.NODE_KEYS:
        assert m[k].tobytes() == base[k].tobytes(), k
    multi.close()
    assert svsdf_amd.live_allocations() == before
    one = pf.robot("L").context(svsdf_amd, device=0)
    one.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, c.margin)
    one.astar_search(start, end, max_expansions=5)
    one.close()
    assert svsdf_amd.live_allocations() == before


def test_traj_optimizer_reaches_a_path_for_a_mesh(built, tmp_path):
    """TrajOptimizer(polygon_front_end=True) on a mesh `inputdata` the shape registry does not know: its context plans a
    path; without the option the same context refuses the map."""
    import svsdf_amd
    bar = pf.robot("bar")
    V, F = pf._extrude([bar.xy])
    obj = tmp_path / "bar_robot.obj"
    obj.write_text("".join("v %.17g %.17g %.17g\n" % tuple(v) for v in V) + "".join("f %d %d %d\n" % tuple(f + 1) for f in F))
    c, start, end, kw, ref = pf.search_case("bar star forward")
    for on in (False, True):
        opt = svsdf_amd.TrajOptimizer(polygon_front_end=on)
        opt.setParam({"inputdata": str(obj), "device": 0})
        opt.setConditions(np.zeros((3, 3)), np.zeros((3, 3)), 4)
        opt.setPoints(np.array([[100.0, 100.0, 0.0]]))
        ctx = opt._context()
        if not on:
            with pytest.raises(svsdf_amd.SvsdfError, match="Polygon"):
                ctx.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, c.margin)
            continue
        ctx.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, c.margin)
        r = ctx.astar_search(start, end)
        assert r["status"] == "FOUND" and r["path_len"] > 1
        assert tuple(r["cells"][0]) == tuple(ref["cells"][0]) and tuple(r["cells"][-1]) == tuple(ref["cells"][-1])
