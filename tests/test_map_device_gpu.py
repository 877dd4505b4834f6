"""The producer on the device (svsdf_map_build_device, svsdf_frontend_set_map_device, svsdf_set_points_from_map) against
the host producer (svsdf_amd.OccupancyMap), the oracle's orc_map_points and a numpy restatement of the host counting loop:
every step bit for bit, on four synthetic clouds and the three demo maps, plus the edge cases."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import orc

ASSETS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_assets.json")))
KS, KC, MARGIN = 17, 18, 0.5        # the yaml's kernel_size / kernel_yaw_num (tests/test_frontend_succ_gpu.py)

# name: (extent, n, resolution, sta_threshold, dims, gathered); dims and gathered are what the host map and the oracle give
# (test_the_synthetic_clouds_are_the_listed_ones).  S1 the basic case; S2 a threshold above 1 with cells on both sides of it;
# S3: Y + 2 side = 177 crosses two 64-bit word boundaries, Z > 1, many blocks; S4 one point past a 256-thread block.
SYNTH = {
    "S1": ((12.0, 20.0, 3.0), 700, 1.0, 1, (12, 20, 3), 424),
    "S2": ((12.0, 20.0, 3.0), 1500, 1.0, 2, (12, 20, 3), 397),
    "S3": ((16.3, 40.1, 0.9), 20000, 0.25, 1, (66, 161, 4), 890),
    "S4": ((30.5, 75.0, 2.0), 257, 1.0, 1, (31, 75, 2), 60),
}
DEMOS = ["star", "sdHorseshoe", "sdHeart"]


@functools.lru_cache(maxsize=None)
def _clouds():
    """S1 - S4 in order from one generator; read-only."""
    rng = np.random.default_rng(20240807)
    out = {}
    for name, (extent, n, _, _, _, _) in SYNTH.items():
        c = (rng.random((n, 3)) * np.array(extent)).astype(np.float32)
        c.setflags(write=False)
        out[name] = c
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cloud, resolution, threshold, centres, halfbd) of a synthetic cloud or a demo map."""
    if name in SYNTH:
        extent, _, res, thr, _, _ = SYNTH[name]
        ex = np.array(extent)
        centres = np.array([[f * ex[0], f * ex[1], 0.4] for f in (0.1, 0.3, 0.3, 0.55, 0.8)] + [[ex[0] + 5, ex[1] + 5, 0.4]])
        return _clouds()[name], res, thr, centres, np.full(3, 17 * res / 3)
    from svsdf_amd import workload
    sc = ASSETS["scenarios"][name]
    cloud = np.array(ASSETS["maps"][name], dtype=np.float32)
    q = workload.waypoints(sc["start"][:2], sc["end"][:2], 8)
    halfbd = np.full(3, sc["kernel_size"] * sc["occupancy_resolution"] / 3.0)   # plan_manager.cpp:57-59,165
    return cloud, sc["occupancy_resolution"], 1, q, halfbd


@functools.lru_cache(maxsize=None)
def _host(name):
    """The host route's results, computed once: info, gather, the oracle's points and dims."""
    import svsdf_amd
    cloud, res, thr, centres, halfbd = _case(name)
    m = svsdf_amd.OccupancyMap(cloud, res, thr)
    opts, odims = orc.map_points(cloud, centres, halfbd, res, thr)
    pts = m.gather(centres, halfbd)
    pts.setflags(write=False)
    return m.info(), pts, opts, odims


def _counts(cloud, res):
    """The host counting loop (PCSmap_manager.cpp:116-160, Gridmap3D.cpp:137-177) in numpy: bounds, dims, points per cell."""
    c = cloud.astype(np.float64).reshape(-1, 3)
    bmin = np.minimum(c.min(axis=0), 999999999.0) if len(c) else np.full(3, 999999999.0)
    bmax = np.maximum(c.max(axis=0), -999999999.0) if len(c) else np.full(3, -999999999.0)
    dims = np.ceil((bmax - bmin) / res).astype(np.int64)
    cnt = np.zeros(np.maximum(dims, 0), dtype=np.int64)
    if cnt.size:
        idx = np.floor((c - bmin) / res).astype(np.int64)
        idx = np.minimum(np.maximum(idx, 0), dims - 1)
        np.add.at(cnt, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    return bmin, bmax, tuple(int(d) for d in dims), cnt


def _ctx(**kw):
    import svsdf_amd
    kw.setdefault("device", 0)
    return svsdf_amd.SvsdfContext(shape="star", **kw)


@pytest.mark.parametrize("name", list(SYNTH))
def test_the_synthetic_clouds_are_the_listed_ones(built, name):
    """No GPU: the host map and the oracle on S1 - S4 give the dims and gathered counts the cases were chosen for."""
    info, pts, opts, odims = _host(name)
    _, n, _, _, dims, gathered = SYNTH[name]
    assert len(_clouds()[name]) == n
    assert info["dims"] == dims == odims
    assert len(pts) == len(opts) == gathered
    assert len(np.unique(pts, axis=0)) == len(pts)
    assert 0 < info["occupied"] < dims[0] * dims[1] * dims[2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SYNTH) + DEMOS)
def test_build_and_gather_match_the_host_and_the_oracle(built, name):
    cloud, res, thr, centres, halfbd = _case(name)
    info, pts, opts, odims = _host(name)
    ctx = _ctx()
    ctx.map_build(cloud, res, thr)
    mi = ctx.map_info()
    # 1. geometry and occupied count
    assert mi["dims"] == info["dims"] == odims
    np.testing.assert_array_equal(mi["bmin"], info["bmin"])
    np.testing.assert_array_equal(mi["bmax"], info["bmax"])
    assert mi["occupied"] == info["occupied"] and mi["n_cloud"] == len(cloud)
    assert mi["resolution"] == res and mi["sta_threshold"] == thr and mi["gathered"] == 0
    # 2. cells against the counting loop
    bmin, bmax, dims, cnt = _counts(cloud, res)
    assert dims == mi["dims"]
    cells = ctx.map_cells()
    np.testing.assert_array_equal(cells, (cnt >= thr).astype(np.uint8))
    assert (cnt[cells != 0] >= thr).all() and int(cells.sum()) == mi["occupied"] > 0
    if thr > 1:
        assert ((cnt > 0) & (cnt < thr)).any()            # cells below the threshold exist, and are not occupied
    # 3. the gather
    assert ctx.map_points().shape == (0, 3)
    n = ctx.set_points_from_map(centres, halfbd)
    got = ctx.map_points()
    print(f"{name}: dims {mi['dims']} occupied {mi['occupied']} gathered {n} build_ms {mi['build_ms']:.3f}")
    np.testing.assert_array_equal(got, pts)
    np.testing.assert_array_equal(got, opts)
    assert n == len(pts) == ctx.num_points() == ctx.map_info()["gathered"] > 20
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SYNTH) + DEMOS)
def test_resident_cloud_is_the_host_routes(built, name):
    import svsdf_amd
    from svsdf_amd import workload
    cloud, res, thr, centres, halfbd = _case(name)
    _, pts, _, _ = _host(name)
    w = workload.make("C1", P=8, minco=svsdf_amd.minco_coeffs)
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], head_state=w["head_state"],
              tail_state=w["tail_state"])
    dev, twin = _ctx(**kw), _ctx(**kw)
    dev.map_build(cloud, res, thr)
    dev.set_points_from_map(centres, halfbd)
    twin.set_points(pts)
    np.testing.assert_array_equal(dev.shard_indices(), twin.shard_indices())
    a, b = dev.query_points(w["coeffs"], w["T"]), twin.query_points(w["coeffs"], w["T"])
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    assert dev.stats()["setup_ms"] >= dev.map_info()["gather_ms"] > 0.0      # setup_ms: gather plus plan
    if name == "star":
        x = workload.x_from(w["q"], w["T"], svsdf_amd.backward_T)
        (f1, g1), (f2, g2) = dev.lmbm_evaluate(x), twin.lmbm_evaluate(x)
        assert f1 == f2
        np.testing.assert_array_equal(g1, g2)
    dev.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S3", "S4", "star"])
def test_front_end_from_the_resident_map(built, name):
    import svsdf_amd
    cloud, res, thr, _, _ = _case(name)
    dev, twin = _ctx(), _ctx()
    dev.map_build(cloud, res, thr)
    dev.frontend_set_map_resident(KS, KC, MARGIN)
    twin.frontend_set_map(svsdf_amd.OccupancyMap(cloud, res, thr), KS, KC, MARGIN)
    a, b = dev.yaw_free(), twin.yaw_free()
    assert a.shape == b.shape == tuple(dev.map_info()["dims"][:2])
    np.testing.assert_array_equal(a, b)
    if name == "star":
        sc = ASSETS["scenarios"]["star"]
        ra, rb = dev.astar_search(sc["start"], sc["end"]), twin.astar_search(sc["start"], sc["end"])
        assert ra["status"] == rb["status"] == "FOUND" and ra["path_len"] == rb["path_len"] > 2
        np.testing.assert_array_equal(ra["cells"], rb["cells"])
        np.testing.assert_array_equal(ra["path"], rb["path"])
        np.testing.assert_array_equal(ra["stage_counts"], rb["stage_counts"])
        for k in ("expansions", "pushes", "relaxed_open", "reopened", "launches", "g_goal"):
            assert ra[k] == rb[k], k
    # the front-end map survives a new resident map until the next set-map call
    dev.map_build(cloud[:50], res, thr)
    np.testing.assert_array_equal(dev.yaw_free(), b)
    dev.close()
    twin.close()


@pytest.mark.gpu
def test_front_end_limits_and_messages(built):
    import svsdf_amd
    ctx = _ctx()
    with pytest.raises(svsdf_amd.SvsdfError, match="no resident map"):
        ctx.frontend_set_map_resident(KS, KC, MARGIN)
    with pytest.raises(svsdf_amd.SvsdfError, match="no resident map"):
        ctx.set_points_from_map(np.zeros((1, 3)), np.ones(3))
    with pytest.raises(svsdf_amd.SvsdfError, match="no resident map"):
        ctx.map_info()
    ctx.map_build(_clouds()["S1"], 1.0, 1)
    for ks, kc, msg in ((16, 18, "kernel_size must be odd and positive"), (65, 18, "kernel_size <= 63"),
                        (17, 65, "kernel_count <= 64"), (17, 0, "kernel_count <= 64")):
        with pytest.raises(svsdf_amd.SvsdfError, match=msg):
            ctx.frontend_set_map_resident(ks, kc, MARGIN)
    with pytest.raises(svsdf_amd.SvsdfError, match="safemargin not finite"):
        ctx.frontend_set_map_resident(KS, KC, float("nan"))
    flat = np.array(_clouds()["S1"])
    flat[:, 2] = 1.0
    ctx.map_build(flat, 1.0, 1)
    with pytest.raises(svsdf_amd.SvsdfError, match="empty map"):
        ctx.frontend_set_map_resident(KS, KC, MARGIN)
    ctx.close()
    host = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)
    for call in (lambda: host.map_build(flat, 1.0, 1), host.map_info, lambda: host.frontend_set_map_resident(KS, KC, MARGIN),
                 lambda: host.set_points_from_map(np.zeros((1, 3)), np.ones(3)), host.map_points):
        with pytest.raises(svsdf_amd.SvsdfError, match=r"\(2\)"):          # SVSDF_ERR_NO_DEVICE
            call()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_block_boundaries(built, n):
    import svsdf_amd
    rng = np.random.default_rng(n)
    cloud = (rng.random((n, 3)) * np.array([9.0, 7.0, 2.0])).astype(np.float32)
    ctx = _ctx()
    ctx.map_build(cloud, 1.0, 1)
    info = svsdf_amd.OccupancyMap(cloud, 1.0, 1).info()
    mi = ctx.map_info()
    assert mi["dims"] == info["dims"] and mi["occupied"] == info["occupied"]
    np.testing.assert_array_equal(mi["bmin"], info["bmin"])
    np.testing.assert_array_equal(mi["bmax"], info["bmax"])
    _, _, dims, cnt = _counts(cloud, 1.0)
    np.testing.assert_array_equal(ctx.map_cells(), (cnt >= 1).astype(np.uint8))
    if n == 1:
        assert mi["dims"] == (0, 0, 0) and ctx.map_cells().size == 0
    else:
        centres, halfbd = np.array([[4.0, 3.0, 1.0], [6.0, 4.0, 1.0]]), np.full(3, 2.5)
        assert ctx.set_points_from_map(centres, halfbd) == len(svsdf_amd.OccupancyMap(cloud, 1.0, 1).gather(centres, halfbd))
        np.testing.assert_array_equal(ctx.map_points(), svsdf_amd.OccupancyMap(cloud, 1.0, 1).gather(centres, halfbd))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thr,occupied", [(1, 3), (1001, 0), (1000, 1)])
def test_atomic_contention(built, thr, occupied):
    """1000 copies of one point and the two corners: every copy is counted."""
    import svsdf_amd
    cloud = np.array([[2.5, 3.5, 0.5]] * 1000 + [[0.0, 0.0, 0.0], [5.0, 6.0, 2.0]], dtype=np.float32)
    ctx = _ctx()
    ctx.map_build(cloud, 1.0, thr)
    _, _, dims, cnt = _counts(cloud, 1.0)
    assert dims == (5, 6, 2) and cnt[2, 3, 0] == 1000
    assert ctx.map_info()["occupied"] == occupied == svsdf_amd.OccupancyMap(cloud, 1.0, thr).info()["occupied"]
    np.testing.assert_array_equal(ctx.map_cells(), (cnt >= thr).astype(np.uint8))
    ctx.close()


@pytest.mark.gpu
def test_flat_and_empty_clouds(built):
    import svsdf_amd
    ctx = _ctx()
    flat = np.array(_clouds()["S1"])
    flat[:, 2] = 1.25
    ctx.map_build(flat, 1.0, 1)
    info, mi = svsdf_amd.OccupancyMap(flat, 1.0, 1).info(), ctx.map_info()
    assert mi["dims"] == info["dims"] == (12, 20, 0) and mi["occupied"] == info["occupied"] == 0
    assert ctx.map_cells().size == 0
    assert ctx.set_points_from_map(np.array([[3.0, 3.0, 1.25]]), np.ones(3)) == 0 and ctx.num_points() == 0
    ctx.map_build(np.zeros((0, 3), dtype=np.float32), 1.0, 1)
    info, mi = svsdf_amd.OccupancyMap(np.zeros((0, 3), dtype=np.float32), 1.0, 1).info(), ctx.map_info()
    assert mi["dims"] == info["dims"] and mi["dims"][0] < 0 and mi["occupied"] == info["occupied"] == 0
    np.testing.assert_array_equal(mi["bmin"], info["bmin"])
    np.testing.assert_array_equal(mi["bmax"], info["bmax"])
    assert mi["n_cloud"] == 0 and ctx.map_cells().size == 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_coordinate_is_refused(built, bad):
    import svsdf_amd
    cloud = np.array(_clouds()["S1"])
    cloud[413, 1] = bad
    ctx = _ctx()
    ctx.map_build(_clouds()["S4"], 1.0, 1)
    with pytest.raises(svsdf_amd.SvsdfError, match="1 non-finite coordinate"):
        ctx.map_build(cloud, 1.0, 1)
    with pytest.raises(svsdf_amd.SvsdfError, match="no resident map"):     # the earlier map went with the failed call
        ctx.map_info()
    with pytest.raises(svsdf_amd.SvsdfError, match="resolution"):
        ctx.map_build(_clouds()["S4"], 0.0, 1)
    with pytest.raises(svsdf_amd.SvsdfError, match="2\\^31 - 1"):
        ctx.map_build(_clouds()["S4"], 0.001, 1)                            # 30 500 x 75 000 x 2 000 cells
    ctx.close()


@pytest.mark.gpu
def test_no_centres_and_a_centre_outside(built):
    import svsdf_amd
    cloud, res, thr, centres, halfbd = _case("S1")
    ctx = _ctx()
    ctx.map_build(cloud, res, thr)
    ctx.set_points_from_map(centres, halfbd)
    assert ctx.num_points() > 0
    assert ctx.set_points_from_map(np.zeros((0, 3)), halfbd) == 0
    assert ctx.num_points() == 0 and ctx.map_points().shape == (0, 3) and ctx.map_info()["gathered"] == 0
    w = svsdf_amd.workload.make("C1", P=8, minco=svsdf_amd.minco_coeffs)
    assert all(len(v) == 0 for v in ctx.query_points(w["coeffs"], w["T"]))   # a valid empty cloud
    host = svsdf_amd.OccupancyMap(cloud, res, thr)
    for outside in ([40.0, 50.0, 0.4], [-30.0, 5.0, 0.4], [6.0, 10.0, 50.0]):
        ref = host.gather(np.array([outside]), halfbd)
        assert ctx.set_points_from_map(np.array([outside]), halfbd) == len(ref)
        np.testing.assert_array_equal(ctx.map_points(), ref)
    with pytest.raises(svsdf_amd.SvsdfError, match="non-finite centre"):
        ctx.set_points_from_map(np.array([[1.0, float("nan"), 0.4]]), halfbd)
    ctx.close()


@pytest.mark.gpu
def test_two_stripes_on_one_device(built):
    import svsdf_amd
    from svsdf_amd import workload
    cloud, res, thr, centres, halfbd = _case("S3")
    w = workload.make("C1", P=8, minco=svsdf_amd.minco_coeffs)
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], head_state=w["head_state"],
              tail_state=w["tail_state"])
    single = _ctx(**kw)
    group = svsdf_amd.SvsdfContext(shape="star", devices=[0, 0], **kw)
    for c in (single, group):
        c.map_build(cloud, res, thr)
        assert c.set_points_from_map(centres, halfbd) == len(_host("S3")[1])
    assert group.group_info()["n_devices"] == 2 and group.num_points() == single.num_points()
    np.testing.assert_array_equal(group.map_points(), single.map_points())
    a, b = single.query_points(w["coeffs"], w["T"]), group.query_points(w["coeffs"], w["T"])
    np.testing.assert_array_equal(a[3], np.arange(single.num_points()))
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    single.close()
    group.close()


@pytest.mark.gpu
def test_device_tensor_input(built):
    import torch
    cloud, res, thr, centres, halfbd = _case("S3")
    a, b = _ctx(), _ctx()
    a.map_build(cloud, res, thr)
    t = torch.from_numpy(np.array(cloud)).to("cuda:0")
    b.map_build(t, res, thr)
    torch.cuda.synchronize()
    ia, ib = a.map_info(), b.map_info()
    assert ia["dims"] == ib["dims"] and ia["occupied"] == ib["occupied"]
    np.testing.assert_array_equal(a.map_cells(), b.map_cells())
    assert a.set_points_from_map(centres, halfbd) == b.set_points_from_map(centres, halfbd)
    np.testing.assert_array_equal(a.map_points(), b.map_points())
    a.close()
    b.close()


@pytest.mark.gpu
def test_allocations_go_with_the_map_and_the_context(built):
    import svsdf_amd
    cloud, res, thr, centres, halfbd = _case("S1")
    before = svsdf_amd.live_allocations()
    ctx = _ctx()
    created = svsdf_amd.live_allocations()
    ctx.map_build(cloud, res, thr)
    with_map = svsdf_amd.live_allocations()
    assert with_map[0] == created[0] + 1 and with_map[1] == created[1] + 12 * 20 * 3      # the occupancy bytes alone stay
    ctx.map_build(cloud, res, thr)
    assert svsdf_amd.live_allocations() == with_map                                      # a rebuild replaces
    ctx.frontend_set_map_resident(KS, KC, MARGIN)
    ctx.set_points_from_map(centres, halfbd)
    ctx.close()
    assert svsdf_amd.live_allocations() == before
