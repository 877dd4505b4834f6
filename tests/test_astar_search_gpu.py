"""svsdf_astar_search / svsdf_astar_nodes (the device A* search on the resident front-end map, k_astar<SHAPE>) against the
plain-Python restatement of AstarPathSearch + getPath (tests/astar_restatement.py, itself checked on the CPU by
tests/test_astar_restatement.py).  Everything must be equal: status, cells, the bits of the path, every counter, the
stage histogram, and from the node records id, father_cell and the bits of g, f and yaw."""
import ctypes as C
import math

import numpy as np
import pytest

import astar_restatement as ar

pytestmark = pytest.mark.gpu

DEMOS = ["star", "sdHorseshoe", "sdHeart"]
DEFAULT_SLICE = 256


@pytest.fixture(scope="module")
def resident(built):
    """One context per shape; the map of a case is made resident only when the context holds another one."""
    import svsdf_amd
    ctxs, held = {}, {}

    def get(case):
        if case.shape not in ctxs:
            ctxs[case.shape] = svsdf_amd.SvsdfContext(shape=case.shape, device=0)
        ctx = ctxs[case.shape]
        if held.get(case.shape) is not case:
            ctx.frontend_set_map(case.device_map(svsdf_amd), case.ks, case.count, ar.MARGIN)
            held[case.shape] = case
        return ctx
    return get


def _device(ctx, start, end, **kw):
    r = ctx.astar_search(start, end, **kw)
    if r["status"] != "OUT_OF_MAP":
        r.update(ctx.astar_nodes())
    return r


def _pops(r):
    return r["expansions"] + (1 if r["status"] == "FOUND" else 0)


def _equal(dev, ref, what, slice_=DEFAULT_SLICE):
    assert ar.same_search(dev, ref) == [], (what, {k: (dev[k], ref[k]) for k in ("status", "path_len") + ar.COUNTERS})
    assert dev["launches"] == math.ceil(_pops(ref) / slice_), (what, dev["launches"], _pops(ref), slice_)
    assert dev["path"].shape == (ref["path_len"], 3) and dev["cells"].dtype == np.int32


# ---------------------------------------------------------------- case 1 / 2: the demo scenarios, both directions
@pytest.mark.parametrize("name", DEMOS)
def test_demo_forward(resident, name):
    c = ar.demo_case(name)
    ref = c.search(c.start, c.end)
    dev = _device(resident(c), c.start, c.end)
    print(name, {k: dev[k] for k in ("status", "path_len", "launches") + ar.COUNTERS}, dev["stage_counts"].tolist())
    _equal(dev, ref, name)
    assert dev["status"] == "FOUND" and dev["relaxed_open"] > 0 and dev["reopened"] > 0      # all three id branches ran
    assert int(dev["stage_counts"].sum()) == 9 * dev["expansions"]


@pytest.mark.parametrize("name", DEMOS)
def test_demo_reverse(resident, name):
    c = ar.demo_case(name)
    ref = c.search(c.end, c.start)
    dev = _device(resident(c), c.end, c.start)
    print(name, {k: dev[k] for k in ("status", "path_len", "launches") + ar.COUNTERS})
    _equal(dev, ref, name)
    if name != "star":
        assert dev["status"] == "EXHAUSTED" and dev["path_len"] == 0 and dev["g_goal"] == 0.0


# ---------------------------------------------------------------- case 3: the smallest grids that can go wrong
@pytest.mark.parametrize("shape", ["sdHorseshoe", "star"])
def test_sparse_grid_with_tied_keys(resident, shape):
    c = ar.grid_case(shape, 9, 8, 1.0, ar.sparse_grid(0.03, 1))
    s, e = c.centre((1, 1)), c.centre((11, 68))
    ref = c.search(s, e)
    assert ref["ties"] > 0 and ref["reopened"] > 0
    _equal(_device(resident(c), s, e), ref, shape)


def test_small_grids(resident):
    c = ar.grid_case("star", 9, 8, 1.0, ar.sparse_grid(0.06, 2))
    s, e = c.centre((1, 1)), c.centre((11, 68))
    dev = _device(resident(c), s, e)
    _equal(dev, c.search(s, e), "blocked start")
    assert (dev["status"], dev["expansions"]) == ("EXHAUSTED", 1)
    c = ar.grid_case("star", 3, 2, 1.0, np.zeros((5, 11), dtype=bool))
    s, e = c.centre((0, 0)), c.centre((4, 10))
    dev = _device(resident(c), s, e)
    _equal(dev, c.search(s, e), "5 x 11")
    assert (dev["path_len"], dev["expansions"], dev["pushes"]) == (11, 10, 31)
    s = c.centre((2, 3))                                             # start == goal: one cell, no expansion, one launch
    dev = _device(resident(c), s, s)
    _equal(dev, c.search(s, s), "start == goal")
    assert (dev["status"], dev["path_len"], dev["expansions"], dev["launches"]) == ("FOUND", 1, 0, 1)
    c = ar.grid_case("star", 3, 2, 0.25, np.zeros((65, 129), dtype=bool))
    s, e = c.centre((0, 0)), c.centre((64, 100))
    ref = c.search(s, e)
    assert ref["max_open"] == 291                                    # more entries than half a workgroup has threads
    dev = _device(resident(c), s, e)
    _equal(dev, ref, "65 x 129")
    assert dev["path_len"] == 101


# ---------------------------------------------------------------- case 4: slicing
@pytest.mark.parametrize("name,reverse", [("star", False), ("sdHorseshoe", True)])
def test_slices_give_identical_bytes(resident, name, reverse):
    c = ar.demo_case(name)
    s, e = (c.end, c.start) if reverse else (c.start, c.end)
    ref = c.search(s, e)
    ctx = resident(c)
    base = _device(ctx, s, e)
    _equal(base, ref, name)
    for sl in (1, 7, 100):
        dev = _device(ctx, s, e, slice=sl)
        _equal(dev, ref, (name, sl), sl)
        for k in ("path", "cells", "stage_counts") + ar.NODE_KEYS:
            assert dev[k].tobytes() == base[k].tobytes(), (sl, k)


# ---------------------------------------------------------------- case 5: the expansion limit
@pytest.mark.parametrize("k", [1, 50, 500])
def test_limit(resident, k):
    c = ar.demo_case("star")
    ctx = resident(c)
    ref = c.search(c.start, c.end, max_expansions=k)
    dev = _device(ctx, c.start, c.end, max_expansions=k)
    _equal(dev, ref, k)
    assert dev["status"] == "LIMIT" and dev["expansions"] == k and dev["path_len"] == 0
    _equal(_device(ctx, c.start, c.end), c.search(c.start, c.end), "unlimited after limited")      # state is reset per search


# ---------------------------------------------------------------- case 6: plumbing
def test_plumbing(built):
    import svsdf_amd
    from svsdf_amd import binding
    from test_frontend_succ import handout_yaws
    c = ar.demo_case("star")
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0)
    with pytest.raises(svsdf_amd.SvsdfError, match="no map"):
        ctx.astar_search(c.start, c.end)
    with pytest.raises(svsdf_amd.SvsdfError, match="no map"):
        ctx.astar_nodes()
    ctx.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, ar.MARGIN)
    with pytest.raises(svsdf_amd.SvsdfError, match="no search"):
        ctx.astar_nodes()
    ref = c.search(c.start, c.end)
    # outside the map: a status, not an error; nothing is launched
    for s, e in (([c.bmax[0] + 1.0, c.start[1], 0.0], c.end), (c.start, [c.end[0], c.bmin[1] - 0.5, 0.0])):
        r = ctx.astar_search(s, e)
        assert (r["status"], r["path_len"], r["launches"], r["expansions"]) == ("OUT_OF_MAP", 0, 0, 0)
    # refused arguments
    with pytest.raises(svsdf_amd.SvsdfError, match="start_yaw"):
        ctx.astar_search(c.start, c.end, start_yaw=3.1415926536)
    with pytest.raises(svsdf_amd.SvsdfError, match="slice"):
        ctx.astar_search(c.start, c.end, slice=-1)
    with pytest.raises(svsdf_amd.SvsdfError, match="not finite"):
        ctx.astar_search([float("nan"), 1.0, 0.0], c.end)
    L = svsdf_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    s3, e3 = np.array(c.start), np.array(c.end)
    res = binding.AstarResult()
    res.struct_size = C.sizeof(binding.AstarResult) - 8
    assert L.svsdf_astar_search(ctx.ctx, dp(s3), dp(e3), None, None, None, 0, C.byref(res)) == 1
    res.struct_size = C.sizeof(binding.AstarResult)
    prm = binding.AstarParams()
    L.svsdf_astar_params_default(C.byref(prm))
    prm.struct_size -= 4
    assert L.svsdf_astar_search(ctx.ctx, dp(s3), dp(e3), C.byref(prm), None, None, 0, C.byref(res)) == 1
    assert b"struct_size" in L.svsdf_last_error_string(ctx.ctx)
    # the query-then-fetch idiom (params = NULL: the defaults), and a capacity that is too small in between
    assert L.svsdf_astar_search(ctx.ctx, dp(s3), dp(e3), None, None, None, 0, C.byref(res)) == 0
    n = int(res.path_len)
    assert n == ref["path_len"] and res.status == 0 and res.expansions == ref["expansions"]
    path, cells = np.zeros((n, 3)), np.zeros((n, 2), dtype=np.int32)
    ip = cells.ctypes.data_as(C.POINTER(C.c_int))
    res2 = binding.AstarResult()
    res2.struct_size = C.sizeof(binding.AstarResult)
    assert L.svsdf_astar_search(ctx.ctx, dp(s3), dp(e3), None, dp(path), ip, n - 1, C.byref(res2)) == 1
    assert b"capacity" in L.svsdf_last_error_string(ctx.ctx)
    assert res2.path_len == n and res2.expansions == ref["expansions"] and not path.any()
    assert ar.same_search(dict(ref, **ctx.astar_nodes()), ref) == []          # the state stays readable
    assert L.svsdf_astar_search(ctx.ctx, dp(s3), dp(e3), None, dp(path), ip, n, C.byref(res2)) == 0
    assert path.tobytes() == ref["path"].tobytes() and cells.tobytes() == ref["cells"].tobytes()
    with pytest.raises(svsdf_amd.SvsdfError, match="capacity"):
        ctx.astar_search(c.start, c.end, capacity=3)
    # two searches back to back; a start yaw other than 0
    a, b = _device(ctx, c.start, c.end), _device(ctx, c.start, c.end)
    _equal(a, ref, "first")
    for k in ("path", "cells", "stage_counts") + ar.NODE_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    y4 = handout_yaws(18)[4]
    _equal(_device(ctx, c.start, c.end, start_yaw=y4), c.search(c.start, c.end, start_yaw=y4), "start_yaw")
    # a multi-device context gives the same bytes
    multi = svsdf_amd.SvsdfContext(shape="star", devices=[0, 0])
    multi.frontend_set_map(c.device_map(svsdf_amd), c.ks, c.count, ar.MARGIN)
    m = _device(multi, c.start, c.end)
    for k in ("path", "cells", "stage_counts") + ar.NODE_KEYS:
        assert m[k].tobytes() == a[k].tobytes(), k
    # a second map replaces the first and its node arrays
    c2 = ar.grid_case("star", 3, 2, 1.0, np.zeros((5, 11), dtype=bool))
    ctx.frontend_set_map(c2.device_map(svsdf_amd), c2.ks, c2.count, ar.MARGIN)
    with pytest.raises(svsdf_amd.SvsdfError, match="no search"):
        ctx.astar_nodes()
    s, e = c2.centre((0, 0)), c2.centre((4, 10))
    dev = _device(ctx, s, e)
    assert dev["id"].shape == (5, 11)
    _equal(dev, c2.search(s, e), "second map")
    assert ctx.astar_search(c.start, c.end)["status"] == "OUT_OF_MAP"       # inside the first map, outside the second


def test_z_outside_layer_0_is_refused(built):
    """A map of two layers: a point in the upper one is inside the map, but the search is planar in layer 0."""
    import svsdf_amd
    g = np.zeros((5, 11), dtype=bool)
    cloud = np.array([[0.0, 0.0, 0.0], [5.0, 11.0, 2.0]], dtype=np.float32)
    om = svsdf_amd.OccupancyMap(cloud, resolution=1.0, sta_threshold=2)
    assert om.info()["dims"] == (5, 11, 2)
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0)
    ctx.frontend_set_map(om, 3, 2, ar.MARGIN)
    with pytest.raises(svsdf_amd.SvsdfError, match="layer 0"):
        ctx.astar_search([0.5, 0.5, 1.5], [4.5, 10.5, 0.5])
    with pytest.raises(svsdf_amd.SvsdfError, match="layer 0"):
        ctx.astar_search([0.5, 0.5, 0.5], [4.5, 10.5, 1.5])
    assert ctx.astar_search([0.5, 0.5, 2.5], [4.5, 10.5, 0.5])["status"] == "OUT_OF_MAP"
    c = ar.grid_case("star", 3, 2, 1.0, g)
    r = ctx.astar_search([0.5, 0.5, 0.5], [4.5, 10.5, 0.5])
    ref = c.search(c.centre((0, 0)), c.centre((4, 10)))
    assert r["status"] == "FOUND" and r["cells"].tobytes() == ref["cells"].tobytes() and r["path"].tobytes() == ref["path"].tobytes()


# ---------------------------------------------------------------- case 7: nothing else changes
def test_search_leaves_the_other_front_end_entries_alone(resident):
    c = ar.demo_case("sdHeart")
    ctx = resident(c)
    X, Y = c.X, c.Y
    ij = np.array([(i, j) for i in range(1, X, 3) for j in range(1, Y, 4)], dtype=np.int32)
    yw = np.zeros(len(ij))
    before = [a.tobytes() for a in ctx.astar_successors(ij, yw)] + [ctx.yaw_free().tobytes()]
    ctx.astar_search(c.start, c.end)
    ctx.astar_search(c.end, c.start, slice=5)
    after = [a.tobytes() for a in ctx.astar_successors(ij, yw)] + [ctx.yaw_free().tobytes()]
    assert before == after
    np.testing.assert_array_equal(ctx.yaw_free(), c.free)
