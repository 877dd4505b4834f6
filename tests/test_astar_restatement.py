"""The plain-Python restatement of AstarPathSearch + getPath (tests/astar_restatement.py) that svsdf_astar_search is
held to, checked on the CPU against a second, literal form of the open set and against its own invariants; and the
host-only plumbing of the two new entry points.  No device."""
import math

import numpy as np
import pytest

import astar_restatement as ar

DEMOS = ["star", "sdHorseshoe", "sdHeart"]
# the issue's tables, recomputed here: (path cells, expansions, pushes, relaxed_open, reopened) forward; reverse:
# (status, path cells, expansions)
FORWARD = {"star": (70, 693, 769, 483, 74), "sdHorseshoe": (63, 584, 740, 272, 36), "sdHeart": (75, 1466, 1569, 828, 337)}
REVERSE = {"star": ("FOUND", 71, 945), "sdHorseshoe": ("EXHAUSTED", 0, 868), "sdHeart": ("EXHAUSTED", 0, 913)}


def _both(case, start, end, **kw):
    a = case.search(start, end, open_set="argmin", **kw)
    b = case.search(start, end, open_set="sorted", **kw)
    assert ar.same_search(a, b, keys=("status", "path_len", "g_goal", "ties", "pops", "max_open") + ar.COUNTERS) == []
    return a


def _check_path(case, r):
    """Every consecutive pair of the path is an accepted slot of successors_ref; g_goal is the sum of the edge costs."""
    cells = [tuple(c) for c in r["cells"]]
    g = 0.0
    for k in range(1, len(cells)):
        (pi, pj), (vi, vj) = cells[k - 1], cells[k]
        i, j = vi - pi, vj - pj
        assert abs(i) <= 1 and abs(j) <= 1
        ok, cy, st = case.successors((pi, pj), float(r["path"][k - 1, 2]))
        s = 3 * (i + 1) + (j + 1)
        assert ok[s] and st[s] == 0
        assert r["father_cell"][vi, vj] == (ar.START if k == 1 else pi * case.Y + pj)
        g = math.sqrt(i * i + j * j) + g
        assert float(r["g"][vi, vj]).hex() == g.hex()
    assert float(r["g_goal"]).hex() == g.hex()


@pytest.mark.parametrize("name", DEMOS)
def test_demo_scenarios_both_open_sets(built, name):
    c = ar.demo_case(name)
    r = _both(c, c.start, c.end)
    print(name, "forward", r["path_len"], r["expansions"], r["pushes"], r["relaxed_open"], r["reopened"], "ties", r["ties"])
    assert r["status"] == "FOUND"
    assert (r["path_len"], r["expansions"], r["pushes"], r["relaxed_open"], r["reopened"]) == FORWARD[name]
    assert r["relaxed_open"] > 0 and r["reopened"] > 0
    _check_path(c, r)
    assert r["path"][0, 2] == 0.0 and tuple(r["cells"][0]) == ar.grid_index(c.start, c.bmin, c.bmax, 1.0, c.occ.shape)[:2]
    b = _both(c, c.end, c.start)
    print(name, "reverse", b["status"], b["path_len"], b["expansions"])
    assert (b["status"], b["path_len"], b["expansions"]) == REVERSE[name]
    if b["status"] == "FOUND":
        _check_path(c, b)


@pytest.mark.parametrize("shape,want", [("sdHorseshoe", (68, 481, 212, 41)), ("star", (75, 782, 277, 30))])
def test_sparse_grid_has_ties(built, shape, want):
    c = ar.grid_case(shape, 9, 8, 1.0, ar.sparse_grid(0.03, 1))
    r = _both(c, c.centre((1, 1)), c.centre((11, 68)))
    print(shape, r["path_len"], r["expansions"], r["reopened"], r["ties"])
    assert r["status"] == "FOUND" and (r["path_len"], r["expansions"], r["reopened"], r["ties"]) == want
    assert r["ties"] > 0
    _check_path(c, r)


def test_small_grids(built):
    c = ar.grid_case("star", 9, 8, 1.0, ar.sparse_grid(0.06, 2))      # the start has no accepted neighbour
    r = _both(c, c.centre((1, 1)), c.centre((11, 68)))
    assert (r["status"], r["expansions"], r["path_len"], r["pushes"]) == ("EXHAUSTED", 1, 0, 1)
    c = ar.grid_case("star", 3, 2, 1.0, np.zeros((5, 11), dtype=bool))
    r = _both(c, c.centre((0, 0)), c.centre((4, 10)))
    assert (r["status"], r["path_len"], r["expansions"], r["pushes"]) == ("FOUND", 11, 10, 31)
    _check_path(c, r)
    s = _both(c, c.centre((2, 3)), c.centre((2, 3)))                    # start == goal
    assert (s["status"], s["path_len"], s["expansions"], s["pops"]) == ("FOUND", 1, 0, 1)
    assert s["id"][2, 3] == 1 and np.count_nonzero(s["id"]) == 1
    c = ar.grid_case("star", 3, 2, 0.25, np.zeros((65, 129), dtype=bool))
    r = _both(c, c.centre((0, 0)), c.centre((64, 100)))
    assert (r["status"], r["path_len"], r["max_open"]) == ("FOUND", 101, 291)
    _check_path(c, r)


@pytest.mark.parametrize("k", [1, 50, 500])
def test_limit_stops_after_k_expansions(built, k):
    c = ar.demo_case("star")
    r = _both(c, c.start, c.end, max_expansions=k)
    full = c.search(c.start, c.end)
    assert r["status"] == "LIMIT" and r["expansions"] == k and r["path_len"] == 0 and r["pops"] == k
    assert np.count_nonzero(r["id"]) <= np.count_nonzero(full["id"])


def test_out_of_map_and_start_yaw(built):
    c = ar.demo_case("star")
    out = [c.bmax[0] + 1.0, c.start[1], 0.0]
    assert c.search(out, c.end)["status"] == "OUT_OF_MAP" and c.search(c.start, out)["status"] == "OUT_OF_MAP"
    from test_frontend_succ import handout_yaws
    r = _both(c, c.start, c.end, start_yaw=handout_yaws(18)[4])
    assert r["path"][0, 2] == handout_yaws(18)[4]
    assert ar.same_search(r, c.search(c.start, c.end)) != []          # the start yaw matters


# ---------------------------------------------------------------- host-only plumbing
def test_host_only_context_has_no_search(built):
    import svsdf_amd
    ctx = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)
    with pytest.raises(svsdf_amd.SvsdfError, match="no device context"):
        ctx.astar_search([1.0, 1.0, 0.0], [2.0, 2.0, 0.0])
    with pytest.raises(svsdf_amd.SvsdfError, match="no device context"):
        ctx.astar_nodes()


def test_new_symbols_and_structs(built):
    import ctypes as C
    import svsdf_amd
    from svsdf_amd import binding
    L = C.CDLL(svsdf_amd.lib_path())
    for name in ("svsdf_astar_params_default", "svsdf_astar_search", "svsdf_astar_nodes"):
        assert hasattr(L, name) and name in binding.EXPORTS
    p = binding.AstarParams()
    p.start_yaw, p.max_expansions, p.slice = 7.0, 7, 7
    svsdf_amd.lib().svsdf_astar_params_default(C.byref(p))
    assert (p.struct_size, p.start_yaw, p.max_expansions, p.slice) == (C.sizeof(binding.AstarParams), 0.0, 0, 0)
    assert C.sizeof(binding.AstarParams) == 32 and C.sizeof(binding.AstarResult) == 104
    # a host-only context refuses through the raw entry as well, before it looks at any other argument
    ctx = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)
    assert svsdf_amd.lib().svsdf_astar_search(ctx.ctx, None, None, None, None, None, 0, None) == 2      # SVSDF_ERR_NO_DEVICE
    assert svsdf_amd.lib().svsdf_astar_nodes(ctx.ctx, None, None, None, None, None, 0, None) == 2
