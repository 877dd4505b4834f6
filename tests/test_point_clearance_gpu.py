"""svsdf_point_clearance on the device: for every resident point a certified bracket lower[p] <= c_p <= upper[p] on its
minimum over the whole duration of the SDF-at-time, a state and a witness time -- against a per-point dense reference
(svsdf_debug_sdf_at over 3000 equispaced times plus every piece boundary, per point; test_gpu_sdf_at.py pins that entry bit
for bit to the oracle) and the oracle itself for the witness.  Clouds, trajectories and the slack constants are those of
test_clearance_gpu.py."""
import functools

import numpy as np
import pytest

from oracle import orc
from test_clearance_gpu import SHAPES, Case, _same, case1

pytestmark = pytest.mark.gpu
EPS = 1e-3


def _dense_per_point(ctx, coeffs, T, pts):
    tt = np.concatenate([np.linspace(0.0, T.sum(), 3000), np.concatenate([[0.0], np.cumsum(T)])])
    out = np.empty(len(pts))
    for k in range(0, len(pts), 256):       # (256 points x 3000 times per call)
        xy = np.repeat(np.asarray(pts)[k:k + 256, :2], len(tt), axis=0)
        out[k:k + 256] = ctx.debug_sdf_at(coeffs, T, xy, np.tile(tt, len(xy) // len(tt)))[:, 0].reshape(-1, len(tt)).min(axis=1)
    return out


def _dense_of(c):
    """The per-point dense minimum of a Case, computed once and kept on it."""
    if not hasattr(c, "dense_p"):
        ctx = c.ctx()
        c.dense_p = _dense_per_point(ctx, c.coeffs, c.T, c.pts)
        ctx.close()
        c.dense_p.setflags(write=False)
    return c.dense_p


def _equal(a, b):
    """Two returns of point_clearance: identical arrays, identical structs except device_ms."""
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and _same(a[4], b[4])


def _check(out, o, T, pts, dense, eps=EPS, cap=None):
    """Every per-point check, and the struct against the arrays."""
    lower, upper, tw, state, res = out
    P = len(pts)
    print({k: res[k] for k in ("status", "levels", "counts", "lower", "upper", "evals", "pairs", "tile_pairs", "tile_pairs_kept")})
    assert len(lower) == len(upper) == len(tw) == len(state) == P
    assert np.all(lower <= upper)
    assert np.all(lower <= dense + 1e-9), np.max(lower - dense)
    conv = state == "CONVERGED"
    assert np.all(upper[conv] - lower[conv] <= eps)
    assert np.all(upper[conv] <= dense[conv] + eps + 1e-9)
    far = state == "FAR"
    assert cap is not None or not far.any()
    if cap is not None:
        assert np.all(lower[far] >= cap)
    assert np.all((0.0 <= tw) & (tw <= T.sum()))
    for p in range(P):
        assert upper[p] == o.sdf_at_time(pts[p, 0], pts[p, 1], tw[p]), (p, upper[p], tw[p])
    assert res["counts"] == {s: int((state == s).sum()) for s in ("CONVERGED", "FAR", "SAFE", "UNSAFE", "OPEN")}
    assert sum(res["counts"].values()) == P
    assert res["status"] == ("BUDGET" if res["counts"]["OPEN"] else "CONVERGED")
    if P:
        i = int(np.argmin(upper))           # (the first of equal minima: the smaller original index)
        assert (res["upper"], res["point_index"], res["t_witness"], res["lower"]) == (upper[i], i, tw[i], lower.min()), res
    return out


def _until_closed(ctx, c, **kw):
    """The automatic budget, raised until nothing is OPEN."""
    out = ctx.point_clearance(c.coeffs, c.T, eps=EPS, **kw)
    budget = out[4]["evals"]
    for _ in range(12):
        if out[4]["status"] == "CONVERGED":
            break
        budget *= 4
        out = ctx.point_clearance(c.coeffs, c.T, eps=EPS, max_evals=budget, **kw)
    assert out[4]["status"] == "CONVERGED" and out[4]["counts"]["OPEN"] == 0, out[4]
    return out


@pytest.mark.parametrize("trial", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape(built, shape, trial):
    c = case1(shape, trial)
    dense = _dense_of(c)
    ctx = c.ctx()
    lower, upper, tw, state, res = _check(_until_closed(ctx, c), c.o, c.T, c.pts, dense)
    assert np.all(state == "CONVERGED"), res
    assert res["lower"] <= dense.min() + 1e-9 and res["upper"] <= dense.min() + EPS + 1e-9, (res, dense.min())
    m = ctx.min_clearance(c.coeffs, c.T, eps=EPS)
    assert res["lower"] <= m["upper"] and m["lower"] <= res["upper"], (res, m)
    ctx.close()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_tile_tails(built, P):
    c = Case("star", 0, P=P, N=3, seed=3000 + P)
    ctx = c.ctx()
    lower, upper, tw, state, res = _check(_until_closed(ctx, c), c.o, c.T, c.pts, _dense_of(c))
    assert np.all(state == "CONVERGED") and res["tile_pairs"] % ((P + 63) // 64) == 0, res
    ctx.close()


def test_cap(built):
    c = case1("star", 0)
    dense = _dense_of(c)
    cap = 0.5
    assert (dense >= cap + EPS).any() and (dense < cap - EPS).any()
    ctx = c.ctx()
    full = _until_closed(ctx, c)
    lower, upper, tw, state, res = _check(_until_closed(ctx, c, cap=cap), c.o, c.T, c.pts, dense, cap=cap)
    clear = np.abs(dense - cap) > EPS
    assert np.array_equal((state == "FAR")[clear], (dense >= cap)[clear]), res
    assert np.all(state[~(state == "FAR")] == "CONVERGED")
    assert res["evals"] < full[4]["evals"], (res, full[4])
    ctx.close()


@functools.lru_cache(maxsize=None)
def _target_case():
    """Seed 6100: chosen with the oracle on the CPU (the same 3006 times per point) so that no point's dense minimum lies
    near the target 0 -- the nearest is 9.1e-3 away, the next 1.5e-2; 192 points collide, 108 do not."""
    return Case("star", 0, seed=6100)


def test_target(built):
    c = _target_case()
    dense = _dense_of(c)
    assert np.abs(dense).min() > 1e-6 and (dense < 0).any() and (dense > 0).any()     # no point's minimum within 1e-6 of the target
    ctx = c.ctx()
    full = _until_closed(ctx, c)
    lower, upper, tw, state, res = _check(_until_closed(ctx, c, target=0.0), c.o, c.T, c.pts, dense)
    assert np.all(upper[state == "UNSAFE"] < 0.0)
    assert np.all(dense[state == "SAFE"] >= -1e-9)
    assert np.all(lower[state == "SAFE"] >= 0.0)
    assert res["counts"]["OPEN"] == 0 and res["counts"]["SAFE"] + res["counts"]["UNSAFE"] == len(c.pts), res
    assert res["levels"] < full[4]["levels"], (res, full[4])
    ctx.close()


def test_twice_passed_obstacle(built):
    """The trajectory and cloud of test_clearance_gpu.py::test_global_not_local: out along y = 0, back along y = 1.5, past
    obstacles the way back comes 1.5 m closer to.  Every point's certified upper is at most its svsdf_query_points value
    (that test's margin, 1e-3), and its witness lies after the turn, on the way back."""
    import svsdf_amd
    shape = "sdCutDisk"
    T = np.array([2.1, 2.3, 1.9, 2.2, 2.0, 2.4]) * 1.003
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3)); ts[1, 0] = 1.5
    q = np.array([[7.0, 0.0, 0.0], [14.0, 0.0, 0.0], [20.0, 0.75, 0.0], [14.0, 1.5, 0.0], [7.0, 1.5, 0.0]])
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(head_state=hs, tail_state=ts)
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0, **kw)
    R = ctx.shape_bound()[0]
    rng = np.random.default_rng(5)
    pts = np.column_stack([10.0 + rng.normal(0, 0.2, 60), 1.5 + R + 2.5 + rng.uniform(0, 1.0, 60), np.zeros(60)])   # exterior only
    ctx.set_points(pts)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    dense = _dense_per_point(ctx, coeffs, T, pts)
    assert dense.min() > 0.0
    lower, upper, tw, state, res = _check(ctx.point_clearance(coeffs, T, eps=EPS, max_evals=10 ** 7), o, T, pts, dense)
    assert np.all(state == "CONVERGED"), res
    sdf = ctx.query_points(coeffs, T)[0]
    print("query_points - upper: max", (sdf - upper).max(), "points read more than 1 m too clear:", int((sdf > upper + 1.0).sum()))
    assert np.all(upper <= sdf + 1e-3), (sdf - upper).min()
    assert np.all(tw > T[:3].sum()), tw.min()
    m = ctx.min_clearance(coeffs, T, eps=EPS)
    assert res["lower"] <= m["upper"] and m["lower"] <= res["upper"] and res["t_witness"] > T[:3].sum(), (res, m)
    ctx.close()


def test_reproducible(built):
    """Two calls, pair_capacity 64 against the default, and a cloud kept in its input order: the same arrays and structs."""
    import svsdf_amd
    c = case1("sdHorseshoe", 0)
    dense = _dense_of(c)
    ctx = c.ctx()
    a = _check(_until_closed(ctx, c), c.o, c.T, c.pts, dense)
    budget = dict(max_evals=4 * a[4]["evals"])
    assert _equal(a, ctx.point_clearance(c.coeffs, c.T, eps=EPS, **budget))
    assert _equal(a, ctx.point_clearance(c.coeffs, c.T, eps=EPS, **budget))
    small = ctx.point_clearance(c.coeffs, c.T, eps=EPS, pair_capacity=64, **budget)
    assert a[4]["pairs"] > 64 and _equal(a, small), (a[4], small[4])
    assert _equal(a, ctx.point_clearance(c.coeffs, c.T, eps=EPS, pair_capacity=1000, **budget))
    ctx.close()
    keep = c.ctx(flags=svsdf_amd.FLAG_KEEP_INPUT_ORDER)
    assert np.array_equal(keep.shard_indices(), np.arange(len(c.pts)))
    k = _check(keep.point_clearance(c.coeffs, c.T, eps=EPS, **budget), c.o, c.T, c.pts, dense)
    assert np.all(k[3] == "CONVERGED"), k[4]
    assert _equal(k, keep.point_clearance(c.coeffs, c.T, eps=EPS, pair_capacity=64, **budget))
    keep.close()


def test_budget(built):
    """max_evals = 1: the seed and level 0 always run, level 1 is not started.  BUDGET, and every bracket still holds."""
    c = case1("sdHorseshoe", 0)
    ctx = c.ctx()
    lower, upper, tw, state, res = _check(ctx.point_clearance(c.coeffs, c.T, eps=EPS, max_evals=1), c.o, c.T, c.pts, _dense_of(c))
    assert res["status"] == "BUDGET" and res["levels"] == 1 and res["pairs"] == 0 and (state == "OPEN").any(), res
    ctx.close()


def test_context_state(built):
    """The sequence of test_clearance_gpu.py::test_context_state around this call, and svsdf_min_clearance before and after."""
    import svsdf_amd
    base = svsdf_amd.live_allocations()
    c = case1("star", 1)
    ctx = c.ctx()
    m0 = ctx.min_clearance(c.coeffs, c.T)
    e0 = ctx.eval_penalty(c.coeffs, c.T)
    s0 = ctx.stats()
    lower, upper, tw, state, res = ctx.point_clearance(c.coeffs * 1.01, c.T * 1.1)     # another trajectory, generic durations
    assert np.all(lower <= upper) and res["evals"] > 0
    assert ctx.stats() == s0
    e1 = ctx.eval_penalty(c.coeffs, c.T)
    assert e0[0] == e1[0] and np.array_equal(e0[1], e1[1]) and np.array_equal(e0[2], e1[2])
    # and against a context that never ran the search: evaluation by evaluation the same bits
    ref = c.ctx()
    f0 = ref.eval_penalty(c.coeffs, c.T)
    f1 = ref.eval_penalty(c.coeffs, c.T)
    assert e0[0] == f0[0] and e1[0] == f1[0] and np.array_equal(e1[2], f1[2]) and np.array_equal(e1[1], f1[1])
    ref.close()
    assert _same(m0, ctx.min_clearance(c.coeffs, c.T))
    ctx.close()
    assert svsdf_amd.live_allocations() == base


def test_group(built):
    """Three stripes (on one device): each searched on its own, its points scattered to their original indices."""
    c = case1("star", 0)
    dense = _dense_of(c)
    ctx = c.ctx(devices=[0, 0, 0])
    lower, upper, tw, state, res = _check(_until_closed(ctx, c), c.o, c.T, c.pts, dense)
    assert np.all(state == "CONVERGED") and sum(res["counts"].values()) == len(c.pts), res
    ctx.close()


def test_refusals(built):
    import svsdf_amd
    c = case1("star", 0)
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0, **c.kw)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"svsdf_point_clearance failed \(3\)"):     # SVSDF_ERR_NO_POINTS
        ctx.point_clearance(c.coeffs, c.T)
    ctx.set_points(c.pts)
    ctx.set_scale(**svsdf_amd.binding.EXAMPLE_SCALE)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance.*scale"):
        ctx.point_clearance(c.coeffs, c.T)
    ctx.set_scale(None)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance.*300"):
        ctx.point_clearance(c.coeffs, np.full(5, 60.0))
    bad = c.coeffs.copy(); bad[7, 1] = np.nan
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(4\): svsdf_point_clearance"):    # SVSDF_ERR_NONFINITE
        ctx.point_clearance(bad, c.T)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance"):    # bad N
        ctx.point_clearance(np.zeros((6 * 129, 3)), np.full(129, 0.5))
    for kw in (dict(eps=0.0), dict(eps=float("nan")), dict(struct_size=8), dict(cap=float("nan"))):
        with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance"):
            ctx.point_clearance(c.coeffs, c.T, **kw)
    _check(_until_closed(ctx, c), c.o, c.T, c.pts, _dense_of(c))                     # and the context still works
    ctx.set_points(np.zeros((0, 3)))
    lower, upper, tw, state, res = ctx.point_clearance(c.coeffs, c.T)
    assert len(lower) == len(state) == 0 and res["lower"] == res["upper"] == np.inf and res["point_index"] == -1, res
    assert res["status"] == "CONVERGED" and sum(res["counts"].values()) == 0 and res["evals"] == 0
    ctx.close()
