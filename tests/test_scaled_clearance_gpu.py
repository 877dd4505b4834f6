"""svsdf_min_clearance and svsdf_point_clearance under a scale schedule, on a context created with
SVSDF_FLAG_SCALED_CLEARANCE ("Under a scale schedule"): the certified brackets on the minimum of
getSDFAtTimeStamp<true> against a dense reference -- svsdf_debug_sdf_at under the same schedule over every point x 3000
equispaced times plus every piece boundary; tests/test_scale_oracle_gpu.py pins that entry bit for bit to the oracle -- and
the oracle's rel_at_time for the witness.  Clouds and trajectories are those of tests/test_clearance_gpu.py.

Every call passes max_evals = 16 x the automatic budget: a condition, so that a plateau of the scaled bound cannot turn a
pass into a budget stop, not a claim about cost (a CPU prototype of the search used 0.27 of the automatic budget); the
evaluations made are printed."""
import functools

import numpy as np
import pytest

from oracle import orc
from test_clearance_gpu import SHAPES, Case, _same, case1
from test_scale_gpu import _with_env

pytestmark = pytest.mark.gpu
EPS = 1e-3
SCHEDULES = {"A": dict(c=(0.8, 0.8), amp=(0.6, 0.4), omega=(1.5, 1.8), phase=(-1.0, 0.0)),       # binding.EXAMPLE_SCALE
             "B": dict(c=(1.3, 0.6), amp=(0.0, 0.0), omega=(0.0, 0.0), phase=(0.0, 0.0))}        # constant, anisotropic
# every name of orc.SHAPES; the Polygon on both of its code paths (compiled id 16: edges in global memory; 17: in LDS),
# selected at context creation the way tests/test_scale_gpu.py::_case selects them
VARIANTS = [(s, 17 if s == "Polygon" else SHAPES.index(s)) for s in SHAPES] + [("Polygon", 16)]


def _budget(P, T):
    return 16 * 4 * P * int(np.ceil(T.sum() / 0.15))


def _flagged(c, sid=0, sched=None, **extra):
    import svsdf_amd
    env = {"SVSDF_POLY_LDS": 0} if sid == 16 else {}
    ctx = _with_env(env, lambda: c.ctx(flags=svsdf_amd.FLAG_SCALED_CLEARANCE, **extra))
    if sched is not None:
        ctx.set_scale(**sched)
    return ctx


def _times(T, n):
    return np.concatenate([np.linspace(0.0, T.sum(), n), np.concatenate([[0.0], np.cumsum(T)])])


def _dense_per_point(ctx, coeffs, T, pts, n=3000):
    """Per point, the smallest debug_sdf_at value (under the context's schedule) over n equispaced times and the boundaries."""
    tt = _times(T, n)
    out = np.empty(len(pts))
    step = max(1, 768000 // len(tt))
    for k in range(0, len(pts), step):
        xy = np.repeat(np.asarray(pts)[k:k + step, :2], len(tt), axis=0)
        out[k:k + step] = ctx.debug_sdf_at(coeffs, T, xy, np.tile(tt, len(xy) // len(tt)))[:, 0].reshape(-1, len(tt)).min(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def _dense(shape, sid, name, trial=0):
    """The per-point dense minimum of case1(shape, trial) under schedule `name`: computed once, shared, read-only."""
    c = case1(shape, trial)
    ctx = _flagged(c, sid, SCHEDULES[name])
    d = _dense_per_point(ctx, c.coeffs, c.T, c.pts)
    ctx.close()
    d.setflags(write=False)
    return d


def _oracle(c, sched):
    """An oracle of this file's own under the schedule (the Case's is shared with the rigid tests and stays rigid)."""
    o = orc.Oracle(c.shape, **c.kw)
    o.set_traj(c.coeffs, c.T)
    o.set_modes(1, 0)          # device-library trig, the reference's piece location
    if sched is not None:
        o.set_scale(**sched)
    return o


def _value(dbg, coeffs, T, xy, t):
    return dbg.debug_sdf_at(coeffs, T, np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(t, dtype=np.float64).reshape(-1))[:, 0]


def _check_min(ctx, coeffs, T, pts, dense, eps=EPS, o=None, dbg=None, **kw):
    """The checks of test_clearance_gpu.py::_check with the scaled value.  dense: the minimum over the cloud.  Returns the result."""
    kw.setdefault("max_evals", _budget(len(pts), T))
    r = ctx.min_clearance(coeffs, T, eps=eps, **kw)
    print({k: r[k] for k in ("status", "levels", "lower", "upper", "evals", "pairs", "tile_pairs", "tile_pairs_kept")}, "dense", dense)
    assert r["lower"] <= r["upper"]
    assert r["lower"] <= dense + 1e-9, (r, dense)
    if r["status"] == "CONVERGED":
        assert r["upper"] - r["lower"] <= eps, r
        assert r["upper"] <= dense + eps + 1e-9, (r, dense)
    x, y = r["point_xy"]
    assert r["upper"] == _value(dbg or ctx, coeffs, T, [[x, y]], [r["t_witness"]])[0], r
    if o is not None:
        assert r["upper"] == o.rel_at_time(np.array([[x, y]]), np.array([r["t_witness"]]))[0, 0], r
    assert 0 <= r["point_index"] < len(pts) and (x, y) == tuple(np.asarray(pts)[r["point_index"], :2]), r
    assert 0.0 <= r["t_witness"] <= T.sum()
    assert _same(r, ctx.min_clearance(coeffs, T, eps=eps, **kw))
    return r


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and _same(a[4], b[4])


def _check_points(ctx, coeffs, T, pts, dense, eps=EPS, cap=None, dbg=None, twice=True, **kw):
    """The checks of test_point_clearance_gpu.py::_check with the scaled value.  dense: per point.  Returns the five results."""
    kw.setdefault("max_evals", _budget(len(pts), T))
    if cap is not None:
        kw["cap"] = cap
    out = ctx.point_clearance(coeffs, T, eps=eps, **kw)
    lower, upper, tw, state, res = out
    P = len(pts)
    print({k: res[k] for k in ("status", "levels", "counts", "lower", "upper", "evals", "pairs", "tile_pairs", "tile_pairs_kept")})
    assert len(lower) == len(upper) == len(tw) == len(state) == P
    assert np.all(lower <= dense + 1e-9), np.max(lower - dense)
    assert np.all(upper >= lower)
    conv = state == "CONVERGED"
    assert np.all(upper[conv] - lower[conv] <= eps)
    assert np.all(upper[conv] <= dense[conv] + eps + 1e-9)
    far = state == "FAR"
    assert cap is not None or not far.any()
    if cap is not None:
        assert np.all(lower[far] >= cap) and np.all(dense[far] >= cap - 1e-9)
    assert np.all((0.0 <= tw) & (tw <= T.sum()))
    assert np.array_equal(upper, _value(dbg or ctx, coeffs, T, np.asarray(pts)[:, :2], tw))       # bit for bit
    assert res["counts"] == {s: int((state == s).sum()) for s in ("CONVERGED", "FAR", "SAFE", "UNSAFE", "OPEN")}
    assert res["status"] == ("BUDGET" if res["counts"]["OPEN"] else "CONVERGED")
    i = int(np.argmin(upper))               # (the first of equal minima: the smaller original index)
    assert (res["upper"], res["point_index"], res["t_witness"], res["lower"]) == (upper[i], i, tw[i], lower.min()), res
    if twice:
        assert _equal(out, ctx.point_clearance(coeffs, T, eps=eps, **kw))
    return out


# ------------------------------------------------------------------------------------------ 1, 2. every shape
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("shape,sid", VARIANTS)
def test_every_shape(built, shape, sid, name):
    c = case1(shape, 0)                     # generic durations, P = 300, N = 5
    dense = _dense(shape, sid, name)
    ctx = _flagged(c, sid, SCHEDULES[name])
    r = _check_min(ctx, c.coeffs, c.T, c.pts, dense.min(), o=_oracle(c, SCHEDULES[name]))
    assert r["status"] == "CONVERGED", r
    ctx.close()


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("shape,sid", VARIANTS)
def test_every_shape_per_point(built, shape, sid, name):
    c = case1(shape, 0)
    dense = _dense(shape, sid, name)
    ctx = _flagged(c, sid, SCHEDULES[name])
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense)
    assert not (state == "OPEN").any() and np.all(state == "CONVERGED"), res
    ctx.close()


# ------------------------------------------------------------------------------------------ 3. tile tails
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_tile_tails(built, P):
    c = Case("star", 0, P=P, N=3, seed=3000 + P)
    ctx = _flagged(c, 4, SCHEDULES["A"])
    dense = _dense_per_point(ctx, c.coeffs, c.T, c.pts)
    r = _check_min(ctx, c.coeffs, c.T, c.pts, dense.min(), o=_oracle(c, SCHEDULES["A"]))
    assert r["status"] == "CONVERGED" and r["tile_pairs"] % ((P + 63) // 64) == 0, r
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense)
    assert np.all(state == "CONVERGED") and res["tile_pairs"] % ((P + 63) // 64) == 0, res
    ctx.close()


# ------------------------------------------------------------------------------------------ 4. each new term carries
# Three inputs in the manner of test_clearance_gpu.py::test_yaw_rate_term, one per term the scaled bound adds to the rigid
# one.  For each, tools/scaled_clearance_prototype.py (this search on the CPU, on the oracle's values) was run with the full
# bound and with that one term in its rigid form: the docstrings hold the brackets it printed.
def _term_case(shape, coeffs, T, hs, ts, pts, sched, n_dense, polygon=None):
    """A flagged context under `sched` on the cloud `pts`; both entries checked against the dense reference."""
    import svsdf_amd
    kw = dict(head_state=hs, tail_state=ts, polygon=polygon)
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0, flags=svsdf_amd.FLAG_SCALED_CLEARANCE, **kw)
    ctx.set_points(pts)
    ctx.set_scale(**sched)
    dense = _dense_per_point(ctx, coeffs, T, pts, n=n_dense)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    o.set_scale(**sched)
    r = _check_min(ctx, coeffs, T, pts, dense.min(), o=o)
    assert r["status"] == "CONVERGED", r
    lower, upper, tw, state, res = _check_points(ctx, coeffs, T, pts, dense)
    assert np.all(state == "CONVERGED"), res
    ctx.close()
    return r, dense


def _straight(length, T):
    """test_clearance_gpu.py::_straight's recipe: rest to rest along +x with the yaw fixed at 0."""
    import svsdf_amd
    N = len(T)
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3)); ts[0, 0] = length
    q = np.column_stack([np.linspace(0.0, length, N + 1)[1:-1], np.zeros(N - 1), np.zeros(N - 1)])
    return svsdf_amd.minco_coeffs(hs, ts, q, T), T, hs, ts


def speed_case():
    """20 m in 8.08 s (up to 4.6 m/s) under the constant scale 0.25 (Imax = 4); 8 points beside the fast middle of the pass,
    0.57 to 0.64 m off the line of motion -- just outside the quarter-size star: in body-frame units each is passed at 4 x the
    robot's speed, a dip of sdf_sc(t) a fraction of a level-0 interval wide."""
    coeffs, T, hs, ts = _straight(20.0, np.array([1.7, 2.3, 1.9, 2.1]) * 1.01)
    k = np.arange(8)
    pts = np.column_stack([7.0 + 0.93 * k, 0.57 + 0.01 * k, np.zeros(8)])
    return "star", coeffs, T, hs, ts, pts, dict(c=(0.25, 0.25), amp=(0.0, 0.0), omega=(0.0, 0.0), phase=(0.0, 0.0)), None


def test_speed_term(built):
    """V * Imax: the body-frame point u = S^-1 R^T (p - x(t)) moves at up to V Imax, here 4 V.  The CPU prototype with the
    rigid speed term V (Imax dropped) returned on this input the bracket [-0.193049, -0.193049], which the dense minimum (200 000 times
    per point) -0.293885 violates; with the full bound it returned [-0.294265, -0.293799]."""
    shape, coeffs, T, hs, ts, pts, sched, poly = speed_case()
    r, dense = _term_case(shape, coeffs, T, hs, ts, pts, sched, 200000, poly)
    assert r["lower"] <= dense.min() + 1e-9


def scale_rate_case():
    """1 m in 9.4 s with the yaw fixed (V <= 0.2 m/s, W = 0) under a fast schedule, w = (5, 6) rad/s, s between 0.5 and 1.1;
    4 points 21 to 36 m ahead: u breathes by metres per level-0 interval while the pose hardly moves."""
    coeffs, T, hs, ts = _straight(1.0, np.array([2.2, 2.5, 2.3, 2.4]))
    pts = np.array([[21.0 + 5.0 * k, 0.3 * k, 0.0] for k in range(4)])
    return "sdHorseshoe", coeffs, T, hs, ts, pts, dict(c=(0.8, 0.8), amp=(0.3, 0.3), omega=(5.0, 6.0), phase=(0.75, -0.7)), None


def test_scale_rate_term(built):
    """Q * |p - x|: what a change of S(t)^-1 over the interval does to u.  The CPU prototype with the Q term dropped (the
    scale frozen at the midpoint) returned on this input the bracket [16.539829, 16.539829], which the dense minimum 16.427679 violates;
    with the full bound it returned [16.426679, 16.427677]."""
    shape, coeffs, T, hs, ts, pts, sched, poly = scale_rate_case()
    r, dense = _term_case(shape, coeffs, T, hs, ts, pts, sched, 20000, poly)
    assert r["lower"] <= dense.min() + 1e-9 and r["lower"] > 0.0


def _path_pos(coeffs, T, t):
    """x, y of the trajectory at time t (row 6 i + k of coeffs: the coefficient of s^k of piece i)."""
    S = np.concatenate([[0.0], np.cumsum(T)])
    i = min(int(np.searchsorted(S, t, side="right")) - 1, len(T) - 1)
    return sum(coeffs[6 * i + k, :2] * (t - S[i]) ** k for k in range(6))


def yaw_case():
    """The trajectory recipe of the rigid tests (yaw waypoints in +-2.5 rad) under the constant scale 0.3; the robot a
    60 x 2 rhombus (a Polygon outline), 18 x 0.6 m in the world; 4 points 5 to 10 m from path positions, |u| = |p - x| / 0.3:
    the yaw sweeps the rhombus's arm over a point at W |u| body-frame units per second, 3.3 x the rigid W |p - x|."""
    from test_clearance_gpu import _traj
    rng = np.random.default_rng(7201)
    coeffs, T, hs, ts = _traj(rng, 5, 0)
    pos = np.array([_path_pos(coeffs, T, t) for t in rng.uniform(0.0, T.sum(), 4)])
    ang, rad = rng.uniform(0, 2 * np.pi, 4), rng.uniform(5.0, 10.0, 4)
    pts = np.column_stack([pos[:, 0] + rad * np.cos(ang), pos[:, 1] + rad * np.sin(ang), np.zeros(4)])
    bar = np.array([[30.0, 0.0], [0.0, 1.0], [-30.0, 0.0], [0.0, -1.0]])
    return "Polygon", coeffs, T, hs, ts, pts, dict(c=(0.3, 0.3), amp=(0.0, 0.0), omega=(0.0, 0.0), phase=(0.0, 0.0)), bar


def test_yaw_rate_term_scaled(built):
    """W * |u| with |u| > |p - x|.  The CPU prototype with the rigid W |p - x(m)| in place of W |u(m)| returned on this
    input the bracket [-0.221651, -0.221651], which the dense minimum -0.396530 (200 000 times per point) violates; with the full bound it returned [-0.397257, -0.396589]."""
    shape, coeffs, T, hs, ts, pts, sched, poly = yaw_case()
    r, dense = _term_case(shape, coeffs, T, hs, ts, pts, sched, 200000, poly)
    assert r["lower"] <= dense.min() + 1e-9 and r["lower"] < 0.0


# ------------------------------------------------------------------------------------------ 5. the flag
def test_flag_semantics(built):
    import svsdf_amd
    c = case1("star", 0)
    plain = c.ctx()
    m0 = plain.min_clearance(c.coeffs, c.T)
    p0 = plain.point_clearance(c.coeffs, c.T, max_evals=10 ** 7)
    plain.set_scale(**SCHEDULES["A"])
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\).*scale"):
        plain.min_clearance(c.coeffs, c.T)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance.*scale.*SVSDF_FLAG_SCALED_CLEARANCE"):
        plain.point_clearance(c.coeffs, c.T)
    plain.close()
    ctx = _flagged(c, 4)
    assert _same(m0, ctx.min_clearance(c.coeffs, c.T))                     # no schedule: the rigid search, bit for bit
    assert _equal(p0, ctx.point_clearance(c.coeffs, c.T, max_evals=10 ** 7))
    ctx.set_scale(**SCHEDULES["A"])
    ms = ctx.min_clearance(c.coeffs, c.T, max_evals=_budget(len(c.pts), c.T))
    ps = ctx.point_clearance(c.coeffs, c.T, max_evals=_budget(len(c.pts), c.T))
    assert ms["upper"] != m0["upper"] and not np.array_equal(ps[1], p0[1]), "the schedule must act"
    ctx.set_scale(None)
    assert _same(m0, ctx.min_clearance(c.coeffs, c.T))                     # and the rigid result again
    assert _equal(p0, ctx.point_clearance(c.coeffs, c.T, max_evals=10 ** 7))
    ctx.close()


# ------------------------------------------------------------------------------------------ 6. the context's state
def test_context_state(built):
    import svsdf_amd
    base = svsdf_amd.live_allocations()
    c = case1("star", 1)
    ctx = _flagged(c, 4, SCHEDULES["A"])
    e0 = ctx.eval_penalty(c.coeffs, c.T)
    s0, plan0 = ctx.stats(), ctx.get_plan()
    r = ctx.min_clearance(c.coeffs * 1.01, c.T * 1.1, max_evals=_budget(len(c.pts), c.T * 1.1))    # another trajectory, generic durations
    assert r["lower"] <= r["upper"] and r["evals"] > 0
    lower, upper, tw, state, res = ctx.point_clearance(c.coeffs * 1.01, c.T * 1.1, max_evals=_budget(len(c.pts), c.T * 1.1))
    assert np.all(lower <= upper) and res["evals"] > 0
    assert ctx.stats() == s0 and ctx.get_plan() == plan0
    e1 = ctx.eval_penalty(c.coeffs, c.T)
    assert e0[0] == e1[0] and np.array_equal(e0[1], e1[1]) and np.array_equal(e0[2], e1[2])
    # and against a context that never ran the search: evaluation by evaluation the same bits
    ref = _flagged(c, 4, SCHEDULES["A"])
    f0 = ref.eval_penalty(c.coeffs, c.T)
    f1 = ref.eval_penalty(c.coeffs, c.T)
    assert e0[0] == f0[0] and e1[0] == f1[0] and np.array_equal(e1[2], f1[2]) and np.array_equal(e1[1], f1[1])
    ref.close()
    ctx.close()
    assert svsdf_amd.live_allocations() == base


# ------------------------------------------------------------------------------------------ 7. target, cap, budget, capacity
def test_target_cap_budget(built):
    """The dense minimum is sampled, so it lies at or above the true minimum c_p; the full search's lower[p] lies at or below
    it.  Every consistency check uses the one of the two that makes it rigorous: dense_p < x proves c_p < x, lower_p > x
    proves c_p > x."""
    c = case1("star", 0)
    dense = _dense("star", 4, "A")
    dmin = float(dense.min())
    ctx = _flagged(c, 4, SCHEDULES["A"])
    auto = _check_min(ctx, c.coeffs, c.T, c.pts, dmin)
    full = _check_points(ctx, c.coeffs, c.T, c.pts, dense)
    assert auto["status"] == "CONVERGED" and np.all(full[3] == "CONVERGED")
    lo_full = full[0]
    # target = 0: UNSAFE / SAFE by the sign of the minimum, wherever it is more than eps from 0
    r = _check_min(ctx, c.coeffs, c.T, c.pts, dmin, target=0.0)
    assert abs(dmin) > EPS and (dmin < -EPS or auto["lower"] > EPS), (dmin, auto)
    assert r["status"] == ("UNSAFE" if dmin < 0.0 else "SAFE"), (r, dmin)
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense, target=0.0)
    assert (dense < -EPS).any() and (lo_full > EPS).any()
    assert np.all(state[dense < -EPS] == "UNSAFE") and np.all(state[lo_full > EPS] == "SAFE"), res
    assert np.all(upper[state == "UNSAFE"] < 0.0) and np.all(lower[state == "SAFE"] >= 0.0)
    assert res["counts"]["OPEN"] == 0 and res["levels"] <= full[4]["levels"], res
    # cap: FAR exactly where the minimum is above it
    cap = 0.5
    assert (lo_full >= cap + EPS).any() and (dense < cap - EPS).any()
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense, cap=cap)
    far = state == "FAR"
    assert far.any() and np.all(dense[far] >= cap - 1e-9) and np.all(lower[far] >= cap)
    assert np.all(far[lo_full >= cap + EPS]) and not far[dense < cap - EPS].any() and np.all(state[~far] == "CONVERGED"), res
    assert res["evals"] < full[4]["evals"], (res, full[4])
    # budget: exactly level 0's evaluations -- level 1 is not started, the brackets still hold
    level0 = ctx.min_clearance(c.coeffs, c.T, target=1e300)            # UNSAFE after level 0: its evaluation count
    assert level0["status"] == "UNSAFE" and level0["levels"] == 1
    r = _check_min(ctx, c.coeffs, c.T, c.pts, dmin, max_evals=level0["evals"])
    assert r["status"] == "BUDGET" and r["levels"] == 1 and r["evals"] == level0["evals"], r
    assert r["lower"] <= dmin + 1e-9 and auto["lower"] <= r["upper"]
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense, max_evals=1)
    assert res["status"] == "BUDGET" and res["levels"] == 1 and res["pairs"] == 0 and (state == "OPEN").any(), res
    assert np.all(lo_full <= upper)
    # pair_capacity: nothing reported depends on it
    assert auto["pairs"] > 64 and full[4]["pairs"] > 64
    for cap_pairs in (64, 1000, 0):
        assert _same(auto, ctx.min_clearance(c.coeffs, c.T, eps=EPS, max_evals=_budget(len(c.pts), c.T), pair_capacity=cap_pairs))
        assert _equal(full, ctx.point_clearance(c.coeffs, c.T, eps=EPS, max_evals=_budget(len(c.pts), c.T), pair_capacity=cap_pairs))
    ctx.close()


# ------------------------------------------------------------------------------------------ 8. a group
def test_group(built):
    """Two stripes on one device, host combine: each searched on its own under the same schedule."""
    c = case1("star", 0)
    dense = _dense("star", 4, "A")
    dbg = _flagged(c, 4, SCHEDULES["A"])
    one = dbg.min_clearance(c.coeffs, c.T, max_evals=_budget(len(c.pts), c.T))
    ctx = _flagged(c, 4, SCHEDULES["A"], devices=[0, 0])
    r = _check_min(ctx, c.coeffs, c.T, c.pts, float(dense.min()), o=_oracle(c, SCHEDULES["A"]), dbg=dbg)
    assert r["status"] == "CONVERGED" and abs(r["upper"] - one["upper"]) <= EPS, (r, one)
    lower, upper, tw, state, res = _check_points(ctx, c.coeffs, c.T, c.pts, dense, dbg=dbg)
    assert np.all(state == "CONVERGED") and sum(res["counts"].values()) == len(c.pts), res
    assert res["upper"] == _value(dbg, c.coeffs, c.T, c.pts[res["point_index"], :2], [res["t_witness"]])[0]
    ctx.close()
    dbg.close()


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_scaled(built):
    import svsdf_amd
    c = case1("star", 0)
    ctx = _flagged(c, 4, SCHEDULES["A"])
    bad = c.coeffs.copy(); bad[7, 1] = np.nan
    for name, call in (("svsdf_min_clearance", ctx.min_clearance), ("svsdf_point_clearance", ctx.point_clearance)):
        with pytest.raises(svsdf_amd.SvsdfError, match=rf"failed \(1\): {name}.*300"):
            call(c.coeffs, np.full(5, 60.0))
        with pytest.raises(svsdf_amd.SvsdfError, match=rf"failed \(4\): {name}"):            # SVSDF_ERR_NONFINITE
            call(bad, c.T)
        for kw in (dict(eps=0.0), dict(eps=float("nan")), dict(eps=float("inf"))):
            with pytest.raises(svsdf_amd.SvsdfError, match=rf"failed \(1\): {name}.*eps"):
                call(c.coeffs, c.T, **kw)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\): svsdf_point_clearance.*cap"):
        ctx.point_clearance(c.coeffs, c.T, cap=float("nan"))
    r = ctx.min_clearance(c.coeffs, c.T, max_evals=_budget(len(c.pts), c.T))                      # and the context still works
    assert r["status"] == "CONVERGED"
    ctx.set_points(np.zeros((0, 3)))
    r = ctx.min_clearance(c.coeffs, c.T)
    assert r["lower"] == r["upper"] == np.inf and r["point_index"] == -1, r
    ctx.close()
