"""svsdf_min_clearance on the device: the certified bracket lower <= c* <= upper on the minimum, over the resident cloud and
over the whole duration, of the SDF-at-time -- against a dense reference (svsdf_debug_sdf_at over every point x 3000
equispaced times plus every piece boundary; test_gpu_sdf_at.py pins that entry bit for bit to the oracle) and the oracle
itself for the witness.  The clouds are tiny on purpose: every path of the search (tile tails, frontier slices, budget,
target, groups) is reached at a few hundred points."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu
SHAPES = list(orc.SHAPES)
ASSETS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_assets.json")))


def _voxel_centres(cloud, res):
    """Centres of the voxels of size `res`, counted from the cloud's minimum corner, that hold a point."""
    c = cloud.astype(np.float64)
    idx = np.unique(np.floor((c - c.min(axis=0)) / res).astype(np.int64), axis=0)
    return c.min(axis=0) + (idx + 0.5) * res


def _same(a, b):
    return {k: v for k, v in a.items() if k != "device_ms"} == {k: v for k, v in b.items() if k != "device_ms"}


def _dense_min(ctx, coeffs, T, pts):
    tt = np.concatenate([np.linspace(0.0, T.sum(), 3000), np.concatenate([[0.0], np.cumsum(T)])])
    best = np.inf
    for k in range(0, len(pts), 256):       # (256 points x 3000 times per call)
        xy = np.repeat(np.asarray(pts)[k:k + 256, :2], len(tt), axis=0)
        best = min(best, float(ctx.debug_sdf_at(coeffs, T, xy, np.tile(tt, len(xy) // len(tt)))[:, 0].min()))
    return best


def _check(ctx, o, coeffs, T, pts, eps, dense, **kw):
    """The common checker.  Returns the result."""
    r = ctx.min_clearance(coeffs, T, eps=eps, **kw)
    print({k: r[k] for k in ("status", "levels", "lower", "upper", "evals", "pairs", "tile_pairs", "tile_pairs_kept")}, "dense", dense)
    assert r["lower"] <= r["upper"]
    assert r["lower"] <= dense + 1e-9, (r, dense)
    if r["status"] == "CONVERGED":
        assert r["upper"] - r["lower"] <= eps, r
        assert r["upper"] <= dense + eps + 1e-9, (r, dense)
    x, y = r["point_xy"]
    assert r["upper"] == o.sdf_at_time(x, y, r["t_witness"]), r
    assert 0 <= r["point_index"] < len(pts) and (x, y) == tuple(np.asarray(pts)[r["point_index"], :2]), r
    assert 0.0 <= r["t_witness"] <= T.sum()
    assert _same(r, ctx.min_clearance(coeffs, T, eps=eps, **kw))
    return r


def _traj(rng, N, trial):
    """The trajectory recipe of test_gpu_sdf_at.py: generic durations (the chain) in trial 0, dyadic 2.5 s in trial 1."""
    import svsdf_amd
    T = rng.uniform(0.4, 3.0, N) if trial % 2 == 0 else np.full(N, 2.5)
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3))
    hs[:2, 0] = rng.uniform(0, 10, 2); ts[:2, 0] = hs[:2, 0] + rng.uniform(-10, 10, 2)
    hs[2, 0] = rng.uniform(-3, 3); ts[2, 0] = rng.uniform(-3, 3)
    q = np.column_stack([np.linspace(hs[0, 0], ts[0, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         np.linspace(hs[1, 0], ts[1, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         rng.uniform(-2.5, 2.5, N - 1)])
    return svsdf_amd.minco_coeffs(hs, ts, q, T), T, hs, ts


class Case:
    """A shape, a trajectory, a cloud, the oracle on them and the dense minimum (computed once, shared)."""

    def __init__(self, shape, trial, P=300, N=5, far=False, seed=None):
        from svsdf_amd import workload
        self.shape = shape
        rng = np.random.default_rng((2000 if seed is None else seed) + 10 * SHAPES.index(shape) + trial)
        pp = (0.0, 0.0, 0.0) if (shape == "Polygon" or trial) else tuple(rng.uniform(-1, 1, 2)) + (float(rng.uniform(-180, 180)),)
        self.coeffs, self.T, hs, ts = _traj(rng, N, trial)
        self.kw = dict(poly_params=pp, polygon=workload.star_outline() if shape == "Polygon" else None, head_state=hs, tail_state=ts)
        self.o = orc.Oracle(shape, **self.kw)
        self.o.set_traj(self.coeffs, self.T)
        self.o.set_modes(1, 0)          # device-library trig, the reference's piece location
        pos = np.array([self.o.pos(t)[:2] for t in rng.uniform(0.0, self.T.sum(), P)])
        if far:                          # 20 to 40 m from the path: the yaw-rate term W |p - x| carries the bound
            ang, rad = rng.uniform(0, 2 * np.pi, P), rng.uniform(20.0, 40.0, P)
            off = np.column_stack([rad * np.cos(ang), rad * np.sin(ang)])
        else:                            # path positions + N(0, 3 m): a share of the points is interior
            off = rng.normal(0.0, 3.0, (P, 2))
        self.pts = np.column_stack([pos + off, np.zeros(P)])
        ctx = self.ctx()
        self.dense = _dense_min(ctx, self.coeffs, self.T, self.pts)
        ctx.close()

    def ctx(self, **extra):
        import svsdf_amd
        c = svsdf_amd.SvsdfContext(shape=self.shape, **{**dict(device=0), **self.kw, **extra})
        c.set_points(self.pts)
        return c


@functools.lru_cache(maxsize=None)
def case1(shape, trial):
    return Case(shape, trial)


@pytest.mark.parametrize("trial", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape(built, shape, trial):
    c = case1(shape, trial)
    ctx = c.ctx()
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense)
    assert r["status"] == "CONVERGED", r
    ctx.close()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_tile_tails(built, P):
    c = Case("star", 0, P=P, N=3, seed=3000 + P)
    ctx = c.ctx()
    # (the automatic budget, 4 P ceil(sum T / 0.15), is a few hundred evaluations at these sizes: not what this test is about)
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, max_evals=100000)
    assert r["status"] == "CONVERGED" and r["tile_pairs"] % ((P + 63) // 64) == 0, r
    ctx.close()


def test_yaw_rate_term(built):
    """Points 20 to 40 m away under yaw waypoints in +-2.5 rad: the robot's far side sweeps metres per level-0 interval, and
    only the W |p - x(m)| term accounts for it.  (A CPU prototype's bracket on such an input: 11.581997 to 11.582951.)"""
    c = Case("sdHorseshoe", 0, far=True, seed=4000)
    ctx = c.ctx()
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense)
    assert r["status"] == "CONVERGED" and r["lower"] > 0.0, r
    ctx.close()


def _straight(shape, pts_of, eps=1e-6):
    """Rest to rest along +x with the yaw fixed at 0; pts_of(R) builds the cloud from the shape's bound radius."""
    import svsdf_amd
    N = 4
    T = np.array([1.7, 2.3, 1.9, 2.1]) * 1.01
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3)); ts[0, 0] = 20.0
    q = np.column_stack([np.linspace(0.0, 20.0, N + 1)[1:-1], np.zeros(N - 1), np.zeros(N - 1)])
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(head_state=hs, tail_state=ts)
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0, **kw)
    pts = pts_of(ctx.shape_bound()[0])
    ctx.set_points(pts)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    r = _check(ctx, o, coeffs, T, pts, eps, _dense_min(ctx, coeffs, T, pts))
    ctx.close()
    return r, T


def test_end_points(built):
    """The nearest point sits behind the start pose, then ahead of the end pose, on the line of motion and outside the
    shape's bounding circle: every point of the shape moves away from (towards) it, so the minimum is at t = 0 (sum T)."""
    far = np.column_stack([np.linspace(-10, 30, 80), np.where(np.arange(80) % 2, 40.0, -40.0), np.zeros(80)])
    r, T = _straight("star", lambda R: np.vstack([far, [[-(R + 1.5), 0.0, 0.0]]]))
    assert r["status"] == "CONVERGED" and r["point_index"] == 80 and r["t_witness"] <= 0.15, r
    r, T = _straight("star", lambda R: np.vstack([[[20.0 + R + 1.5, 0.0, 0.0]], far]))
    assert r["status"] == "CONVERGED" and r["point_index"] == 0 and r["t_witness"] >= T.sum() - 0.15, r


def test_global_not_local(built):
    """Out along y = 0, back along y = 1.5, past an obstacle that the way back comes 1.5 m closer to: the certified minimum is
    the second pass's, whatever basin the per-point solves of svsdf_query_points fell into."""
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
    dense = _dense_min(ctx, coeffs, T, pts)
    assert dense > 0.0
    r = _check(ctx, o, coeffs, T, pts, 1e-3, dense)
    sdf = ctx.query_points(coeffs, T)[0]
    print("query_points min", sdf.min(), "certified", r["lower"], r["upper"])
    assert r["status"] == "CONVERGED" and r["upper"] <= sdf.min() + 1e-3, (r, sdf.min())
    assert r["t_witness"] > T[:3].sum(), r          # after the turn: on the way back
    ctx.close()


def test_target(built):
    c = case1("star", 0)
    assert c.dense < 0.0                             # the cloud has interior points
    ctx = c.ctx()
    full = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense)
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, target=c.dense - 0.5)
    assert r["status"] == "SAFE" and r["lower"] >= c.dense - 0.5 and r["evals"] <= full["evals"], (r, full)
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, target=c.dense + 0.5)
    assert r["status"] == "UNSAFE" and r["upper"] < c.dense + 0.5, r
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, target=0.0)
    assert r["status"] == "UNSAFE" and r["levels"] == 1 and r["upper"] < 0.0, r
    ctx.close()


def test_budget(built):
    """A budget of exactly level 0's evaluations: the search stops there with BUDGET and a bracket that still holds."""
    c = case1("sdHorseshoe", 0)
    ctx = c.ctx()
    level0 = ctx.min_clearance(c.coeffs, c.T, target=1e300)          # UNSAFE after level 0: its evaluation count
    assert level0["status"] == "UNSAFE" and level0["levels"] == 1
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, max_evals=level0["evals"])
    assert r["status"] == "BUDGET" and r["levels"] == 1 and r["evals"] == level0["evals"], r
    ctx.close()


@pytest.mark.parametrize("shape", ["star", "sdHorseshoe"])
def test_capacity(built, shape):
    """pair_capacity = 64: every level's frontier goes through the slices; nothing reported depends on it."""
    c = case1(shape, 0)
    ctx = c.ctx()
    auto = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense)
    small = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense, pair_capacity=64)
    assert auto["pairs"] > 64 and _same(auto, small), (auto, small)
    assert _same(auto, ctx.min_clearance(c.coeffs, c.T, pair_capacity=1000))
    ctx.close()


def test_tight_eps(built):
    c = case1("sdHeart", 0)
    ctx = c.ctx()
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-6, c.dense)
    assert r["status"] == "CONVERGED" and r["levels"] > 8, r
    ctx.close()


def test_context_state(built):
    import svsdf_amd
    base = svsdf_amd.live_allocations()
    c = case1("star", 1)
    ctx = c.ctx()
    e0 = ctx.eval_penalty(c.coeffs, c.T)
    s0 = ctx.stats()
    r = ctx.min_clearance(c.coeffs * 1.01, c.T * 1.1)              # another trajectory, generic durations
    assert r["lower"] <= r["upper"] and r["evals"] > 0
    assert ctx.stats() == s0
    e1 = ctx.eval_penalty(c.coeffs, c.T)
    assert e0[0] == e1[0] and np.array_equal(e0[1], e1[1]) and np.array_equal(e0[2], e1[2])
    # and against a context that never ran the search: evaluation by evaluation the same bits
    ref = c.ctx()
    f0 = ref.eval_penalty(c.coeffs, c.T)
    f1 = ref.eval_penalty(c.coeffs, c.T)
    assert e0[0] == f0[0] and e1[0] == f1[0] and np.array_equal(e1[2], f1[2]) and np.array_equal(e1[1], f1[1])
    ref.close()
    ctx.close()
    assert svsdf_amd.live_allocations() == base


def test_refusals(built):
    import svsdf_amd
    c = case1("star", 0)
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0, **c.kw)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(3\)"):               # SVSDF_ERR_NO_POINTS
        ctx.min_clearance(c.coeffs, c.T)
    ctx.set_points(c.pts)
    ctx.set_scale(**svsdf_amd.binding.EXAMPLE_SCALE)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\).*scale"):
        ctx.min_clearance(c.coeffs, c.T)
    ctx.set_scale(None)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\).*300"):
        ctx.min_clearance(c.coeffs, np.full(5, 60.0))
    bad = c.coeffs.copy(); bad[7, 1] = np.nan
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(4\)"):               # SVSDF_ERR_NONFINITE
        ctx.min_clearance(bad, c.T)
    assert ctx.min_clearance(c.coeffs, c.T)["status"] == "CONVERGED"               # and the context still works
    ctx.set_points(np.zeros((0, 3)))
    r = ctx.min_clearance(c.coeffs, c.T)
    assert r["lower"] == r["upper"] == np.inf and r["point_index"] == -1, r
    ctx.close()


def test_group(built):
    """Three stripes (on one device): each searched on its own, combined on the host; the index is the original one."""
    c = case1("star", 0)
    single = c.ctx()
    one = single.min_clearance(c.coeffs, c.T)
    single.close()
    ctx = c.ctx(devices=[0, 0, 0])
    r = _check(ctx, c.o, c.coeffs, c.T, c.pts, 1e-3, c.dense)
    assert r["status"] == "CONVERGED" and abs(r["upper"] - one["upper"]) <= 1e-3, (r, one)
    ctx.close()


def test_reference_map(built):
    """The star demo's whole map -- every occupied voxel centre, not the corridor the optimiser sees -- against the
    24-piece trajectory of the benchmark's reference_scale case."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.reference_case("star", N=24, iterates=1)
    sc = ASSETS["scenarios"]["star"]
    pts = _voxel_centres(np.array(ASSETS["maps"]["star"], dtype=np.float32), sc["occupancy_resolution"])
    assert len(pts) > 100
    kw = dict(poly_params=w["poly_params"], head_state=w["head_state"], tail_state=w["tail_state"])
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0, **kw)
    coeffs, T = ctx.lmbm_prepare(w["xs"][0])
    ctx.set_points(pts)
    o = orc.Oracle("star", **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    r = _check(ctx, o, coeffs, T, pts, 1e-3, _dense_min(ctx, coeffs, T, pts))
    assert r["status"] in ("CONVERGED", "BUDGET"), r
    ctx.close()
