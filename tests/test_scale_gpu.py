"""Time-varying robot scale on the MI355X (svsdf_set_scale).

  * Identity schedule (c = 1, A = 0) on every compiled shape id (17 = the Polygon with its edges in LDS, 16 with them in
    global memory) and at the reference's scale: the launch record shows the scaled kernels ran, and every per-point sdf,
    t*, gradient and the cost / gradient sums are bit-identical to the rigid path.  Clearing the schedule gives the bits of
    a context that never had one.
  * The reference's example schedule on star, sdHorseshoe, sdHeart and a Polygon outline, clouds with interior points
    (GSIP): the results differ from the rigid ones; every plan the scaled path can take -- bound modes, batches, lanes,
    a pinned tail (ignored), the culls' switch -- gives the same bits; an exterior point's sdf is the scaled evaluation at
    its t* (svsdf_debug_sdf_at, bit for bit), and that evaluation matches the arithmetic restated in Python on the device's
    pose; two stripes on one GPU match one device per point; the full callback and the outline honour the schedule.
"""
import math
import os

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu

SHAPES = ["sdUnevenCapsule", "sdCutDisk", "sdTrapezoid", "sdRhombus", "star", "sdTunnel", "sdHorseshoe", "sdHeart",
          "sdOrientedVesica", "sdRoundedCross", "sdRoundedX", "bigX", "sdMoon", "sdPie", "sdPie2", "sdArc", "Polygon"]
OFFSETS = {"sdCutDisk": (0.0, -0.6, 0.0), "sdHeart": (0.3, -0.4, 25.0), "sdArc": (-0.4, 0.5, -140.0),
           "star": (0.5, 0.2, 10.0), "sdTrapezoid": (0.2, 0.1, 70.0)}
OUTLINE = np.array([[1.6, 0.0], [0.7, 1.1], [-0.5, 1.3], [-1.4, 0.2], [-0.9, -1.1], [0.8, -1.2]])
IDENT = dict(c=(1.0, 1.0), amp=(0.0, 0.0), omega=(1.5, 1.8), phase=(-1.0, 0.0))
EXAMPLE = dict(c=(0.8, 0.8), amp=(0.6, 0.4), omega=(1.5, 1.8), phase=(-1.0, 0.0))
RIGID_KINDS = {"solve", "classify", "tail", "reduce"}
SCALED_KINDS = {"solve_scaled", "classify_scaled", "reduce_scaled"}


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _case(sid, seed=0):
    import svsdf_amd
    shape = SHAPES[min(sid, 16)]
    rng = np.random.default_rng(9100 + sid + 100 * seed)
    T = np.array([1.3, 2.2, 0.9, 1.7]) * rng.uniform(0.9, 1.1, 4)
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:, 0] = [0.0, 0.0, 0.4]
    ts[:, 0] = [14.0, 5.0, -1.2]
    q = np.array([[4.0, 3.0, 1.1], [8.0, 1.5, -0.6], [11.0, 4.5, 0.8]]) + rng.uniform(-0.5, 0.5, (3, 3))
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, poly_params=OFFSETS.get(shape, (0.0, 0.0, 0.0)),
              polygon=OUTLINE if shape == "Polygon" else None, head_state=hs, tail_state=ts)
    env = {"SVSDF_POLY_LDS": 0} if sid == 16 else {}
    return shape, kw, coeffs, T, env


def _cloud(shape, kw, coeffs, T, n, R, seed):
    """n points around the path: about a third inside the swept volume (GSIP), the rest outside."""
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    rng = np.random.default_rng(seed)
    tt = rng.uniform(0.0, T.sum(), n)
    pos = np.array([o.pos(t)[:2] for t in tt])
    ang, rad = rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.6, n))
    pts = np.zeros((n, 3))
    pts[:, 0] = pos[:, 0] + rad * np.cos(ang)
    pts[:, 1] = pos[:, 1] + rad * np.sin(ang)
    return pts


def _ctx(shape, kw, env, **extra):
    import svsdf_amd
    return _with_env(env, lambda: svsdf_amd.SvsdfContext(shape=shape, device=0, **kw, **extra))


def _run(ctx, coeffs, T):
    """per-point results (query_points) and the sums (eval_penalty), with the kernel kinds of each evaluation"""
    q = ctx.query_points(coeffs, T)
    kq = {r["kernel"] for r in ctx.last_launches()}
    cost, gT, gC = ctx.eval_penalty(coeffs, T)
    recs = ctx.last_launches()
    kp = {r["kernel"] for r in recs}
    return {"q": [np.asarray(a, dtype=np.float64).copy() for a in q], "cost": float(cost), "gT": np.asarray(gT).copy(),
            "gC": np.asarray(gC).copy(), "kinds": kq | kp, "recs": recs}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what=""):
    assert len(a["q"]) == len(b["q"])
    for k, (x, y) in enumerate(zip(a["q"], b["q"])):
        bad = np.flatnonzero((_bits(x) != _bits(y)).reshape(len(x), -1).any(axis=1))
        assert bad.size == 0, f"{what}: per-point output {k} differs at {bad.size} points, first {bad[:5]}"
    assert _bits(a["cost"]) == _bits(b["cost"]), (what, a["cost"], b["cost"])
    assert np.array_equal(_bits(a["gT"]), _bits(b["gT"])), what
    assert np.array_equal(_bits(a["gC"]), _bits(b["gC"])), what


@pytest.mark.parametrize("sid", list(range(18)))
def test_identity_schedule_is_the_rigid_path(built, sid):
    shape, kw, coeffs, T, env = _case(sid)
    ctx = _ctx(shape, kw, env)
    pts = _cloud(shape, kw, coeffs, T, 2500, ctx.shape_bound()[0], 500 + sid)
    ctx.set_points(pts)
    rigid = _run(ctx, coeffs, T)
    assert rigid["kinds"] & {"solve"} and not rigid["kinds"] & SCALED_KINDS
    assert (rigid["q"][0] <= 0).sum() >= 50, "the cloud needs interior points (GSIP)"
    ctx.set_scale(**IDENT)
    sc = _run(ctx, coeffs, T)
    assert SCALED_KINDS <= sc["kinds"] and not sc["kinds"] & RIGID_KINDS, sc["kinds"]
    assert {r["shape"] for r in sc["recs"] if r["kernel"] in ("solve_scaled", "classify_scaled")} <= {sid, min(sid, 16)}
    assert sid in {r["shape"] for r in sc["recs"] if r["kernel"] == "solve_scaled"}
    _same(rigid, sc, f"identity schedule, shape id {sid}")
    # reset: the bits of a context that never had a schedule
    ctx.set_scale(None)
    back = _run(ctx, coeffs, T)
    assert not back["kinds"] & SCALED_KINDS
    fresh = _ctx(shape, kw, env)
    fresh.set_points(pts)
    _same(_run(fresh, coeffs, T), back, f"reset, shape id {sid}")
    fresh.close()
    ctx.close()


def test_identity_schedule_at_reference_scale(built):
    """~ 100 points, full callback: the one-block reduction, the solo solve, the launch chain instead of the fused tail."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C1", P=110, minco=svsdf_amd.minco_coeffs)
    x = workload.x_from(w["q"], w["T"], svsdf_amd.backward_T)
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], head_state=w["head_state"],
              tail_state=w["tail_state"])
    ctx = svsdf_amd.SvsdfContext(shape=w["shape"], device=0, **kw)
    ctx.set_points(w["points"])
    out = []
    for sched in (None, IDENT):
        if sched is None:
            ctx.set_scale(None)
        else:
            ctx.set_scale(**sched)
        f, g = ctx.lmbm_evaluate(x)
        kinds = {r["kernel"] for r in ctx.last_launches()}
        out.append((f, g.copy(), kinds))
    assert _bits(out[0][0]) == _bits(out[1][0]) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    assert SCALED_KINDS <= out[1][2] and not out[1][2] & RIGID_KINDS
    ctx.close()


EXAMPLE_SIDS = [4, 6, 7, 17]   # star, sdHorseshoe, sdHeart, the star.obj Polygon outline (edges in LDS)


def _example(sid):
    from svsdf_amd import workload
    shape, kw, coeffs, T, env = _case(sid, seed=1)
    if shape == "Polygon":
        kw["polygon"] = workload.mesh_outline("star")   # the 77-vertex z = 0 section of the reference's star.obj
    ctx = _ctx(shape, kw, env)
    pts = _cloud(shape, kw, coeffs, T, 1500, ctx.shape_bound()[0], 800 + sid)
    ctx.set_points(pts)
    return shape, kw, coeffs, T, env, ctx, pts


@pytest.mark.parametrize("sid", EXAMPLE_SIDS)
def test_example_schedule_acts_and_plans_agree(built, sid):
    shape, kw, coeffs, T, env, ctx, pts = _example(sid)
    rigid = _run(ctx, coeffs, T)
    ctx.set_scale(**EXAMPLE)
    base = _run(ctx, coeffs, T)
    assert SCALED_KINDS <= base["kinds"] and not base["kinds"] & RIGID_KINDS
    sdf = base["q"][0]
    assert np.isfinite(sdf).all() and (sdf <= 0).sum() >= 30, "interior points (GSIP) under the schedule"
    moved = (_bits(sdf) != _bits(rigid["q"][0])).sum()
    assert moved > len(sdf) // 4 and base["cost"] != rigid["cost"], "the scale must visibly act"
    plan = ctx.get_plan()
    assert plan["tail_iter"] == -2 and plan["lanes_per_query"] in (4, 8, 32)
    # every plan of the scaled path: same bits
    for label, p in [("mode %d" % m, dict(bound_mode=m)) for m in range(4)] + \
                    [("batches 3", dict(batches=3)), ("batches 1", dict(batches=1)), ("tail pinned", dict(tail_iter=0))] + \
                    [("lanes %d" % g, dict(lanes_per_query=g)) for g in (2, 4, 8, 16, 32)]:
        ctx.set_plan(**p)
        r = _run(ctx, coeffs, T)
        assert not r["kinds"] & RIGID_KINDS, label
        _same(base, r, f"shape id {sid}, {label}")
        ctx.set_plan()
    # the culls' switch and the Lipschitz devices do not enter the scaled path
    for e in ({"SVSDF_CULL": 0}, {"SVSDF_ASSUME_NOT_LIPSCHITZ": 1}, {"SVSDF_SCAN_ANCHORS": 0}):
        c2 = _ctx(shape, kw, {**env, **e})
        c2.set_points(pts)
        c2.set_scale(**EXAMPLE)
        _same(base, _run(c2, coeffs, T), f"shape id {sid}, {e}")
        c2.close()
    # the schedule survives set_points / set_conditions
    ctx.set_points(pts)
    ctx.set_conditions(kw["head_state"], kw["tail_state"])
    _same(base, _run(ctx, coeffs, T), f"shape id {sid}, after set_points / set_conditions")
    ctx.close()


@pytest.mark.parametrize("sid", EXAMPLE_SIDS)
def test_exterior_value_is_the_scaled_evaluation_at_t_star(built, sid):
    """An exterior point's result is the descent's value: the scaled evaluation at its t* (svsdf_debug_sdf_at under the
    same schedule, bit for bit).  And that evaluation is the arithmetic of SWM:528-535 restated here on the device's pose:
    s_a(t) with libm sin, S^-1 by cofactors, u = (Rt^T S^-1)(p - x), the shape SDF of the oracle."""
    shape, kw, coeffs, T, env, ctx, pts = _example(sid)
    # exterior under the schedule whatever the shape does: rigid swept value > 1.5 R (R: circumradius) means |p - x(t)| > 2.5 R
    # at every t, and |S^-1 d| >= |d| / 1.4 - R > 0 for s <= 1.4.  (A positive result of an INTERIOR point is -r* of its
    # GSIP rounds, not an evaluation.)
    R = ctx.shape_bound()[0]
    far = _cloud(shape, kw, coeffs, T, 600, 3.0 * R, 900 + sid)     # out to 3.8 R from a pose ...
    pts = np.concatenate([pts, far])
    ctx.set_points(pts)
    rig = np.asarray(ctx.query_points(coeffs, T)[0]).copy()
    ctx.set_scale(**EXAMPLE)
    sdf, tst = ctx.query_points(coeffs, T)[:2]
    sdf, tst = np.asarray(sdf).copy(), np.asarray(tst).copy()
    ext = np.flatnonzero(rig > 1.5 * R)[:400]
    assert len(ext) >= 50
    out = ctx.debug_sdf_at(coeffs, T, pts[ext, :2], tst[ext])
    assert np.array_equal(_bits(out[:, 0]), _bits(sdf[ext]))
    # restatement
    u = np.zeros((len(ext), 2))
    for k, (i, t) in enumerate(zip(ext, tst[ext])):
        sx = EXAMPLE["c"][0] + math.sin(EXAMPLE["omega"][0] * t + EXAMPLE["phase"][0]) * EXAMPLE["amp"][0]
        sy = EXAMPLE["c"][1] + math.sin(EXAMPLE["omega"][1] * t + EXAMPLE["phase"][1]) * EXAMPLE["amp"][1]
        inv = 1.0 / (sy * sx)
        i00, i11 = sy * inv, sx * inv
        x, y, cs, sn = out[k, 1:5]
        dx, dy = pts[i, 0] - x, pts[i, 1] - y
        u[k] = ((cs * i00) * dx + (sn * i11) * dy, ((-sn) * i00) * dx + (cs * i11) * dy)
    np.testing.assert_allclose(out[:, 5:7], u, rtol=0, atol=1e-13)
    ref = np.array([float(orc.shape_sdf(shape, float(ux), float(uy), poly_params=kw["poly_params"], polygon=kw["polygon"]))
                    for ux, uy in u])
    np.testing.assert_allclose(out[:, 0], ref, rtol=0, atol=1e-12)
    # the rigid debug value differs: the schedule reaches the unit of work
    ctx.set_scale(None)
    rig = ctx.debug_sdf_at(coeffs, T, pts[ext, :2], tst[ext])
    assert (rig[:, 0] != out[:, 0]).mean() > 0.9
    ctx.close()


def test_two_stripes_on_one_gpu_match_one_device(built):
    import svsdf_amd
    sid = 6
    shape, kw, coeffs, T, env = _case(sid, seed=1)
    one = _ctx(shape, kw, env)
    pts = _cloud(shape, kw, coeffs, T, 3000, one.shape_bound()[0], 77)
    one.set_points(pts)
    one.set_scale(**EXAMPLE)
    a = one.query_points(coeffs, T)
    ca, gTa, gCa = one.eval_penalty(coeffs, T)
    two = _ctx(shape, kw, env, devices=[0, 0], combine=svsdf_amd.COMBINE_HOST)
    two.set_scale(**EXAMPLE)                 # before set_points: the schedule belongs to the context
    two.set_points(pts)
    assert two.get_scale() == {k: tuple(v) for k, v in EXAMPLE.items()}
    b = two.query_points(coeffs, T)
    cb, gTb, gCb = two.eval_penalty(coeffs, T)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert abs(ca - cb) <= 1e-12 * abs(ca)   # (the two stripes' partials are summed in another order)
    np.testing.assert_allclose(gCb, gCa, rtol=1e-10, atol=1e-12 * np.abs(gCa).max())
    np.testing.assert_allclose(gTb, gTa, rtol=1e-10, atol=1e-12 * np.abs(gTa).max())
    two.close()
    one.close()


def test_full_callback_and_outline_honour_the_schedule(built):
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C1", P=3000, minco=svsdf_amd.minco_coeffs)
    x = workload.x_from(w["q"], w["T"], svsdf_amd.backward_T)
    ctx = svsdf_amd.SvsdfContext(shape=w["shape"], safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"],
                                 head_state=w["head_state"], tail_state=w["tail_state"], device=0)
    ctx.set_points(w["points"])
    f0, g0 = ctx.lmbm_evaluate(x)
    g0 = g0.copy()
    ctx.set_scale(**EXAMPLE)
    f1, g1 = ctx.lmbm_evaluate(x)
    g1 = g1.copy()
    assert SCALED_KINDS <= {r["kernel"] for r in ctx.last_launches()}
    f2, g2 = ctx.lmbm_evaluate(x)
    assert _bits(f1) == _bits(f2) and np.array_equal(_bits(g1), _bits(g2))     # reproducible
    assert np.isfinite(f1) and np.isfinite(g1).all() and f1 != f0 and not np.array_equal(g0, g1)
    # the outline of the swept volume (sw_calculate runs <useScale> too) changes its area under the schedule
    coeffs, T = ctx.lmbm_prepare(x)
    loops1, _ = ctx.swept_outline(coeffs, T, cell=0.1)
    ctx.set_scale(None)
    loops0, _ = ctx.swept_outline(coeffs, T, cell=0.1)
    area = lambda ls: sum(abs(0.5 * np.sum(l[:, 0] * np.roll(l[:, 1], -1) - np.roll(l[:, 0], -1) * l[:, 1])) for l in ls)
    a1, a0 = area(loops1), area(loops0)
    assert a1 > 0 and a0 > 0 and abs(a1 - a0) > 1e-3 * a0, (a0, a1)
    ctx.close()
