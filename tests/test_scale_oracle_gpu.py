"""The scaled kernels (svsdf_set_scale) against the C oracle's useScale path, bit for bit.

The oracle runs in device-arithmetic mode (orc set_modes(1, 0): the device library's sin / cos / atan2 -- the schedule's
sine among them --, the reference's piece location) under the same schedule as the library; tests/test_oracle_scale.py pins
that oracle to the pure-Python restatement on the CPU.  Trajectories and clouds are those of tests/test_scale_gpu.py: four
generic-duration pieces, points out to sqrt(1.6) R around the path, about a third of them interior (GSIP).  Schedules: A the
reference's example, B anisotropic with s_x up to 1.45, C constant (0.7, 1.3).
  a. the unit of work: k_debug_sdf_at_sc on 512 (point, time) pairs, every piece boundary and its ulp neighbours among the
     times, equals orc_rel_at_time (sdf, u_x, u_y) on all 18 shape ids under A and B -- the triage point for the rest;
  b. every scaled instantiation: per shape id three clouds that show the three forms of k_reduce_sc in the launch record
     (one block; 2 - 4 blocks fused; more, with k_final / k_finish), per point sdf, t* and gradient bit for bit, the sums to
     summation order (1e-12), the solve at widths 4, 8 and 32 and in three batches with the same bits, no rigid kernel kind
     in any record; and the large cloud against the oracle of record (libm trig) at the project's gates;
  c. 1, 65 and 128 generic pieces and 32 coarse ones with the layer-2 / layer-3 pose tables forced on and off;
  d. the full callback at the reference's scale (~ 100 points) against the oracle's callback;
  e. 24 seeded random cases: shape id, schedule, 3 - 6 pieces.
Every case asserts its own count of interior points (main solve <= 0, the oracle's counter) and that the schedule acted.
Which kernel ran is read from the launch record.
"""
import os

import numpy as np
import pytest

from oracle import orc
from test_scale_gpu import EXAMPLE, OFFSETS, OUTLINE, RIGID_KINDS, SCALED_KINDS, SHAPES, _case, _cloud, _ctx, _with_env

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)

A = EXAMPLE                                                                        # the reference's example (EXAMPLE_SCALE)
B = dict(c=(1.1, 0.9), amp=(0.35, 0.3), omega=(0.9, 2.3), phase=(0.4, -2.0))       # anisotropic, s_x up to 1.45
C = dict(c=(0.7, 1.3), amp=(0.0, 0.0), omega=(0.0, 0.0), phase=(0.0, 0.0))         # constant
SCHEDULES = {"A": A, "B": B, "C": C}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _oracle(shape, kw, coeffs, T, sched, modes=(1, 0)):
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    o.set_modes(*modes)
    if sched is not None:
        o.set_scale(**sched)
    return o


def _per_point(o, pts, sub=None):
    """the oracle's sums, per-point sdf / t*, the gradient of pts[sub], and how many main solves were <= 0"""
    cost, gT, gC, sdf, ts, _ = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
    n_in = o.counters()["interior_points"]
    sub = np.arange(len(pts)) if sub is None else sub
    g = o.query(pts[sub], nthreads=NT)[2]
    return dict(cost=cost, gT=gT, gC=gC, sdf=sdf, ts=ts, g=g, sub=sub, interior=n_in)


def _assert_per_point(what, got, ref):
    sdf, ts, g = got
    bad_s, bad_t = _bits(sdf) != _bits(ref["sdf"]), _bits(ts) != _bits(ref["ts"])
    bad_g = (_bits(g[ref["sub"]]) != _bits(ref["g"])).any(axis=1)
    inner = ref["sdf"] <= 0
    msg = (what, f"sdf {int(bad_s.sum())} (of them interior-valued {int((bad_s & inner).sum())}), t* {int(bad_t.sum())}, "
                 f"gradient {int(bad_g.sum())} of {len(sdf)} points differ", np.flatnonzero(bad_s | bad_t)[:5])
    assert not bad_s.any() and not bad_t.any() and not bad_g.any(), msg


# ------------------------------------------------------------------------------------------ a. the unit of work
def _pairs(shape, kw, coeffs, T, tt, R, rng):
    """one point per time, placed around the pose of ITS time the way _cloud places points around the path (out to
    sqrt(1.6) R; every other one at 0.35 of that: the schedules shrink the robot to 0.2 of its size), so that the pairs lie
    on both sides of the scaled shape's zero set"""
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    pos = np.array([o.pos(float(t))[:2] for t in tt])
    ang, rad = rng.uniform(0, 2 * np.pi, len(tt)), R * np.sqrt(rng.uniform(0, 1.6, len(tt)))
    rad[1::2] *= 0.35
    return np.column_stack([pos[:, 0] + rad * np.cos(ang), pos[:, 1] + rad * np.sin(ang)])


@pytest.mark.parametrize("sid", list(range(18)))
def test_a_unit_of_work_equals_orc_rel_at_time(built, sid):
    shape, kw, coeffs, T, env = _case(sid)
    ctx = _ctx(shape, kw, env)
    n = 512
    rng = np.random.default_rng(4200 + sid)
    cum = np.cumsum(T)                       # left to right, like the durations' own sum
    dur = float(cum[-1])
    edge = [0.0, np.nextafter(0.0, 1.0), dur, np.nextafter(dur, 0.0)]
    for s in cum[:-1]:
        edge += [float(s), np.nextafter(s, 0.0), np.nextafter(s, np.inf)]
    tt = np.concatenate([np.tile(edge, 8), rng.uniform(0.0, dur, n - 8 * len(edge))])
    assert len(tt) == n
    pxy = _pairs(shape, kw, coeffs, T, tt, ctx.shape_bound()[0], rng)
    rigid = ctx.debug_sdf_at(coeffs, T, pxy, tt)
    for name in ("A", "B"):
        ctx.set_scale(**SCHEDULES[name])
        out = ctx.debug_sdf_at(coeffs, T, pxy, tt)
        assert out[:, 7].min() >= 1, "generic durations: the chain locates the piece"
        ref = _oracle(shape, kw, coeffs, T, SCHEDULES[name]).rel_at_time(pxy, tt)
        bad = [int((_bits(out[:, k]) != _bits(ref[:, j])).sum()) for k, j in ((0, 0), (5, 1), (6, 2))]
        first = np.flatnonzero((_bits(out[:, [0, 5, 6]]) != _bits(ref)).any(axis=1))[:3]
        assert bad == [0, 0, 0], (sid, name, "sdf / u_x / u_y differ at", bad, first, tt[first], out[first][:, [0, 5, 6]], ref[first])
        assert (out[:, 5] != rigid[:, 5]).mean() > 0.9 and (out[:, 0] != rigid[:, 0]).mean() > 0.5, "the schedule must act"
        assert (out[:, 0] <= 0).sum() >= 20 and (out[:, 0] > 0).sum() >= 20, "pairs on both sides of the zero set"
    ctx.close()


# ------------------------------------------------------------------------------------------ b. every scaled instantiation
CLOUDS = {"S": (150, 20), "M": (700, 100), "L": (1500, 100)}      # points, least interior points
# The clouds' seed.  The flip cap of the comparison with the oracle of record is a condition on the cloud, like its count of
# interior points, and is met by the reference's arithmetic alone or not at all: a basin flip is a point on a flat stretch of
# SDF(t) whose t* moves under any last-bit change of a sine, and where its two basins differ in value (a GSIP point inside
# the sweep of a concave shape) one such point of 1 500 moves the cost by ~ 3e-5.  With seed 5000 the sdRoundedX cloud held
# one (point 464): the oracle with the device library's trig against the oracle of record, both on the CPU, differ there by
# cost 2.8e-5, gradC 1.1e-3, and so does the oracle of record against itself under every +-1 ulp perturbation of its libm
# (orc set_trig_perturb, seeds 1 - 7: cost 8e-7 ... 3e-5).  With this seed the two oracles agree on all 18 large clouds with 0
# flips, cost <= 2.8e-9, gradT <= 4.1e-8, gradC <= 7.4e-9 -- chosen on the CPU from the two oracles, no device result involved.
CLOUD_SEED = 6000


def _eval(ctx, coeffs, T):
    """two consecutive eval_penalty calls, then the per-point query; every launch record"""
    pens, recs = [], []
    for _ in range(2):
        pens.append(ctx.eval_penalty(coeffs, T))
        recs.append(ctx.last_launches())
    sdf, ts, g, _ = ctx.query_points(coeffs, T)
    recs.append(ctx.last_launches())
    return pens, (np.array(sdf), np.array(ts), np.array(g)), recs


@pytest.mark.parametrize("sid", list(range(18)))
def test_b_every_scaled_instantiation(built, sid):
    shape, kw, coeffs, T, env = _case(sid)
    ctx = _ctx(shape, kw, env)
    R = ctx.shape_bound()[0]
    clouds = {k: _cloud(shape, kw, coeffs, T, n, R, CLOUD_SEED + 10 * sid + i) for i, (k, (n, _)) in enumerate(CLOUDS.items())}
    sub_l = np.random.default_rng(sid).choice(CLOUDS["L"][0], 500, replace=False)
    covered, all_kinds = set(), set()

    def note(recs):
        for rr in recs:
            for r in rr:
                all_kinds.add(r["kernel"])
                if r["kernel"] == "solve_scaled":
                    covered.add(("solve_scaled", r["shape"], r["targ"][0]))
                elif r["kernel"] == "classify_scaled":
                    covered.add(("classify_scaled", r["shape"]))
                elif r["kernel"] == "reduce_scaled":
                    covered.add(("reduce_scaled",))

    base_l = None
    for cls, name in (("S", "A"), ("M", "A"), ("L", "A"), ("L", "B"), ("L", "C")):
        what = (shape, sid, cls, name)
        pts = clouds[cls]
        ctx.set_plan()
        ctx.set_points(pts)
        ctx.set_scale(None)
        rigid_sdf = np.array(ctx.query_points(coeffs, T)[0])
        ctx.set_scale(**SCHEDULES[name])
        ref = _per_point(_oracle(shape, kw, coeffs, T, SCHEDULES[name]), pts, sub_l if cls == "L" else None)
        assert ref["interior"] >= CLOUDS[cls][1], (what, "interior points (main solve <= 0)", ref["interior"])
        assert (_bits(ref["sdf"]) != _bits(rigid_sdf)).sum() > len(pts) // 4, (what, "the schedule must act")
        pens, got, recs = _eval(ctx, coeffs, T)
        note(recs)
        _assert_per_point(what, got, ref)
        for cost, gT, gC in pens:
            assert abs(cost - ref["cost"]) <= 1e-12 * abs(ref["cost"]), (what, cost, ref["cost"])
            assert _rel(gT, ref["gT"]) <= 1e-12 and _rel(gC, ref["gC"]) <= 1e-12, (what, _rel(gT, ref["gT"]), _rel(gC, ref["gC"]))
        assert ref["cost"] > 0 and np.linalg.norm(ref["gC"]) > 0
        assert _bits(pens[0][0]) == _bits(pens[1][0]) and np.array_equal(_bits(pens[0][1]), _bits(pens[1][1])) \
            and np.array_equal(_bits(pens[0][2]), _bits(pens[1][2])), (what, "two consecutive evaluations")
        # the form of the reduction, from the record
        for rr in recs[:2]:
            red = [r for r in rr if r["kernel"] == "reduce_scaled"]
            kinds = {r["kernel"] for r in rr}
            assert red, what
            for r in red:
                if cls == "S":
                    assert r["grid"] == 1 and r["fused"] == 1, (what, r)
                elif cls == "M":
                    assert 2 <= r["grid"] <= 4 and r["fused"] == 1, (what, r)
                else:
                    assert r["grid"] > 4 and r["fused"] == 0, (what, r)
            assert ({"final", "finish"} <= kinds) == (cls == "L"), (what, kinds)
        if (cls, name) == ("L", "A"):
            base_l = (pens[0], got)
    # L under A: every solve width and three batches give the same bits
    ctx.set_points(clouds["L"])
    ctx.set_scale(**A)
    for label, plan, width in [(f"lanes {g}", dict(lanes_per_query=g), g) for g in (4, 8, 32)] + [("batches 3", dict(batches=3), None)]:
        ctx.set_plan(**plan)
        pens, got, recs = _eval(ctx, coeffs, T)
        note(recs)
        for rr in recs:
            # (the main solve, iter 0, runs at the pinned width; the library may widen a round's sample solves)
            widths = {r["targ"][0] for r in rr if r["kernel"] == "solve_scaled" and r["iter"] == 0}
            assert widths and (width is None or widths == {width}), (sid, label, widths)
            if width is None:
                assert len({r["batch"] for r in rr if r["kernel"] == "solve_scaled" and r["iter"] == 0}) == 3, (sid, label)
        for x, y in zip(got, base_l[1]):
            assert np.array_equal(_bits(x), _bits(y)), (sid, label, "per point")
        for p in pens:
            for x, y in zip(p, base_l[0]):
                assert np.array_equal(_bits(x), _bits(y)), (sid, label, "sums")
        ctx.set_plan()
    need = {("solve_scaled", sid, g) for g in (4, 8, 32)} | {("classify_scaled", min(sid, 16)), ("reduce_scaled",)}
    assert need <= covered, sorted(need - covered, key=str)
    # (the rigid queries made for "the schedule must act" are not evaluations under a schedule: `note` never sees them)
    assert SCALED_KINDS <= all_kinds and not all_kinds & RIGID_KINDS, all_kinds
    # the oracle of record (libm trig): L under A at the project's gates
    pts = clouds["L"]
    rec = _per_point(_oracle(shape, kw, coeffs, T, A, modes=(0, 0)), pts, sub_l)
    (cost, gT, gC), (sdf, ts, g) = base_l
    flips = int((np.abs(ts - rec["ts"]) > 1e-4).sum())
    dc, dT, dC = abs(cost - rec["cost"]) / abs(rec["cost"]), _rel(gT, rec["gT"]), _rel(gC, rec["gC"])
    print(f"shape id {sid} ({shape}{', edges in global memory' if sid == 16 else ''}): covered "
          + " ".join("/".join(map(str, k)) for k in sorted(covered, key=str))
          + f"; L under A against the oracle of record: cost {dc:.2e} gradT {dT:.2e} gradC {dC:.2e} basin flips {flips} of {len(pts)}")
    assert dc <= 1e-7 and dT <= 1e-5 and dC <= 1e-5, (sid, dc, dT, dC)
    assert flips <= int(0.002 * len(pts)), (sid, flips)
    ctx.close()


# ------------------------------------------------------------------------------------------ c. piece counts, pose tables
@pytest.mark.parametrize("N,generic", [(1, True), (65, True), (128, True), (32, False)],
                         ids=["1 piece", "65 pieces", "128 pieces", "32 coarse pieces"])
def test_c_piece_counts_and_pose_tables(built, N, generic):
    from test_layer_tables_gpu import _case as lt_case, _ctx as lt_ctx
    w = lt_case("C3", 1500, N=N, generic=generic, seed=N)
    if not generic:
        assert np.all(w["T"] == 2.5)
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], poly_params=w["poly_params"],
              polygon=w["polygon"], head_state=w["head_state"], tail_state=w["tail_state"])
    o = _oracle(w["shape"], kw, w["coeffs"], w["T"], A)
    osdf, ots, og = o.query(w["points"], nthreads=NT)
    n_in = o.counters()["interior_points"]
    assert n_in >= 100, ("interior points (main solve <= 0)", n_in)
    ref = dict(sdf=osdf, ts=ots, g=og, sub=np.arange(len(osdf)))
    ctx = lt_ctx(w)
    rigid_sdf = np.array(ctx.query_points(w["coeffs"], w["T"])[0])
    assert (_bits(osdf) != _bits(rigid_sdf)).sum() > len(osdf) // 4, "the schedule must act"
    ctx.set_scale(**A)
    for tables in (3, 0):
        ctx.set_plan(layer_tables=tables)
        sdf, ts, g, _ = ctx.query_points(w["coeffs"], w["T"])
        recs = ctx.last_launches()
        kinds = {r["kernel"] for r in recs}
        assert [r["targ"][0] for r in recs if r["kernel"] == "layer_tables"] == ([3] if tables else []), (N, tables)
        assert "solve_scaled" in kinds and not kinds & RIGID_KINDS, kinds
        assert ctx.stats()["piece_time_exact"] == (1 if generic else 0)
        _assert_per_point((f"{N} pieces", f"layer_tables {tables}"), (np.array(sdf), np.array(ts), np.array(g)), ref)
    print(f"C3 {N} pieces under A: duration {np.sum(w['T']):.1f} s, {n_in} interior of {len(osdf)}, identical to the oracle")
    ctx.close()


# ------------------------------------------------------------------------------------------ d. the full callback
def test_d_full_callback_at_reference_scale(built):
    """C1 at 110 points (test_scale_gpu.py::test_identity_schedule_at_reference_scale) under A: lmbm_evaluate against the
    oracle's callback in device mode and in mode (0, 0), at the gates test_round5_gpu.py::test_reference_scale_callback holds
    the rigid callback to (the host MINCO and the oracle's may differ in the last bits); per point bit for bit on the
    trajectory the device stage received."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C1", P=110, minco=svsdf_amd.minco_coeffs)
    x = workload.x_from(w["q"], w["T"], svsdf_amd.backward_T)
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], head_state=w["head_state"],
              tail_state=w["tail_state"])
    ctx = svsdf_amd.SvsdfContext(shape=w["shape"], device=0, **kw)
    ctx.set_points(w["points"])
    f0, _ = ctx.lmbm_evaluate(x)
    ctx.set_scale(**A)
    f, g = ctx.lmbm_evaluate(x)
    g = g.copy()
    kinds = {r["kernel"] for r in ctx.last_launches()}
    assert SCALED_KINDS <= kinds and not kinds & RIGID_KINDS, kinds
    assert f != f0, "the schedule must act"
    for modes in ((1, 0), (0, 0)):
        o = orc.Oracle(w["shape"], **kw)
        o.set_modes(*modes)
        o.set_scale(**A)
        fo, go, _ = o.cost_function(w["points"], x, nthreads=NT)
        n_in = o.counters()["interior_points"]
        assert n_in >= 10, ("interior points (main solve <= 0)", n_in)
        print(f"C1 110 points under A, oracle modes {modes}: f {abs(f - fo) / abs(fo):.2e} g {_rel(g, go):.2e}, {n_in} interior")
        assert abs(f - fo) <= 1e-7 * abs(fo) and _rel(g, go) <= 1e-5, (modes, f, fo, _rel(g, go))
    coeffs, T = ctx.lmbm_prepare(x)
    sdf, ts, gp, _ = ctx.query_points(coeffs, T)
    ref = _per_point(_oracle(w["shape"], kw, coeffs, T, A), w["points"])
    _assert_per_point("C1 110 points", (np.array(sdf), np.array(ts), np.array(gp)), ref)
    ctx.close()


# ------------------------------------------------------------------------------------------ e. seeded random cases
def _random_case(k):
    import svsdf_amd
    rng = np.random.default_rng([20240807, k])
    sid = int(rng.integers(0, 18))
    shape = SHAPES[min(sid, 16)]
    c = rng.uniform(0.5, 1.5, 2)
    amp = rng.uniform(-1.0, 1.0, 2) * (c - 0.2)                  # |A_a| <= c_a - 0.2
    sched = dict(c=tuple(c), amp=tuple(amp), omega=tuple(rng.uniform(-3.0, 3.0, 2)), phase=tuple(rng.uniform(-np.pi, np.pi, 2)))
    N = int(rng.integers(3, 7))
    T = rng.uniform(0.9, 2.4, N)                                 # generic durations
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:, 0] = [0.0, 0.0, rng.uniform(-1.0, 1.0)]
    ts[:, 0] = [3.5 * N, rng.uniform(-4.0, 6.0), rng.uniform(-1.5, 1.5)]
    u = (np.arange(N - 1) + 1.0) / N
    q = hs[:, 0] * (1.0 - u[:, None]) + ts[:, 0] * u[:, None] + rng.uniform(-1.5, 1.5, (N - 1, 3)) * [1.0, 1.0, 0.5]
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, poly_params=OFFSETS.get(shape, (0.0, 0.0, 0.0)),
              polygon=OUTLINE if shape == "Polygon" else None, head_state=hs, tail_state=ts)
    env = {"SVSDF_POLY_LDS": 0} if sid == 16 else {}
    return sid, shape, kw, coeffs, T, env, sched


@pytest.mark.parametrize("k", list(range(24)))
def test_e_seeded_random_cases(built, k):
    sid, shape, kw, coeffs, T, env, sched = _random_case(k)
    ctx = _ctx(shape, kw, env)
    pts = _cloud(shape, kw, coeffs, T, 400, ctx.shape_bound()[0], 7000 + k)
    ctx.set_points(pts)
    rigid_sdf = np.array(ctx.query_points(coeffs, T)[0])
    ctx.set_scale(**sched)
    ref = _per_point(_oracle(shape, kw, coeffs, T, sched), pts)
    assert ref["interior"] >= 40, ("interior points (main solve <= 0)", ref["interior"])
    assert (_bits(ref["sdf"]) != _bits(rigid_sdf)).sum() > len(pts) // 4, "the schedule must act"
    pens, got, recs = _eval(ctx, coeffs, T)
    kinds = {r["kernel"] for rr in recs for r in rr}
    assert SCALED_KINDS <= kinds and not kinds & RIGID_KINDS, kinds
    assert sid in {r["shape"] for rr in recs for r in rr if r["kernel"] == "solve_scaled"}
    what = (k, sid, shape, len(T), sched)
    _assert_per_point(what, got, ref)
    for cost, gT, gC in pens:
        assert abs(cost - ref["cost"]) <= 1e-12 * abs(ref["cost"]), (what, cost, ref["cost"])
        assert _rel(gT, ref["gT"]) <= 1e-12 and _rel(gC, ref["gC"]) <= 1e-12, what
    ctx.close()
