"""Generic piece durations, bit for bit, up to 128 pieces: the kernels' piece-local time against the oracle.

Every iterate of an optimisation after the first has generic durations, and then the library locates the piece-local time
with the reference's chain of subtractions (TRJ:498-516; svsdf_stats.piece_time_exact = 1):
chain_local_time (uniform blocks of 4, windows of 8, the per-lane rest, the two boundary comparisons) in every solve
kernel, and locate_local_exact in k_prep's pose table, k_classify's rescans and the assembly.  The oracle settles each
case exactly (orc set_modes(1, 0): the device library's trig and the reference's chain; set_modes(1, 1): the cumulative
form), and test_piece_time_restatement.py pins the oracle itself against the reference's text.

  * unit level: svsdf_debug_sdf_at (the solve kernels' pose_at, one wave per block) at 1 ... 128 pieces, at every partial
    sum, its ulp neighbours and the chain's exact boundaries, sorted / shuffled / partial-wave lane layouts; mode 2 (a
    piece below 1e-6 s) and both forcing flags;
  * pipeline level: the BASELINE workloads under generic durations at throughput-path sizes, every launch plan on one
    32-piece case, a stale trajectory duration at 128 pieces, waves that mix pieces (no Morton sort), a return-to-start
    trajectory, mode 2 end to end.
Per point the SVSDF, t* and gradient must be the oracle's bits; cost, gradT and gradC its sums to summation order (1e-12,
sum_mode 1).  Which path ran is read from the records (stats, last_launches), and each case prints one line saying so.
"""
import os
import time

import numpy as np
import pytest

from oracle import orc
from test_piece_time_restatement import generic_durations, locate_chain, locate_cumulative, partial_sums, probe_times

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
PIECE_COUNTS = [1, 2, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 64, 65, 127, 128]


def _rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _path(N, rng, back=False):
    """Head / tail states and waypoints of an N-piece path (back: it returns to its start, the fuzz's kind 1)."""
    start = rng.uniform(0, 20, 2)
    end = start if back else start + rng.uniform(-15, 15, 2)
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:2, 0], ts[:2, 0] = start, end
    hs[2, 0], ts[2, 0] = rng.uniform(-3, 3), rng.uniform(-3, 3)
    q = np.column_stack([np.linspace(start[0], end[0], N + 1)[1:-1] + rng.uniform(-3, 3, N - 1),
                         np.linspace(start[1], end[1], N + 1)[1:-1] + rng.uniform(-3, 3, N - 1),
                         rng.uniform(-2.5, 2.5, N - 1)]) if N > 1 else np.zeros((0, 3))
    return hs, ts, q


# ---- unit level: svsdf_debug_sdf_at ------------------------------------------------------------------------------------
def _sdf_at_case(T, rng, shape="star", flags=0):
    import svsdf_amd
    N = len(T)
    hs, ts, q = _path(N, rng)
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(head_state=hs, tail_state=ts)
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0, flags=flags, **kw)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    return ctx, o, coeffs


def _layouts(tt, rng):
    """sorted (a wave shares a piece: the uniform blocks and windows run), shuffled (every wave mixes pieces: the __all
    tests fail early, the per-lane rest runs), and a count that is not a multiple of 64 (a partial last wave)."""
    srt = np.sort(tt)
    n = len(srt) - (len(srt) % 64) + 37 if len(srt) % 64 != 37 else len(srt)
    part = np.concatenate([srt, rng.uniform(0.0, srt[-1], max(0, n - len(srt)))])[:n]
    return {"sorted": srt, "shuffled": tt[rng.permutation(len(tt))], "partial": np.sort(part)}


def _check_sdf_at(ctx, o, coeffs, T, tt, rng, want_mode, what):
    """debug_sdf_at vs the oracle's sdf_at_time / pos (whatever modes `o` is in), bit for bit; returns mismatches."""
    pos = np.array([o.pos(t)[:2] for t in tt])
    xy = pos + rng.normal(0, 2.0, (len(tt), 2))
    xy[::7] = pos[::7]                                          # on the path: deep interior
    d = ctx.debug_sdf_at(coeffs, T, xy, tt)
    ref = np.array([o.sdf_at_time(x, y, t) for (x, y), t in zip(xy, tt)])
    bad = (d[:, 0] != ref) | (d[:, 1] != pos[:, 0]) | (d[:, 2] != pos[:, 1])
    assert np.all(d[:, 7] == want_mode), (what, np.unique(d[:, 7]))
    return int(bad.sum()), d, ref, pos


@pytest.mark.parametrize("N", PIECE_COUNTS)
def test_debug_sdf_at_chain_is_bit_identical(built, N):
    rng = np.random.default_rng(9000 + N)
    T = generic_durations(N, rng)
    if N >= 12 and N % 4 == 0:                                  # a 1e-3 s piece next to a 3 s one (the comparison margin)
        T[N // 2], T[N // 2 + 1] = 1.0e-3 * (1 + 1e-4 * rng.standard_normal()), 3.0 * (1 + 1e-4 * rng.standard_normal())
    ctx, o, coeffs = _sdf_at_case(T, rng)
    o.set_modes(1, 0)                                           # device-library trig, the reference's chain
    tt = probe_times(T, rng, n_uniform=1500)
    tt = np.concatenate([tt, T.sum() + rng.uniform(0.0, 3.4, 64)])
    for layout, ts in _layouts(tt, rng).items():
        nbad, d, ref, pos = _check_sdf_at(ctx, o, coeffs, T, ts, rng, 1, (N, layout))
        print(f"sdf_at N {N:3d} total {T.sum():8.3f} s mode {int(d[0, 7])} {layout:8s} n {len(ts):5d}: "
              f"{nbad} mismatches")
        bad = np.nonzero((d[:, 0] != ref) | (d[:, 1] != pos[:, 0]))[0]
        assert nbad == 0, (N, layout, nbad, ts[bad[:3]], d[bad[:3], 1], pos[bad[:3], 0])
    ctx.close()


@pytest.mark.parametrize("tiny,mode", [(5e-7, 2), (1e-6, 1)])
def test_debug_sdf_at_mode_two_threshold(built, tiny, mode):
    """A piece shorter than 1e-6 s: the chain keeps every comparison (mode 2); exactly 1e-6 s is still mode 1."""
    rng = np.random.default_rng(77)
    for N, k in ((17, 5), (40, 33), (9, 1)):
        T = rng.uniform(0.3, 4.0, N)
        T[k] = tiny
        ctx, o, coeffs = _sdf_at_case(T, rng)
        o.set_modes(1, 0)
        S = partial_sums(T)
        tt = np.concatenate([probe_times(T, rng, n_uniform=600),
                             np.linspace(max(S[k] - 1e-6, 0.0), S[k + 1] + 1e-6, 200)])   # (the library's t >= 0)
        # MINCO through a 5e-7 s piece can fling the whole path far out; the oracle's device trig is the device library's
        # small-argument path (|yaw| < 2^30), so the case must stay inside it to be settled bit for bit
        assert max(abs(o.pos(t)[2]) for t in tt) < 2.0 ** 30, (N, k, tiny)
        for layout, ts in _layouts(tt, rng).items():
            nbad, d, _, _ = _check_sdf_at(ctx, o, coeffs, T, ts, rng, mode, (N, tiny, layout))
            print(f"sdf_at N {N:3d} piece {k} of {tiny:g} s mode {int(d[0, 7])} {layout:8s}: {nbad} mismatches")
            assert nbad == 0, (N, tiny, layout, nbad)
        ctx.close()


def test_debug_sdf_at_honours_the_piece_time_flags(built):
    """FLAG_FAST_PIECE_TIME on generic durations: the cumulative form, i.e. the oracle's set_modes(1, 1).
    FLAG_EXACT_PIECE_TIME on coarse durations (2.5 s pieces): the chain, whose bits equal the default mode-0 run's and the
    oracle's in both of its modes -- the device-side half of the coarse rule."""
    import svsdf_amd
    rng = np.random.default_rng(31)
    for N in (9, 33, 128):
        T = generic_durations(N, rng)
        ctx, o, coeffs = _sdf_at_case(T, rng, flags=svsdf_amd.FLAG_FAST_PIECE_TIME)
        o.set_modes(1, 1)
        tt = probe_times(T, rng, n_uniform=800)
        nbad, d, _, _ = _check_sdf_at(ctx, o, coeffs, T, tt[rng.permutation(len(tt))], rng, 0, (N, "fast"))
        print(f"sdf_at N {N:3d} FLAG_FAST_PIECE_TIME generic: mode {int(d[0, 7])}, {nbad} mismatches")
        assert nbad == 0, (N, nbad)
        ctx.close()
        assert any(locate_chain(T, float(t)) != locate_cumulative(T, float(t)) for t in tt), N   # (not vacuous)
    for N in (16, 65, 128):
        T = np.full(N, 2.5)
        T[::3] = 0.75 + 2.0 ** -20
        dflt, o, coeffs = _sdf_at_case(T, rng)
        hs, ts_ = dflt.head_state, dflt.tail_state
        exact = svsdf_amd.SvsdfContext(shape="star", device=0, flags=svsdf_amd.FLAG_EXACT_PIECE_TIME,
                                       head_state=hs, tail_state=ts_)
        tt = probe_times(T, rng, n_uniform=800)
        for layout, ts in _layouts(tt, rng).items():
            xy = np.array([o.pos(t)[:2] for t in ts]) + rng.normal(0, 2.0, (len(ts), 2))
            a = dflt.debug_sdf_at(coeffs, T, xy, ts)
            b = exact.debug_sdf_at(coeffs, T, xy, ts)
            assert np.all(a[:, 7] == 0) and np.all(b[:, 7] == 1), layout
            assert np.array_equal(a[:, :7], b[:, :7]), (N, layout, int((a[:, :7] != b[:, :7]).any(axis=1).sum()))
            for cum in (0, 1):
                o.set_modes(1, cum)
                ref = np.array([o.sdf_at_time(x, y, t) for (x, y), t in zip(xy, ts)])
                assert np.array_equal(b[:, 0], ref), (N, layout, cum, int((b[:, 0] != ref).sum()))
            print(f"sdf_at N {N:3d} coarse: default mode 0 == FLAG_EXACT_PIECE_TIME mode 1 == oracle, {layout}")
        dflt.close()
        exact.close()


# ---- pipeline level ----------------------------------------------------------------------------------------------------
def _kw(w):
    return dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], poly_params=w["poly_params"],
                polygon=w["polygon"], head_state=w["head_state"], tail_state=w["tail_state"])


def _generic(w, seed=11):
    """bench.py's generic_durations: tau of the 2.5 s pieces perturbed by 1e-3 N(0, 1), then forward_T, then MINCO."""
    import svsdf_amd
    rng = np.random.default_rng(seed)
    N = len(w["T"])
    tau = svsdf_amd.backward_T(w["T"]) * (1.0 + 1e-3 * rng.standard_normal(N))
    T = svsdf_amd.forward_T(tau)
    return svsdf_amd.minco_coeffs(w["head_state"], w["tail_state"], w["q"], T), T


class _Oracle:
    """One oracle evaluation of a cloud in device-arithmetic mode, kept for every configuration run against it."""

    def __init__(self, o, pts, nsub=3000, seed=0):
        t0 = time.perf_counter()
        c0 = o.counters()["sdf_evals"]
        self.cost, self.gT, self.gC, self.sdf, self.ts, _ = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
        dt = time.perf_counter() - t0
        self.rate = (o.counters()["sdf_evals"] - c0) / max(dt, 1e-9) / NT
        self.secs = dt
        self.sub = np.arange(len(pts)) if len(pts) <= nsub else \
            np.sort(np.random.default_rng(seed).choice(len(pts), nsub, replace=False))
        self.g = o.query(pts[self.sub], nthreads=NT)[2]


def _evaluate(label, kw, shape, pts, coeffs, T, ref, flags=0, plan=None, ctx=None, evals=2, want_mode=1,
              throughput=True):
    """Evaluates on the device, checks against `ref` (an _Oracle) and prints the case's line; returns the penalties."""
    import svsdf_amd
    own = ctx is None
    if own:
        ctx = svsdf_amd.SvsdfContext(shape=shape, device=0, flags=flags, **kw)
        ctx.set_points(pts)
        if plan:
            ctx.set_plan(**plan)
    pens, recs = [], []
    for _ in range(evals):
        pens.append(ctx.eval_penalty(coeffs, T))
        recs += ctx.last_launches()
    st = ctx.stats()
    sdf, ts, g, _ = ctx.query_points(coeffs, T)
    recs += ctx.last_launches()
    if own:
        ctx.close()
    bad = (sdf != ref.sdf) | (ts != ref.ts)
    bad[ref.sub] |= (g[ref.sub] != ref.g).any(axis=1)
    kinds = sorted({r["kernel"] + ("<%d,%d,%d>" % (r["targ"][0], r["targ"][1], r["points_per_wave"])
                                   if r["kernel"] == "tail" else "") for r in recs})
    N = len(T)
    print(f"{label}: N {N} total {T.sum():.3f} s mode {st['piece_time_exact']} interior {st['interior_points']} "
          f"batches {st['batches']} kernels {' '.join(kinds)}; {int(bad.sum())} per-point mismatches of {len(pts)} "
          f"(oracle {ref.secs:.1f} s, {ref.rate:.3g} SDF evals/s/core)")
    assert st["piece_time_exact"] == want_mode, (label, st["piece_time_exact"])
    assert int(bad.sum()) == 0, (label, int((sdf != ref.sdf).sum()), int((ts != ref.ts).sum()))
    for cost, gT, gC in pens:
        assert abs(cost - ref.cost) <= 1e-12 * abs(ref.cost), (label, cost, ref.cost)
        assert _rel(gT, ref.gT) <= 1e-12 and _rel(gC, ref.gC) <= 1e-12, (label, _rel(gT, ref.gT), _rel(gC, ref.gC))
    if throughput:
        assert any(r["kernel"] == "round" or (r["kernel"] == "tail" and r["targ"][1] == 3) for r in recs), (label, kinds)
    return pens, st


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("config", ["C2", "C3", "NS", "C4", "C5"])
def test_baseline_workloads_under_generic_durations(built, config):
    """The BASELINE workloads with bench.py's generic durations, sized so that more than 12 interior points per CU reach
    the GSIP loop (k_round / k_tail<., ., 3>); C2 also at 100 k points, where three point batches run concurrently."""
    import svsdf_amd
    from svsdf_amd import workload
    n_cu = _n_cu()
    sizes = [20000] + ([100000] if config == "C2" else [])
    for P in sizes:
        w = workload.make(config, P=P, minco=svsdf_amd.minco_coeffs)
        coeffs, T = _generic(w)
        o = orc.Oracle(w["shape"], **_kw(w))
        o.set_traj(coeffs, T)
        o.set_modes(1, 0)
        ref = _Oracle(o, w["points"])
        assert int((ref.sdf <= 0).sum()) > 12 * n_cu, (config, int((ref.sdf <= 0).sum()), n_cu)
        ctx = svsdf_amd.SvsdfContext(shape=w["shape"], device=0, **_kw(w))
        ctx.set_points(w["points"])
        _, st = _evaluate(f"{config} P {P}", _kw(w), w["shape"], w["points"], coeffs, T, ref, ctx=ctx, evals=3)
        if P == 100000:
            assert st["batches"] == 3 and ctx.get_plan()["batches"] == 3, st["batches"]
        ctx.close()


def test_every_plan_gives_the_same_bits_at_32_pieces(built):
    """C3 (32 pieces) with generic durations: bound mode 0 ... 3 x tail start {0, 2, -2}, each the oracle's bits and the
    same cost / gradient bits as every other."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C3", P=20000, minco=svsdf_amd.minco_coeffs)
    coeffs, T = _generic(w, seed=5)
    o = orc.Oracle(w["shape"], **_kw(w))
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    ref = _Oracle(o, w["points"])
    first = None
    for bm in range(4):
        for ti in (0, 2, -2):
            pens, st = _evaluate(f"C3 plan bound {bm} tail {ti}", _kw(w), w["shape"], w["points"], coeffs, T, ref,
                                 plan=dict(bound_mode=bm, tail_iter=ti))
            assert st["gsip_bound_mode"] == bm, (bm, st["gsip_bound_mode"])
            if first is None:
                first = pens[0]
            for cost, gT, gC in pens:
                assert cost == first[0] and np.array_equal(gT, first[1]) and np.array_equal(gC, first[2]), (bm, ti)


@pytest.mark.parametrize("N", [32, 128])
def test_waves_that_mix_pieces(built, N):
    """FLAG_KEEP_INPUT_ORDER with a shuffled cloud: no Morton sort, so every wave of k_solve, k_classify and the assembly
    spans many pieces (the uniform phase of the chain ends early, the per-lane rest does the work)."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C3", P=16000, N=N, minco=svsdf_amd.minco_coeffs)
    w["T"] = np.full(N, 2.5 if N == 32 else 0.9)
    coeffs, T = _generic(w, seed=N)
    pts = w["points"][np.random.default_rng(N).permutation(len(w["points"]))]
    o = orc.Oracle(w["shape"], **_kw(w))
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    ref = _Oracle(o, pts)
    _evaluate(f"C3 N {N} shuffled, input order kept", _kw(w), w["shape"], pts, coeffs, T, ref,
              flags=svsdf_amd.FLAG_KEEP_INPUT_ORDER, throughput=False)


def test_return_to_start_trajectory(built):
    """32 generic pieces that end where they start (the fuzz's kind 1): many plateau points and interior points whose t*
    sits near either end -- where k_classify's low-speed rescans run."""
    import svsdf_amd
    rng = np.random.default_rng(4242)
    N = 32
    hs, ts, q = _path(N, rng, back=True)
    T = rng.uniform(0.3, 4.0, N)
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    anchors = np.vstack([hs[:2, 0][None, :], q[:, :2]])
    P = 12000
    pts = np.zeros((P, 3))
    pts[:, :2] = anchors[rng.integers(0, len(anchors), P)] + rng.normal(0, 2.5, (P, 2))
    pts[: P // 10, :2] = hs[:2, 0] + rng.normal(0, 0.8, (P // 10, 2))      # around the common start / end
    kw = dict(safety_hor=0.9, weight_p=60.0, rho=3.8, head_state=hs, tail_state=ts)
    o = orc.Oracle("sdHorseshoe", **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    ref = _Oracle(o, pts)
    _evaluate("return to start, sdHorseshoe", kw, "sdHorseshoe", pts, coeffs, T, ref, throughput=False)


def test_mode_two_end_to_end(built):
    """One piece of 5e-7 s among 16 generic ones: every piece time with every comparison (piece_time_exact == 2)."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C2", P=12000, minco=svsdf_amd.minco_coeffs)
    coeffs, T = _generic(w, seed=2)
    T[7] = 5e-7
    coeffs = svsdf_amd.minco_coeffs(w["head_state"], w["tail_state"], w["q"], T)
    o = orc.Oracle(w["shape"], **_kw(w))
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    ref = _Oracle(o, w["points"])
    _evaluate("C2 with a 5e-7 s piece", _kw(w), w["shape"], w["points"], coeffs, T, ref, want_mode=2, throughput=False)


def test_stale_duration_at_128_pieces(built):
    """128 pieces of ~2.5 s (~320 s, past the 300 s update rule of SWM:376-385): on a fresh context (the first call sets
    the duration) and on one that has just evaluated a shorter trajectory (the duration stays stale, the scan table and
    the search keep the short one's span); the oracle is driven through the same set_traj sequence."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C3", P=8000, N=128, minco=svsdf_amd.minco_coeffs)
    coeffs, T = _generic(w, seed=128)
    assert 300.0 < T.sum() < 340.0, T.sum()
    ws = workload.make("C3", P=8, N=64, minco=svsdf_amd.minco_coeffs)
    cs, Ts = _generic(ws, seed=64)
    kw = _kw(w)
    for label, prior in (("fresh", None), ("stale", (cs, Ts))):
        o = orc.Oracle(w["shape"], **kw)
        o.set_modes(1, 0)
        ctx = svsdf_amd.SvsdfContext(shape=w["shape"], device=0, **kw)
        ctx.set_points(w["points"])
        if prior is not None:
            o.set_traj(*prior)
            ctx.eval_penalty(*prior)
        o.set_traj(coeffs, T)
        want = partial_sums(T if prior is None else Ts)[-1]
        assert o.duration() == want, (label, o.duration(), want)
        ref = _Oracle(o, w["points"])
        _evaluate(f"C3 128 pieces {label} duration {o.duration():.1f} s", kw, w["shape"], w["points"], coeffs, T, ref,
                  ctx=ctx, throughput=False)
        ctx.close()
