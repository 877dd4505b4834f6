"""svsdf_motion_bounds (the Bernstein bounds the certified clearance search rests on) against the analytic velocity
polynomials, and the argument checks of svsdf_min_clearance that need no device."""
import ctypes as C

import numpy as np
import pytest


def _traj(rng, N):
    """The recipe of test_gpu_sdf_at.py: generic durations, waypoints scattered around a straight line."""
    import svsdf_amd
    T = rng.uniform(0.4, 3.0, N)
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3))
    hs[:2, 0] = rng.uniform(0, 10, 2); ts[:2, 0] = hs[:2, 0] + rng.uniform(-10, 10, 2)
    hs[2, 0] = rng.uniform(-3, 3); ts[2, 0] = rng.uniform(-3, 3)
    q = np.column_stack([np.linspace(hs[0, 0], ts[0, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         np.linspace(hs[1, 0], ts[1, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         rng.uniform(-2.5, 2.5, N - 1)])
    return svsdf_amd.minco_coeffs(hs, ts, q, T), T


def _derivs(coeffs, T, t, order=1):
    """d^order/dt^order of (x, y, yaw) at the times t: the piece polynomials differentiated term by term.  (len(t), 3)."""
    S = np.concatenate([[0.0], np.cumsum(T)])
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    i = np.clip(np.searchsorted(S, t, side="right") - 1, 0, len(T) - 1)
    s = t - S[i]
    out = np.zeros((len(t), 3))
    for k in range(order, 6):
        f = np.prod(np.arange(k, k - order, -1.0))
        out += f * coeffs[6 * i + k] * (s ** (k - order))[:, None]
    return out


def _sampled_max(coeffs, T, ta, tb, n=2000):
    tt = np.linspace(max(ta, 0.0), min(tb, T.sum()), n)
    v = _derivs(coeffs, T, tt)
    # a sample on a piece boundary belongs to both pieces (their velocities agree to rounding there)
    return np.hypot(v[:, 0], v[:, 1]).max(), np.abs(v[:, 2]).max()


def test_motion_bounds_dominate_the_sampled_velocities(built):
    import svsdf_amd
    for seed in range(20):
        rng = np.random.default_rng(7000 + seed)
        N = int(rng.integers(3, 9))
        coeffs, T = _traj(rng, N)
        td = T.sum()
        S = np.concatenate([[0.0], np.cumsum(T)])
        spans = [(0.0, td), (0.3 * td, 0.3 * td), (0.0, 0.0), (td, td), (S[1] - 0.05, S[2] + 0.05), (S[1], S[1])]
        for _ in range(10):
            a, b = np.sort(rng.uniform(0.0, td, 2))
            spans.append((a, b))
            c = rng.uniform(0.0, td)
            spans.append((c, min(c + 0.15, td)))
        for ta, tb in spans:
            V, W = svsdf_amd.motion_bounds(coeffs, T, ta, tb)
            sv, sw = _sampled_max(coeffs, T, ta, tb)
            assert V >= sv and W >= sw, (seed, ta, tb, V, sv, W, sw)
        # an interval reaching outside [0, sum T] is clipped to it
        assert svsdf_amd.motion_bounds(coeffs, T, -1.0, td + 1.0) == svsdf_amd.motion_bounds(coeffs, T, 0.0, td)


def test_motion_bounds_converge_to_the_sampled_value(built):
    """Interval width 0.15 -> 0.15 / 64 around a fixed time: the bound closes on the maximum over the interval to 1e-6
    relative.  The Bernstein gap of a degree-n polynomial p on an interval of width w is at most (n - 1) / (8 n) w^2
    max |p''|; the time is the first of a fixed list at which that figure, from the analytic derivatives, is below 5e-7 of
    the value for both the squared planar speed (n = 8) and the yaw rate (n = 4) -- where the property is attainable at
    this width.  The trajectory is the benchmark's C1 recipe."""
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make("C1", P=10, minco=svsdf_amd.minco_coeffs)
    coeffs, T = w["coeffs"], w["T"]
    td = T.sum()
    wmin = 0.15 / 64
    t0 = None
    for c in td * (0.3 + 0.0137 * np.arange(40)):
        v, a, j, s = (_derivs(coeffs, T, c, o)[0] for o in (1, 2, 3, 4))
        v2 = v[0] ** 2 + v[1] ** 2
        v2dd = 2.0 * (a[0] ** 2 + a[1] ** 2 + v[0] * j[0] + v[1] * j[1])
        if v2 > 0.25 and abs(v[2]) > 0.05 and 7.0 / 64 * wmin ** 2 * abs(v2dd) / (2.0 * v2) < 5e-7 \
                and 3.0 / 32 * wmin ** 2 * abs(j[2]) / abs(v[2]) < 5e-7:
            t0 = c
            break
    assert t0 is not None
    gaps = []
    for k in range(7):
        h = 0.5 * 0.15 / 2 ** k
        V, W = svsdf_amd.motion_bounds(coeffs, T, t0 - h, t0 + h)
        sv, sw = _sampled_max(coeffs, T, t0 - h, t0 + h)
        assert V >= sv and W >= sw
        gaps.append((V / sv - 1.0, W / sw - 1.0))
    print(t0, gaps)
    assert gaps[-1][0] <= 1e-6 and gaps[-1][1] <= 1e-6, gaps


def test_motion_bounds_refuses_bad_arguments(built):
    import svsdf_amd
    L = svsdf_amd.lib()
    dp = C.POINTER(C.c_double)
    coeffs, T = _traj(np.random.default_rng(1), 4)
    cm = np.asfortranarray(coeffs).ravel(order="F").copy()
    out = np.zeros(2)
    p = lambda a: a.ctypes.data_as(dp)
    assert L.svsdf_motion_bounds(4, p(cm), p(T), 0.0, 1.0, p(out)) == 0
    assert L.svsdf_motion_bounds(0, p(cm), p(T), 0.0, 1.0, p(out)) == 1            # SVSDF_ERR_INVALID
    assert L.svsdf_motion_bounds(129, p(cm), p(T), 0.0, 1.0, p(out)) == 1
    assert L.svsdf_motion_bounds(4, p(cm), p(T), 1.0, 0.5, p(out)) == 1            # tb < ta
    assert L.svsdf_motion_bounds(4, p(cm), p(T), float("nan"), 0.5, p(out)) == 1
    bad = cm.copy(); bad[7] = np.inf
    assert L.svsdf_motion_bounds(4, p(bad), p(T), 0.0, 1.0, p(out)) == 4           # SVSDF_ERR_NONFINITE
    Tb = T.copy(); Tb[2] = np.nan
    assert L.svsdf_motion_bounds(4, p(cm), p(Tb), 0.0, 1.0, p(out)) == 4


def test_min_clearance_argument_checks_on_a_host_only_context(built):
    import svsdf_amd
    coeffs, T = _traj(np.random.default_rng(2), 4)
    ctx = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(2\)"):               # SVSDF_ERR_NO_DEVICE
        ctx.min_clearance(coeffs, T)
    for kw in (dict(struct_size=8), dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("nan")), dict(eps=float("inf"))):
        with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\)"):           # SVSDF_ERR_INVALID
            ctx.min_clearance(coeffs, T, **kw)
    prm = svsdf_amd.binding.ClearanceParams()
    svsdf_amd.lib().svsdf_clearance_params_default(C.byref(prm))
    assert prm.struct_size == C.sizeof(svsdf_amd.binding.ClearanceParams) == 40
    assert prm.eps == 1e-3 and prm.target != prm.target and prm.max_evals == 0 and prm.pair_capacity == 0
    assert C.sizeof(svsdf_amd.binding.ClearanceResult) == 96
    ctx.close()
