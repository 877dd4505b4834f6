"""The trajectory intake of the device entry points (csrc/svsdf_traj_host.hpp, upload_traj): a probe upload
(svsdf_min_clearance) leaves the persistent duration, the statistics and the launch record to the evaluations, and a faulty
trajectory gets the same error code from every entry, whether the stripe it reaches holds points or not.  Star, 200 points,
five pieces: every path here is host logic around one k_prep."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# SVSDF_ERR_INVALID, SVSDF_ERR_NONFINITE
INVALID, NONFINITE = 1, 4


@functools.lru_cache(maxsize=None)
def _case():
    """Head and tail state, waypoints and a 200-point cloud around them (the recipe of test_clearance_gpu.py)."""
    rng = np.random.default_rng(77)
    N, P = 5, 200
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3))
    hs[:2, 0] = rng.uniform(0, 10, 2); ts[:2, 0] = hs[:2, 0] + rng.uniform(-10, 10, 2)
    hs[2, 0] = rng.uniform(-3, 3); ts[2, 0] = rng.uniform(-3, 3)
    q = np.column_stack([np.linspace(hs[0, 0], ts[0, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         np.linspace(hs[1, 0], ts[1, 0], N + 1)[1:-1] + rng.uniform(-2, 2, N - 1),
                         rng.uniform(-2.5, 2.5, N - 1)])
    way = np.vstack([hs[:2, 0], q[:, :2], ts[:2, 0]])
    pts = np.column_stack([way[rng.integers(0, len(way), P)] + rng.normal(0.0, 3.0, (P, 2)), np.zeros(P)])
    return hs, ts, q, pts


def _ctx(pts, **kw):
    import svsdf_amd
    hs, ts, _, _ = _case()
    c = svsdf_amd.SvsdfContext(shape="star", head_state=hs, tail_state=ts, **{**dict(device=0), **kw})
    if pts is not None:
        c.set_points(pts)
    return c


def _coeffs(T):
    import svsdf_amd
    hs, ts, q, _ = _case()
    return svsdf_amd.minco_coeffs(hs, ts, q, T)


def _counted(stats):
    """The statistics without what differs between two runs of the same evaluation: the measured times and clocks, and
    speculative_evals with the sdf_evals that include them (ladder candidates evaluated behind the accepted one: how many
    depends on which descents share a wave's step, i.e. on scheduling; two fresh contexts differ in them on their first
    evaluation)."""
    return {k: v for k, v in stats.items() if "_ms" not in k and k not in ("shader_clock_mhz", "speculative_evals", "sdf_evals")}


def _same_result(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_probe_leaves_the_stale_duration_alone(built):
    """Context A: an evaluation (12.5 s), a clearance search on another trajectory (13.75 s), an evaluation of 5 x 60 s --
    300 s, the reference's stale regime, where the first evaluation's 12.5 s stay in force.  Context B: the two
    evaluations alone.  Had the search stored its 13.75 s, A's last evaluation would scan another table."""
    pts = _case()[3]
    T1, T2, T3 = np.full(5, 2.5), np.full(5, 2.5) * 1.1, np.full(5, 60.0)
    c1, c2, c3 = _coeffs(T1), _coeffs(T2) * 1.01, _coeffs(T3)
    A, B = _ctx(pts), _ctx(pts)
    a1, b1 = A.eval_penalty(c1, T1), B.eval_penalty(c1, T1)
    sa, la = A.stats(), A.last_launches()
    assert _same_result(a1, b1) and _counted(sa) == _counted(B.stats()) and la == B.last_launches()
    assert sa["points"] == 200 and len(la) > 3 and la[0]["kernel"] == "prep"
    r = A.min_clearance(c2, T2)
    assert r["lower"] <= r["upper"] and r["evals"] > 0
    assert A.stats() == sa and A.last_launches() == la            # the search notes nothing for the evaluations
    a3, b3 = A.eval_penalty(c3, T3), B.eval_penalty(c3, T3)
    assert _same_result(a3, b3) and _counted(A.stats()) == _counted(B.stats()) and A.last_launches() == B.last_launches()
    assert A.last_launches()[0]["work"] == la[0]["work"] == 84    # k_prep's table: 12.5 s / 0.15 s, not 13.75 s (92) nor 300 s
    A.close(); B.close()


def _faults():
    """(name, N, coeffs, T, code): every single fault check_traj knows, as in tests/cpp/traj_host.cpp."""
    out = []
    for N in (0, 129):
        out.append((f"N = {N}", np.full((6 * N, 3), 0.25), np.full(N, 1.5), INVALID))
    T5 = np.full(5, 2.5)
    c5 = _coeffs(T5)
    for name, v, code in (("T = 0", 0.0, INVALID), ("T < 0", -1.0, INVALID), ("T NaN", np.nan, NONFINITE), ("T +inf", np.inf, NONFINITE)):
        T = T5.copy(); T[1] = v
        out.append((name, c5, T, code))
    for name, v in (("coefficient NaN", np.nan), ("coefficient inf", np.inf)):
        c = c5.copy(); c[7, 1] = v
        out.append((name, c, T5, NONFINITE))
    return out


def _code(call, *args):
    import svsdf_amd
    with pytest.raises(svsdf_amd.SvsdfError) as e:
        call(*args)
    msg = str(e.value)
    return int(msg[msg.index("failed (") + 8:].split(")")[0])


def test_error_code_does_not_depend_on_empty_stripes(built):
    pts = _case()[3]
    full, empty, group = _ctx(pts), _ctx(np.zeros((0, 3))), _ctx(pts[:1], devices=[0, 0])
    assert group.group_stripe(0)["points"] == 1 and group.group_stripe(1)["points"] == 0
    T5 = np.full(5, 2.5)
    c5 = _coeffs(T5)
    # two faults at once: a non-positive duration and an infinite one -- the total is tested first, everywhere
    c2, T2 = np.full((12, 3), 0.25), np.array([-1.0, np.inf])
    for ctx in (full, empty, group):
        assert _code(ctx.eval_penalty, c2, T2) == NONFINITE
        assert _code(ctx.min_clearance, c2, T2) == NONFINITE
    # ... and a non-positive duration with a NaN coefficient: the durations are tested before the coefficients
    bad = c5.copy(); bad[7, 1] = np.nan
    Tb = T5.copy(); Tb[3] = -1.0
    for ctx in (full, empty, group):
        assert _code(ctx.eval_penalty, bad, Tb) == INVALID
        assert _code(ctx.min_clearance, bad, Tb) == INVALID
    for name, c, T, code in _faults():
        for ctx in (full, empty, group):
            assert _code(ctx.eval_penalty, c, T) == code, name
            assert _code(ctx.min_clearance, c, T) == code, name
    for ctx in (full, empty, group):                              # and the contexts still work
        assert np.isfinite(ctx.eval_penalty(c5, T5)[0])
        ctx.close()
