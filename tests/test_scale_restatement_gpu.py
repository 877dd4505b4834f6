"""The scaled path against an independent restatement of the reference's useScale arithmetic.

The restatement is tests/golden/make_golden.py's pure-Python reference path (libm trig, no FMA, written from the reference
sources) with S(t) put where the reference's `useScale = true` puts it -- and nowhere else:
  * choiceTInit stays rigid (SWM:567-570 call the non-scale overloads);
  * gradientDescent evaluates getSDFAtTimeStamp<true> and getSDF_DOTAtTimeStamp<true>: u = (Rt^T S(t)^-1)(p - x(t)),
    S^-1 as Eigen's 3x3 inverse() forms it (cofactors times 1 / det), Rt^T S^-1 formed first (SWM:528-535, 799-806);
  * the exterior gradient is getonlyGrad1 at the scaled u at t* (SWM:779-797);
  * grad_cost_p_sw takes -(S(t*)^-1)^T R g for the position gradient, the rigid yaw term (BEO:1050, 1062).
The library must match it under the reference's example schedule on star, sdHorseshoe, sdHeart and the star.obj Polygon
outline, with interior (GSIP) points in every cloud: per point (basin flips <= 0.2 %, sdf of the others <= 1e-7) through
svsdf_query_points, and the full callback (cost <= 1e-7, gradient <= 1e-5 relative) through svsdf_lmbm_evaluate.  A
constant schedule pins the S^-1 form on the device bit for bit (the cofactor form, not 1 / s).

The restatement itself lives in tests/scale_restatement.py (shared with tests/test_oracle_scale.py, which holds the C oracle
to it on the CPU).
"""
import numpy as np
import pytest

from scale_restatement import CASES, EXAMPLE, HEAD, Q, T, TAIL, _points, _x, mg, restated_cost_function

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", list(CASES))
def test_example_schedule_matches_the_restatement(built, shape):
    import svsdf_amd
    from svsdf_amd import workload
    safety_hor, n = CASES[shape]
    verts = [tuple(map(float, v)) for v in workload.mesh_outline("star")] if shape == "Polygon" else None
    pts = _points(shape, n, 40 + len(shape))
    x = _x()
    f_ref, g_ref, _, rows, Tv, per, _, main_f = restated_cost_function(shape, verts, pts, safety_hor, EXAMPLE, x)
    per = np.array(per)
    assert (np.array(main_f) <= 0).sum() >= 5, "the cloud needs interior points (GSIP)"
    hs, ts = np.array(HEAD).T, np.array(TAIL).T
    ctx = svsdf_amd.SvsdfContext(shape=shape, safety_hor=safety_hor, weight_p=60.0, rho=3.8,
                                 polygon=np.array(verts) if verts else None, head_state=hs, tail_state=ts, device=0)
    xyz = np.array([[p[0], p[1], 0.0] for p in pts])
    ctx.set_points(xyz)
    ctx.set_scale(**EXAMPLE)
    # per point, on the restatement's own trajectory coefficients
    sdf, tst, grad, _ = ctx.query_points(np.array(rows), Tv)
    assert {"solve_scaled", "classify_scaled"} <= {r["kernel"] for r in ctx.last_launches()}
    flip = np.abs(tst - per[:, 1]) > 1e-4
    assert flip.sum() <= int(0.002 * len(pts)), (shape, np.flatnonzero(flip), tst[flip], per[flip, 1], sdf[flip], per[flip, 0])
    ok = ~flip
    assert np.max(np.abs(sdf[ok] - per[ok, 0])) <= 1e-7, shape
    np.testing.assert_allclose(grad[ok], per[ok, 2:4], rtol=0, atol=1e-5)
    # the full callback
    f, g = ctx.lmbm_evaluate(np.array(x))
    assert abs(f - f_ref) <= 1e-7 * abs(f_ref), (shape, f, f_ref)
    g_ref = np.array(g_ref)
    assert np.linalg.norm(g - g_ref) <= 1e-5 * np.linalg.norm(g_ref), (shape, np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref))
    # and the schedule acts: the rigid callback is another number
    ctx.set_scale(None)
    f0, _ = ctx.lmbm_evaluate(np.array(x))
    assert abs(f0 - f_ref) > 1e-6 * abs(f_ref)
    ctx.close()


def test_inverse_form_is_pinned_on_the_device(built):
    """A constant schedule (A = 0, so no sin enters): the device's body-frame point equals u with Eigen's cofactor inverse
    bit for bit, and for these scales that differs from u with 1 / s_x, 1 / s_y at some points."""
    import svsdf_amd
    rows, _, _ = mg.minco(HEAD, TAIL, Q, T)
    ctx = svsdf_amd.SvsdfContext(shape="star", safety_hor=0.7, head_state=np.array(HEAD).T, tail_state=np.array(TAIL).T, device=0)
    rng = np.random.default_rng(5)
    n = 512
    pxy = np.column_stack([rng.uniform(0, 16, n), rng.uniform(-2, 12, n)])
    tt = rng.uniform(0, sum(T), n)
    differs = 0
    for sx, sy in ((0.7, 1.3), (1.9, 0.45), (0.33, 0.83)):
        ctx.set_scale(c=(sx, sy))
        out = ctx.debug_sdf_at(np.array(rows), T, pxy, tt)
        inv = 1.0 / (sy * sx)
        i00, i11 = sy * inv, sx * inv
        cs, sn, x, y = out[:, 3], out[:, 4], out[:, 1], out[:, 2]
        dx, dy = pxy[:, 0] - x, pxy[:, 1] - y
        ux = (cs * i00) * dx + (sn * i11) * dy
        uy = ((-sn) * i00) * dx + (cs * i11) * dy
        assert np.array_equal(out[:, 5].view(np.int64), ux.view(np.int64)) and np.array_equal(out[:, 6].view(np.int64), uy.view(np.int64))
        wx = (cs * (1.0 / sx)) * dx + (sn * (1.0 / sy)) * dy
        wy = ((-sn) * (1.0 / sx)) * dx + (cs * (1.0 / sy)) * dy
        differs += int(np.sum((wx != ux) | (wy != uy)))
    assert differs > 0, "the scales chosen do not tell the two forms apart"
    ctx.close()
