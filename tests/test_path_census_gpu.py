"""The census cases (tests/golden/golden_census.json, tests/test_path_census.py) on the device.

Per case, the cloud of 24 points as it is, repeated 11 times and repeated 43 times: P = 24 takes the one-block reduce, the
solo solve and the wave-per-point tail; P = 264 lies in (256, 1024] (the fused reduce over several blocks); P = 1032 lies
above 1024 (k_final / k_finish, batched rounds).  Each run is held
  * to the C oracle in device-arithmetic mode (orc set_modes(1, 0), as test_kernel_instantiations_gpu.py): per-point sdf,
    t* and gradient bit for bit, cost and gradients to 1e-12;
  * to the fixture, whose restatement uses libm, by the project's own gates with no excused point (make_census.py kept only
    points on which the oracle's two trig modes stay within half of them): lmbm_evaluate cost 1e-7 and gradient 1e-5
    relative, query_points sdf 1e-8 and t* 1e-6;
  * to the single-copy run: every copy of a point carries its bits, the cost is r times the single cost to 1e-12.
Counters: svsdf_stats.interior_points and .gsip_samples (ring samples emitted; the reference solves every one) equal the
census.  .gsip_iterations is left out: it counts the iterations of the launch chain that had solve work, rounds AND the
supplementary iterations that solve samples a bound could not exclude (include/svsdf_c.h), which is not the census's number
of GSIP rounds.  The scaled cases run under svsdf_set_scale with the fixture's schedule.
"""
import numpy as np
import pytest

import path_census as pc

pytestmark = pytest.mark.gpu
DOC = pc.load_fixture()
CASES = DOC["cases"]
IDS = [c["id"] for c in CASES]
REPEATS = (1, 11, 43)


def _rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _form(recs):
    red = [r for r in recs if r["kernel"] in ("reduce", "reduce_scaled")]
    assert len(red) >= 1, recs
    kinds = {r["kernel"] for r in recs}
    if red[-1]["fused"]:
        assert not ({"final", "finish"} & kinds)
        return "one block" if red[-1]["grid"] == 1 else "fused"
    assert {"final", "finish"} <= kinds
    return "final"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_census_case_on_the_device(built, case):
    import svsdf_amd
    o, tj = pc.oracle_of(DOC, case)
    coeffs, T, x = np.array(tj["coeffs"]), np.array(tj["T"]), np.array(tj["x"])
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)                     # the device library's sin / cos / atan2; the reference's piece location
    ctx = svsdf_amd.SvsdfContext(shape=case["shape"], safety_hor=case["safety_hor"], weight_p=case["weight_p"],
                                 rho=case["rho"], poly_params=case["poly_params"],
                                 polygon=None if case["polygon"] is None else np.array(case["polygon"]),
                                 head_state=np.array(tj["head"]).T, tail_state=np.array(tj["tail"]).T, device=0)
    if case["scale"]:
        ctx.set_scale(**case["scale"])
    per = np.array(case["per_point"])
    recs_census = [pc.decode(r) for r in case["rec"]]
    interior = sum(r["interior"] for r in recs_census)
    ring = sum(r["ring"] for r in recs_census)
    n = len(case["points"])
    pts1 = pc.cloud(case)
    ocost, ogT, ogC = o.penalty(pts1)
    osdf, ots, og = o.query(pts1)
    forms, single = set(), None
    for r in REPEATS:
        what = (case["id"], r)
        pts = pc.cloud(case, r)
        ctx.set_points(pts)
        cost, gT, gC = ctx.eval_penalty(coeffs, T)
        forms.add(_form(ctx.last_launches()))
        st = ctx.stats()
        sdf, ts, g, _ = ctx.query_points(coeffs, T)
        sdf, ts, g = np.array(sdf), np.array(ts), np.array(g)
        # every copy: the bits of the oracle in device arithmetic (and so of the single-copy run)
        for k in range(r):
            s = slice(k * n, (k + 1) * n)
            assert np.array_equal(sdf[s], osdf), (what, k, np.abs(sdf[s] - osdf).max())
            assert np.array_equal(ts[s], ots), (what, k, np.abs(ts[s] - ots).max())
            assert np.array_equal(g[s], og), (what, k, np.abs(g[s] - og).max())
        if single is None:
            single = (cost, sdf.copy(), ts.copy(), g.copy())
            assert abs(cost - ocost) <= 1e-12 * abs(ocost), (what, cost, ocost)
            assert _rel(gT, ogT) <= 1e-12 and _rel(gC, ogC) <= 1e-12, (what, _rel(gT, ogT), _rel(gC, ogC))
        assert np.array_equal(sdf, np.tile(single[1], r)) and np.array_equal(ts, np.tile(single[2], r)) \
            and np.array_equal(g, np.tile(single[3], (r, 1))), what
        assert abs(cost - r * single[0]) <= 1e-12 * abs(r * single[0]), (what, cost, single[0])
        assert abs(cost - r * ocost) <= 1e-12 * abs(r * ocost), (what, cost, ocost)
        assert _rel(gT, r * ogT) <= 1e-12 and _rel(gC, r * ogC) <= 1e-12, (what, _rel(gT, r * ogT), _rel(gC, r * ogC))
        # the fixture (libm): the project's gates, no excused point
        np.testing.assert_allclose(sdf, np.tile(per[:, 0], r), rtol=0, atol=1e-8, err_msg=str(what))
        np.testing.assert_allclose(ts, np.tile(per[:, 1], r), rtol=0, atol=1e-6, err_msg=str(what))
        if r == 1:
            f, gx = ctx.lmbm_evaluate(x)
            assert abs(f - case["cost"]) <= 1e-7 * abs(case["cost"]), (what, f, case["cost"])
            assert np.linalg.norm(gx - np.array(case["grad"])) <= 1e-5 * np.linalg.norm(case["grad"]), what
        assert st["points"] == r * n and st["interior_points"] == r * interior and st["gsip_samples"] == r * ring, \
            (what, st["points"], st["interior_points"], st["gsip_samples"], interior, ring)
    ctx.close()
    assert forms == {"one block", "fused", "final"}, (case["id"], forms)
