"""tests/golden/golden_census.json: the whole callback on every branch of the reference's solve that a trajectory reaches.

The fixture is made by tests/golden/make_census.py from tests/path_census.py: make_golden's restatement of the reference
path, run unchanged over the second reading of the sixteen analytic shapes, with a branch record per point.  Here:
  * the fixture cannot drift: every case is regenerated from its stored inputs, numbers and records exactly;
  * the C oracle in libm mode reproduces it within test_golden_vectors.py's gates;
  * the oracle's two trig modes stay within half of the project's gates on the census points (the selection rule);
  * the census requirements hold on the committed file, and the branches nobody requires keep their committed counts.
The GPU half is tests/test_path_census_gpu.py.
"""
import numpy as np
import pytest

from oracle import orc
import path_census as pc

DOC = pc.load_fixture()
CASES = DOC["cases"]
IDS = [c["id"] for c in CASES]


@pytest.fixture(scope="module")
def pool():
    with pc.executor() as ex:
        yield ex


@pytest.mark.parametrize("third", range(3))
def test_fixture_regenerates_exactly(pool, third):
    """a fixed third of the cases per test function: stored inputs -> path_census -> the stored numbers and records"""
    for case in CASES[third::3]:
        tj = DOC["trajectories"][case["traj"]]
        rows, durs = pc.coefficients(tj["head"], tj["tail"], tj["x"])
        assert durs == tj["T"] and [list(r) for r in rows] == tj["coeffs"], case["id"]
        res = pc.evaluate(pool, case, tj["head"], tj["tail"], tj["x"])
        assert res["rec"] == case["rec"], case["id"]
        for key in ("per_point", "n_solves", "cost", "costs3", "grad"):
            assert res[key] == case[key], (case["id"], key)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_reproduces_the_census(case):
    """test_golden_vectors.py's gates, libm mode"""
    o, tj = pc.oracle_of(DOC, case)
    pts = pc.cloud(case)
    f, g, c3 = o.cost_function(pts, np.array(tj["x"]))
    assert abs(f - case["cost"]) <= 1e-12 * abs(case["cost"])
    np.testing.assert_allclose(c3, case["costs3"], rtol=1e-12)
    np.testing.assert_allclose(g, case["grad"], rtol=1e-10, atol=1e-10)
    coeffs = np.array(tj["coeffs"])
    N = len(tj["T"])
    np.testing.assert_allclose(orc.minco_coeffs(np.array(tj["head"]).T, np.array(tj["tail"]).T,
                                                np.array(tj["x"][N:]).reshape(-1, 3), tj["T"]), coeffs, rtol=0, atol=1e-13)
    np.testing.assert_allclose(orc.forward_T(tj["x"][:N]), tj["T"], rtol=0, atol=1e-15)
    o.set_traj(coeffs, tj["T"])
    sdf, tstar, grad = o.query(pts)
    cnt = o.counters()
    per = np.array(case["per_point"])
    np.testing.assert_allclose(sdf, per[:, 0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(tstar, per[:, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(grad, per[:, 2:4], rtol=0, atol=1e-9)
    assert cnt["solves"] == case["n_solves"]
    assert cnt["interior_points"] == sum(pc.decode(r)["interior"] for r in case["rec"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_trig_modes_within_half_the_gates(case):
    """the selection rule of make_census.py, re-checked: libm against the device library's algorithms, both on the CPU"""
    o, tj = pc.oracle_of(DOC, case)
    o.set_traj(np.array(tj["coeffs"]), tj["T"])
    pts = pc.cloud(case)
    o.set_modes(0, 0)
    s0, t0, _ = o.query(pts)
    o.set_modes(1, 0)
    s1, t1, _ = o.query(pts)
    assert np.abs(s1 - s0).max() <= 5e-9 and np.abs(t1 - t0).max() <= 5e-7
    assert DOC["dropped"] < 0.02 * DOC["pool"]


def test_census_requirements():
    tab = pc.check_requirements(DOC)
    assert len(CASES) == 17 * 3 + 4 * 2 and all(len(c["points"]) == 24 for c in CASES)
    assert {c["weight_p"] for c in CASES} == {60.0, 7.5} and {c["rho"] for c in CASES} == {3.8, 0.5}
    assert min(c["safety_hor"] for c in CASES) == 0.5 and max(c["safety_hor"] for c in CASES) == 0.9
    # the branches nobody requires: a count that moves is a finding (see make_census.py's docstring)
    assert {b: sum(tab[b].values()) for b in pc.NEVER_REQUIRED} == DOC["never_required"]
    for b in ("gd_exit_trials", "gd_exit_tol", "t_tmin", "t_tmax", "z0"):      # believed unreachable
        assert DOC["never_required"][b] == 0, b
    for b in pc.PER_CASE + pc.PER_SHAPE + pc.IN_THREE_SHAPES:
        print("%-18s" % b, " ".join("%s=%d" % (s, n) for s, n in sorted(tab[b].items())))
