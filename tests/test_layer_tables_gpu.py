"""Pose tables of scan layers 2 and 3 (k_layer_tables): a solve that reads the poses of those two
layers from the tables returns the bits of one that computes them.

Forced on (plan field layer_tables = 3, and 2 = layer 2 alone) against forced off (0), per point (SVSDF, t*, gradient) and
for cost / gradT / gradC, all with numpy.array_equal: the BASELINE workloads at reduced sizes under coarse and generic
piece durations, 1 / 65 / 128 pieces, points at both trajectory ends (windows clamped at 0 and at the duration), a scale
schedule, every lane-group width of the solve kernel; and the tables-on run against the oracle in device-arithmetic mode,
bit for bit per point, the way test_gpu_parity.py compares.  Which path ran is read from the launch record.  tests/
test_layer_table_times.py pins the keying of the tables on the CPU."""
import os

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)


def _case(config, P, N=None, generic=False, seed=1):
    import svsdf_amd
    from svsdf_amd import workload
    w = workload.make(config, P=P, N=(2 if N == 1 else N), minco=svsdf_amd.minco_coeffs)
    if N == 1:   # (the workload's corridor points need a waypoint: its two-piece cloud around a one-piece trajectory)
        w["q"], w["T"] = w["q"][:0], np.array([float(np.sum(w["T"]))])
        w["coeffs"] = svsdf_amd.minco_coeffs(w["head_state"], w["tail_state"], w["q"], w["T"])
    if generic:
        rng = np.random.default_rng(seed)
        n = len(w["T"])
        w["T"] = rng.uniform(1.5, 3.5, n) if n <= 32 else rng.uniform(0.4, 1.2, n)
        w["coeffs"] = svsdf_amd.minco_coeffs(w["head_state"], w["tail_state"], w["q"], w["T"])
    return w


def _ctx(w):
    import svsdf_amd
    ctx = svsdf_amd.SvsdfContext(shape=w["shape"], safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"],
                                 poly_params=w["poly_params"], polygon=w["polygon"], head_state=w["head_state"],
                                 tail_state=w["tail_state"], device=0)
    ctx.set_points(w["points"])
    return ctx


def _run(ctx, w, tables, lanes=-1):
    """per-point results and sums with the plan's layer_tables pinned; the kinds of kernels both evaluations launched"""
    ctx.set_plan(layer_tables=tables, lanes_per_query=lanes)
    assert ctx.get_plan()["layer_tables"] == tables
    q = ctx.query_points(w["coeffs"], w["T"])
    recs = ctx.last_launches()
    cost, gT, gC = ctx.eval_penalty(w["coeffs"], w["T"])
    recs += ctx.last_launches()
    built = [r["targ"][0] for r in recs if r["kernel"] == "layer_tables"]
    return {"q": [np.array(a, dtype=np.float64) for a in q[:3]], "cost": float(cost), "gT": np.array(gT), "gC": np.array(gC),
            "built": built, "widths": sorted({r["targ"][0] for r in recs if r["kernel"] in ("solve", "solve_scaled")})}


def _same(a, b, what):
    for i, name in enumerate(("sdf", "t*", "gradient")):
        assert np.array_equal(a["q"][i], b["q"][i]), (what, name, int((a["q"][i] != b["q"][i]).sum()))
    assert a["cost"] == b["cost"], (what, a["cost"], b["cost"])
    assert np.array_equal(a["gT"], b["gT"]) and np.array_equal(a["gC"], b["gC"]), what


def _on_off(w, what, lanes=-1, scale=None, polygon=False):
    ctx = _ctx(w)
    if scale is not None:
        ctx.set_scale(**scale)
    off = _run(ctx, w, 0, lanes)
    assert off["built"] == [], what
    outs = {0: off}
    for tables in (3, 2):
        on = _run(ctx, w, tables, lanes)
        # one table launch per evaluation; the Polygon kernels compute every layer themselves, so nothing is built for them
        assert on["built"] == ([] if polygon else [tables, tables]), (what, on["built"])
        _same(on, off, (what, tables))
        outs[tables] = on
    print(f"{what}: P={len(w['points'])} pieces={len(w['T'])} widths={off['widths']} cost={off['cost']:.9g} identical on / off")
    ctx.close()
    return outs


@pytest.mark.parametrize("generic", [False, True], ids=["coarse", "generic"])
@pytest.mark.parametrize("config,P,N", [("C1", 20000, None), ("C2", 20000, None), ("C3", 30000, None), ("NS", 30000, None),
                                        ("C5", 3000, 8)])
def test_tables_on_equals_off(built, config, P, N, generic):
    w = _case(config, P, N=N, generic=generic)
    _on_off(w, f"{config} {'generic' if generic else 'coarse'}", polygon=(w["shape"] == "Polygon"))


@pytest.mark.parametrize("N", [1, 65, 128])
def test_piece_counts_generic_durations(built, N):
    w = _case("C3", 6000, N=N, generic=True, seed=N)
    _on_off(w, f"C3 {N} pieces generic")


def test_windows_clamped_at_both_ends(built):
    """Points around the first and the last pose: their layer-1 seeds are the first / last table indices, whose windows
    start at 0 / end at the duration (fewer than 21 samples)."""
    w = _case("C3", 4000, generic=True, seed=7)
    rng = np.random.default_rng(3)
    ends = np.array([w["head_state"][:2, 0], w["tail_state"][:2, 0]])
    pts = np.zeros((4000, 3))
    pts[:, :2] = ends[rng.integers(0, 2, 4000)] + rng.normal(0.0, 0.6, (4000, 2))
    w["points"] = pts
    outs = _on_off(w, "C3 both ends")
    ts, dur = outs[3]["q"][1], float(np.sum(w["T"]))
    assert (ts < 0.15).sum() > 10 and (ts > dur - 0.15).sum() > 10, ((ts < 0.15).sum(), (ts > dur - 0.15).sum())


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32])
def test_every_solve_width(built, lanes):
    w = _case("C3", 5000, generic=(lanes in (2, 16)), seed=lanes)
    outs = _on_off(w, f"C3 width {lanes}", lanes=lanes)
    assert lanes in outs[3]["widths"], outs[3]["widths"]


@pytest.mark.parametrize("generic", [False, True], ids=["coarse", "generic"])
def test_scale_schedule(built, generic):
    """Layers 2 - 4 stay rigid under a schedule (the reference's choiceTInit), so the scaled solve reads the same tables."""
    import svsdf_amd
    w = _case("C3", 5000, generic=generic, seed=11)
    outs = _on_off(w, f"C3 scaled {'generic' if generic else 'coarse'}", scale=svsdf_amd.binding.EXAMPLE_SCALE)
    rigid = _on_off(w, "C3 rigid")
    assert outs[3]["cost"] != rigid[3]["cost"]     # the schedule was in force


@pytest.mark.parametrize("config,P,generic", [("C1", 6000, False), ("C3", 4000, False), ("NS", 4000, True), ("C3", 4000, True)])
def test_tables_on_is_the_device_arithmetic_oracle(built, config, P, generic):
    w = _case(config, P, generic=generic, seed=5)
    ctx = _ctx(w)
    ctx.set_plan(layer_tables=3)
    sdf, ts, g, _ = ctx.query_points(w["coeffs"], w["T"])
    assert [r["targ"][0] for r in ctx.last_launches() if r["kernel"] == "layer_tables"] == [3]
    o = orc.Oracle(w["shape"], safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], poly_params=w["poly_params"],
                   polygon=w["polygon"], head_state=w["head_state"], tail_state=w["tail_state"])
    o.set_traj(w["coeffs"], w["T"])
    o.set_modes(1, 0)     # the device library's trig, the reference's chain of subtractions
    osdf, ots, og = o.query(w["points"], nthreads=NT)
    same_t, same_s, same_g = ts == ots, sdf == osdf, (g == og).all(axis=1)
    print(f"{config}: identical t* {same_t.mean():.5f}  sdf {same_s.mean():.5f}  grad {same_g.mean():.5f} of {P}")
    assert same_t.all() and same_s.all() and same_g.all()
    ctx.close()


def test_rule_leaves_small_clouds_alone_and_serves_large_ones(built):
    """layer_tables = AUTO: a reference-scale cloud (hundreds of points) never builds tables -- its launch chain is what it
    was --, a cloud whose solves read many times the poses the tables hold does, from the first evaluation on."""
    small = _case("C3", 600)
    ctx = _ctx(small)
    for _ in range(3):
        ctx.eval_penalty(small["coeffs"], small["T"])
        assert "layer_tables" not in {r["kernel"] for r in ctx.last_launches()}
    assert ctx.get_plan()["layer_tables"] == -1
    ctx.close()
    large = _case("C3", 200000)
    ctx = _ctx(large)
    for _ in range(3):
        ctx.eval_penalty(large["coeffs"], large["T"])
        assert [r["targ"][0] for r in ctx.last_launches() if r["kernel"] == "layer_tables"] == [3]
    ctx.close()
