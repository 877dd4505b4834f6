"""Time svsdf_min_clearance beside svsdf_query_points, today's only (uncertified) way to ask how close a trajectory comes.

  three reference maps   the whole demo map's occupied-voxel centres as the cloud, the 24-piece trajectory of bench.py's
                         reference_scale case (workload.reference_case, first iterate)
  C3                     1 M corridor points, 32 pieces (workload.make("C3"))

At eps 1e-3, without a target and with target = 0: median wall ms of --steps calls after --warmup (the call synchronises
itself), the device time the call reports, evals, tile_pairs_kept / tile_pairs, levels, pairs; next to them the median
time of svsdf_query_points on the same cloud and the minimum it reports.  One JSON line per case; nothing is asserted.

--per-point: svsdf_point_clearance on the same four cases instead, with cap = the context's safety_hor and without a cap
(median wall ms, device ms, status, levels, evals, pairs, the state counts, the global bracket), and beside them
svsdf_min_clearance without a target and svsdf_query_points on the same cloud: the ratio to svsdf_min_clearance is the
figure of interest, and how many of the points svsdf_query_points reads clear (sdf > 0) the certified upper puts in
collision (upper < 0).

--scaled: the same cases under the reference's worked scale schedule (binding.EXAMPLE_SCALE) on a context created with
FLAG_SCALED_CLEARANCE: the scaled search ("Under a scale schedule").  The lines carry "scaled": true
and the schedule; svsdf_query_points beside them runs under the same schedule.  The rigid lines are the comparison.

    python tools/clearance_timing.py [--steps 5] [--warmup 1] [--cases star sdHorseshoe sdHeart C3] [--per-point] [--scaled] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

try:
    import torch  # noqa: F401  (first: one HIP runtime per process, as in bench.py)
except Exception:
    pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "implicit-svsdf-planner_amd")]

import numpy as np  # noqa: E402

import svsdf_amd  # noqa: E402
from svsdf_amd import workload  # noqa: E402

ASSETS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_assets.json")))


def _case(name, flags=0):
    """(context, coeffs, T, number of points, safety_hor)"""
    if name == "C3":
        w = workload.make("C3", minco=svsdf_amd.minco_coeffs)
        kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], poly_params=w["poly_params"],
                  head_state=w["head_state"], tail_state=w["tail_state"], polygon=w["polygon"])
        ctx = svsdf_amd.SvsdfContext(shape=w["shape"], device=0, flags=flags, **kw)
        ctx.set_points(w["points"])
        return ctx, w["coeffs"], w["T"], len(w["points"]), float(w["safety_hor"])
    w = workload.reference_case(name, N=24, iterates=1)
    sc = ASSETS["scenarios"][name]
    c = np.array(ASSETS["maps"][name], dtype=np.float32).astype(np.float64)      # every occupied voxel's centre
    res = sc["occupancy_resolution"]
    pts = c.min(axis=0) + (np.unique(np.floor((c - c.min(axis=0)) / res).astype(np.int64), axis=0) + 0.5) * res
    kw = dict(safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"], poly_params=w["poly_params"],
              head_state=w["head_state"], tail_state=w["tail_state"])
    ctx = svsdf_amd.SvsdfContext(shape=name, device=0, flags=flags, **kw)
    coeffs, T = ctx.lmbm_prepare(w["xs"][0])
    ctx.set_points(pts)
    return ctx, coeffs, T, len(pts), float(w["safety_hor"])


def _median_ms(fn, steps, warmup):
    ts, last = [], None
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        last = fn()
        if it >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", nargs="+", default=["star", "sdHorseshoe", "sdHeart", "C3"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--per-point", action="store_true", help="time svsdf_point_clearance (see above)")
    ap.add_argument("--scaled", action="store_true", help="under binding.EXAMPLE_SCALE on a FLAG_SCALED_CLEARANCE context")
    a = ap.parse_args()
    for name in a.cases:
        ctx, coeffs, T, P, safety_hor = _case(name, svsdf_amd.FLAG_SCALED_CLEARANCE if a.scaled else 0)
        row = {"case": name, "points": P, "pieces": len(T), "duration_s": float(np.sum(T)), "eps": 1e-3}
        if a.scaled:
            ctx.set_scale(**svsdf_amd.binding.EXAMPLE_SCALE)
            row["scaled"] = True
            row["schedule"] = svsdf_amd.binding.EXAMPLE_SCALE
        upper = None
        if a.per_point:
            row["mode"] = "per_point"
            row["safety_hor"] = safety_hor
            for label, cap in (("cap_safety_hor", safety_hor), ("no_cap", None)):
                ms, out = _median_ms(lambda: ctx.point_clearance(coeffs, T, eps=1e-3, cap=cap), a.steps, a.warmup)
                r = out[4]
                row[label] = {"median_ms": ms, **{k: r[k] for k in ("device_ms", "status", "levels", "lower", "upper", "t_witness",
                                                                     "point_index", "evals", "pairs", "tile_pairs",
                                                                     "tile_pairs_kept", "counts")}}
                upper = out[1]
        for label, target in (("no_target", None),) if a.per_point else (("no_target", None), ("target_0", 0.0)):
            ms, r = _median_ms(lambda: ctx.min_clearance(coeffs, T, eps=1e-3, target=target), a.steps, a.warmup)
            row[label] = {"median_ms": ms, **{k: r[k] for k in ("device_ms", "status", "levels", "lower", "upper", "t_witness",
                                                                 "evals", "pairs", "tile_pairs", "tile_pairs_kept")}}
        # the foreign call itself, arguments marshalled once (sdf only; no reordering to the input order)
        from svsdf_amd.binding import _colmajor, _p
        cm, Tc, sdf = _colmajor(coeffs), np.ascontiguousarray(T, dtype=np.float64), np.zeros(ctx.num_points())
        ms, rc = _median_ms(lambda: ctx.L.svsdf_query_points(ctx.ctx, len(Tc), _p(cm), _p(Tc), _p(sdf), None, None),
                            a.steps, max(a.warmup, 6))   # (its launch plan settles first)
        row["query_points"] = {"median_ms": ms, "rc": rc, "min_sdf": float(sdf.min()), "sdf_evals": int(ctx.stats()["sdf_evals"])}
        if upper is not None:   # (sdf is in shard order: bring the certified upper into it)
            up = upper[ctx.shard_indices()]
            row["query_points"]["reads_clear"] = int((sdf > 0.0).sum())
            row["query_points"]["reads_clear_but_upper_below_0"] = int(((sdf > 0.0) & (up < 0.0)).sum())
            row["per_point_over_min_clearance"] = row["no_cap"]["median_ms"] / row["no_target"]["median_ms"]
        ctx.close()
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
