"""Time the scaled path (svsdf_set_scale) beside the rigid one: ms per svsdf_eval_penalty of a workload, rigid and with
the reference's example schedule (s_x = 0.8 + sin(1.5 t - 1.0) 0.6, s_y = sin(1.8 t) 0.4 + 0.8), and the full callback of
the three reference-scale maps.  Prints one line per measurement; nothing is asserted.

    python tools/scale_timing.py [--configs C3 NS] [--steps 20] [--maps]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "implicit-svsdf-planner_amd")]

import numpy as np  # noqa: E402

import svsdf_amd  # noqa: E402
from svsdf_amd import workload  # noqa: E402
from svsdf_amd.binding import EXAMPLE_SCALE  # noqa: E402


def _ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C3", "NS"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--maps", action="store_true", help="also the reference-scale maps (full callback)")
    a = ap.parse_args()
    for name in a.configs:
        w = workload.make(name, minco=svsdf_amd.minco_coeffs)
        ctx = svsdf_amd.SvsdfContext(shape=w["shape"], safety_hor=w["safety_hor"], weight_p=w["weight_p"], rho=w["rho"],
                                     head_state=w["head_state"], tail_state=w["tail_state"], device=0)
        ctx.set_points(w["points"])
        for label, sched in (("rigid", None), ("example schedule", EXAMPLE_SCALE)):
            ctx.set_scale(None) if sched is None else ctx.set_scale(**sched)
            ms = _ms(lambda: ctx.eval_penalty(w["coeffs"], w["T"]), a.steps, a.warmup)
            st = ctx.stats()
            print(f"{name} {label}: {ms:.3f} ms per evaluation; points {st['points']}, interior {st['interior_points']}, "
                  f"solves {st.get('solves', 0)}, plan {ctx.get_plan()}", flush=True)
        ctx.close()
    if a.maps:
        for m in ("star", "sdHorseshoe", "sdHeart"):   # the three demo maps of the README table
            case = workload.reference_case(m)
            ctx = svsdf_amd.SvsdfContext(shape=case["shape"], safety_hor=case["safety_hor"], weight_p=case["weight_p"],
                                         rho=case["rho"], poly_params=case["poly_params"], head_state=case["head_state"],
                                         tail_state=case["tail_state"], device=0)
            ctx.set_points(case["points"])
            x = case["xs"][0]
            for label, sched in (("rigid", None), ("example schedule", EXAMPLE_SCALE)):
                ctx.set_scale(None) if sched is None else ctx.set_scale(**sched)
                us = 1e3 * _ms(lambda: ctx.lmbm_evaluate(np.asarray(x)), a.steps * 5, a.warmup)
                print(f"{m} {label}: {us:.0f} us per full callback ({len(case['points'])} points)", flush=True)
            ctx.close()


if __name__ == "__main__":
    main()
