"""CPU prototype of the certified clearance search under a scale schedule ("Under a scale schedule"),
on the oracle's values: no GPU.  The search of svsdf_min_clearance without its tile broad phase -- level-0 intervals at most
0.15 s wide, a pair of half width h around m bounded below by

    sdf_sc(p, m) - h (V Imax + W |u(m)| + Q |p - x(m)|) (1 + 1e-9) - 1e-9,

settled against upper - eps or halved -- with V, W from svsdf_motion_bounds and Imax, Q from svsdf_scale_bounds over the
level-0 interval widened by 1e-4 s.  `drop` removes one term of the bound, to show on an input that the term carries:

    drop = "imax"   V in place of V Imax          (the rigid speed term)
    drop = "q"      no Q |p - x(m)|               (the scale treated as frozen over the interval)
    drop = "u"      W |p - x(m)| in place of W |u(m)|   (the rigid yaw term)

A dropped term that carries gives a bracket whose lower end lies ABOVE a densely sampled minimum.  The three inputs of
tests/test_scaled_clearance_gpu.py (speed_case, scale_rate_case, yaw_case) are run by

    python tools/scaled_clearance_prototype.py

which prints, per input, the full bound's bracket, the dropped-term bracket and the dense minimum.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "implicit-svsdf-planner_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def search(o, coeffs, T, pts, sched, eps=1e-3, drop=None, max_level=40):
    """(lower, upper, levels, evals) of min over pts and [0, sum T] of the oracle's scaled SDF-at-time."""
    import svsdf_amd
    td = float(np.sum(T))
    n0 = max(1, int(np.ceil(td / 0.15)))
    if td / n0 > 0.15:
        n0 += 1
    w = td / n0
    VW = [svsdf_amd.motion_bounds(coeffs, T, j * w - 1e-4, (j + 1) * w + 1e-4) for j in range(n0)]
    SB = [svsdf_amd.scale_bounds(sched, j * w - 1e-4, (j + 1) * w + 1e-4) for j in range(n0)]
    pairs = [(p, j, 0) for p in range(len(pts)) for j in range(n0)]
    upper, settled, opened, evals, levels = np.inf, np.inf, np.inf, 0, 0
    for L in range(max_level + 1):
        h = w / 2.0 ** (L + 1)
        thr = upper - eps
        vals = []
        for (p, j, k) in pairs:
            m = min((j + (2 * k + 1) / 2.0 ** (L + 1)) * w, td)
            f, ux, uy = o.rel_at_time(pts[p:p + 1, :2], [m])[0]
            x = o.pos(m)
            D, U = float(np.hypot(pts[p, 0] - x[0], pts[p, 1] - x[1])), float(np.hypot(ux, uy))
            V, W = VW[j]
            Imax, Q = SB[j][2], SB[j][3]
            slope = V * (1.0 if drop == "imax" else Imax) + W * (D if drop == "u" else U) + (0.0 if drop == "q" else Q * D)
            vals.append((f, f - (h * slope * (1.0 + 1e-9) + 1e-9)))
        evals += len(pairs)
        levels += 1
        if L == 0:                      # (level 0's threshold: the smallest value of the level itself, as the seed gives the device one)
            thr = min(v[0] for v in vals) - eps
        upper = min(upper, min(v[0] for v in vals))
        nxt, opened = [], np.inf
        for (p, j, k), (f, lb) in zip(pairs, vals):
            if lb >= thr:
                settled = min(settled, lb)
            else:
                opened = min(opened, lb)
                nxt += [(p, j, 2 * k), (p, j, 2 * k + 1)]
        pairs = nxt
        if not pairs:
            break
    return min(upper, settled, opened), upper, levels, evals


def dense_min(o, T, pts, n):
    tt = np.concatenate([np.linspace(0.0, float(np.sum(T)), n), [0.0], np.cumsum(T)])
    return min(float(o.rel_at_time(np.repeat(pts[p:p + 1, :2], len(tt), axis=0), tt)[:, 0].min()) for p in range(len(pts)))


def main():
    from oracle import orc
    import test_scaled_clearance_gpu as tc      # the three inputs are defined beside their tests

    for label, case, drop, n_dense in (("speed", tc.speed_case, "imax", 200000), ("scale rate", tc.scale_rate_case, "q", 20000),
                                      ("yaw rate", tc.yaw_case, "u", 200000)):
        shape, coeffs, T, hs, ts, pts, sched, poly = case()
        o = orc.Oracle(shape, head_state=hs, tail_state=ts, polygon=poly)
        o.set_traj(coeffs, T)
        o.set_scale(**sched)
        full = search(o, coeffs, T, pts, sched)
        part = search(o, coeffs, T, pts, sched, drop=drop)
        d = dense_min(o, T, pts, n_dense)
        print(f"{label}: full bound [{full[0]:.6f}, {full[1]:.6f}] levels {full[2]} evals {full[3]};  drop={drop} "
              f"[{part[0]:.6f}, {part[1]:.6f}] levels {part[2]} evals {part[3]};  dense {d:.6f};  "
              f"violated by the dropped form: {part[0] > d + 1e-9};  by the full form: {full[0] > d + 1e-9}", flush=True)


if __name__ == "__main__":
    main()
