#!/usr/bin/env python3
"""The census cases -> tests/golden/golden_census.json: points chosen so that every branch of the reference's solve that a
trajectory can reach is reached, recorded with what tests/path_census.py (make_golden's whole callback, counted) returns.

Trajectories (generic durations: the reference's chained piece location runs; x holds backwardT of the T below):
  A  make_golden's head, tail and waypoints with T = [2.2, 0.8, 2.4, 0.9]: two tau <= 0, rest to rest;
  B  near-stationary: (2, 1, 0) -> (2.1, 1.05, 0.02) -> (2.2, 1.1, 0.05), T = [30, 25]: speed below 0.01 throughout;
  C  one piece, T = [3.0], (2, 1, 0) with velocity (1, 0.5, 0.1) -> (8, 5, 0.7) with velocity (0.5, 1, -0.1).
All 17 shapes on A, B and C (Polygon: the 6-vertex outline of test_kernel_instantiations_gpu.py; the shapes with an entry
in that file's OFFSETS take it on one path); under the schedule scale_restatement.EXAMPLE the four shapes of
scale_restatement.CASES on A and C.  weight_p, rho and safety_hor vary over the cases.

Per case a seeded pool (points around the path and its two ends, and knee candidates bisected along rays to
solve(...)[0] = safety_hor - 0.005) is classified; candidates on which the C oracle's two trig modes differ by more than
half a project gate (5e-9 in sdf, 5e-7 in t*) are dropped (fewer than 2 %, asserted); 24 points are kept, greedily, so that
every branch the pool reaches keeps two representatives where it has them.  Exactly 24: 24 x 11 and 24 x 43 points put
the repeated clouds of test_path_census_gpu.py into the two larger reduction forms.

Not required, only counted (path_census.NEVER_REQUIRED; the CPU test holds the committed counts, so a change is noticed).
Believed unreachable, and at 0 in the pool and in the file:
  gd_exit_trials, gd_exit_tol  the descent always ends by 29 halvings: a step that does not lower f is halved to nothing
                               long before 1000 trials, and |x - prev| <= 1e-16 needs an accepted step of that size;
  t_tmin, t_tmax               t* on a window edge INSIDE the path: the window is +-3.4 s around a seed that the four scan
                               layers have already put within 0.15 ms of a local minimum;
  z0                           needs r_star == 0 exactly.
Believed unreachable before this census, and reached:
  positive                     an interior point whose result -r_star comes back positive.  Rigid: a few points just inside
                               the surface (sdHorseshoe, sdRoundedCross: +0.1 ... +3.7).  Under the schedule the shape value
                               is no distance (the scale stretches it up to 1 / 0.2), r - max_g overshoots, the ring leaves
                               the volume and the loop runs its nine rounds to values of 1e3 ... 1e5 m: every scaled case
                               has such points, all l1_inactive.  155 of the 9 051 pool points, 40 of the 1 416 kept.
  locate_fall_through          at t = dur the chain of subtractions can leave a remainder one ulp above the last duration
                               (TRJ:498-516 then steps back and gets the same local time).  Trajectory A only: 571 pool
                               points, 116 kept, in every shape.

Run:  python tests/golden/make_census.py        (minutes; needs oracle/liborc.so for the selection rule)
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import path_census as pc            # noqa: E402
from oracle import orc              # noqa: E402

mg = pc.mg
KEEP = 24
OUTLINE = [[1.6, 0.0], [0.7, 1.1], [-0.5, 1.3], [-1.4, 0.2], [-0.9, -1.1], [0.8, -1.2]]
OFFSETS = {"sdCutDisk": (0.0, -0.6, 0.0), "sdHeart": (0.3, -0.4, 25.0), "sdArc": (-0.4, 0.5, -140.0),
           "star": (0.5, 0.2, 10.0), "sdTrapezoid": (0.2, 0.1, 70.0)}
Z = [0.0, 0.0, 0.0]
TRAJ = {
    "A": dict(head=[[2.0, 1.0, 0.0], Z, Z], tail=[[14.0, 9.0, 0.0], Z, Z],
              q=[[5.0, 2.5, 0.4], [8.5, 6.0, -0.3], [11.0, 7.0, 0.5]], T=[2.2, 0.8, 2.4, 0.9]),
    "B": dict(head=[[2.0, 1.0, 0.0], Z, Z], tail=[[2.2, 1.1, 0.05], Z, Z], q=[[2.1, 1.05, 0.02]], T=[30.0, 25.0]),
    "C": dict(head=[[2.0, 1.0, 0.0], [1.0, 0.5, 0.1], Z], tail=[[8.0, 5.0, 0.7], [0.5, 1.0, -0.1], Z], q=[], T=[3.0]),
}
SHAPES = orc.SHAPES
SCALED = ["star", "sdHorseshoe", "sdHeart", "Polygon"]


def case_list():
    out = []
    for tn in "ABC":
        for s in SHAPES:
            pp = OFFSETS[s] if s in OFFSETS and "ABC"[sorted(OFFSETS).index(s) % 3] == tn else (0.0, 0.0, 0.0)
            out.append(dict(id=f"{tn}-{s}", traj=tn, shape=s, poly_params=list(pp), scale=None))
    for tn in "AC":
        for s in SCALED:
            out.append(dict(id=f"{tn}-{s}-scaled", traj=tn, shape=s, poly_params=[0.0, 0.0, 0.0],
                            scale={k2: list(v) for k2, v in pc.EXAMPLE.items()}))
    for k, c in enumerate(out):
        c.update(polygon=OUTLINE if c["shape"] == "Polygon" else None, weight_p=(60.0, 7.5)[k % 2],
                 rho=(3.8, 0.5)[(k // 2) % 2], safety_hor=round(0.5 + 0.05 * (k % 9), 2))
    return out


def radius(c):
    """the farthest point of the shape's interior from the body origin (0.25 grid), times the schedule's largest scale"""
    sh = pc.CensusShape(c["shape"], tuple(c["poly_params"]), c["polygon"])
    r = 0.5
    for i in range(-40, 41):
        for j in range(-40, 41):
            if sh.sdf(0.25 * i, 0.25 * j) <= 0:
                r = max(r, math.hypot(0.25 * i, 0.25 * j))
    return r * (1.4 if c["scale"] else 1.0)


def _knees(args):
    """worker: knee candidates of one case, by bisection of solve(...)[0] - (safety_hor - 0.005) along rays"""
    c, rows, durs, R, seed = args
    sw = pc.make_swept(c["shape"], tuple(c["poly_params"]), c["polygon"], rows, durs, c["scale"])
    rng = np.random.default_rng(seed)
    tr, want, out = sw.traj, c["safety_hor"] - 0.005, []
    solve = mg.Swept.solve if c["scale"] is None else pc.scr.ScaledSwept.solve      # (the inherited solve: nothing counted)
    for _ in range(10):
        o = tr.pos(float(rng.uniform(0, sw.dur)))
        a = float(rng.uniform(0, 2 * math.pi))
        f = lambda r: solve(sw, o[0] + r * math.cos(a), o[1] + r * math.sin(a))[0] - want
        lo = hi = None              # the first sign change along the ray, in steps of 0.25
        fa, ra = f(0.0), 0.0
        while ra < 3.0 * R + 2.0:
            fb = f(ra + 0.25)
            if (fa < 0) != (fb < 0):
                lo, hi = (ra, ra + 0.25) if fa < 0 else (ra + 0.25, ra)
                break
            fa, ra = fb, ra + 0.25
        if lo is None:
            continue
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            if f(mid) < 0:
                lo = mid
            else:
                hi = mid
        r = 0.5 * (lo + hi)
        out.append([round(o[0] + r * math.cos(a), 4), round(o[1] + r * math.sin(a), 4)])
    return out


def candidates(rows, durs, R, seed):
    """points around the path (96) and around its first and last pose (24 each), on a 1e-4 grid"""
    rng = np.random.default_rng(seed)
    tr = mg.Traj(rows, durs)
    dur, out = tr.total(), []
    for t0, t1, n, spread in ((0.0, dur, 96, 1.7), (0.0, 0.0, 24, 2.2), (dur, dur, 24, 2.2)):
        for t, a, r in zip(rng.uniform(t0, t1, n) if t1 > t0 else [t0] * n, rng.uniform(0, 2 * np.pi, n),
                           R * np.sqrt(rng.uniform(0, spread, n))):
            p = tr.pos(float(t))
            out.append([round(p[0] + float(r) * math.cos(float(a)), 4), round(p[1] + float(r) * math.sin(float(a)), 4)])
    return out


def oracle_for(c, tj):
    o = orc.Oracle(c["shape"], safety_hor=c["safety_hor"], weight_p=c["weight_p"], rho=c["rho"],
                   poly_params=c["poly_params"], polygon=c["polygon"], head_state=np.array(tj["head"]).T,
                   tail_state=np.array(tj["tail"]).T)
    o.set_traj(np.array(tj["coeffs"]), tj["T"])
    if c["scale"]:
        o.set_scale(**c["scale"])
    return o


def trig_mode_gap(c, tj, pts):
    """|sdf|, |t*| differences of the oracle's two trig modes at the points"""
    o = oracle_for(c, tj)
    xyz = np.array([[p[0], p[1], 0.0] for p in pts])
    o.set_modes(0, 0)
    s0, t0, _ = o.query(xyz, nthreads=8)
    o.set_modes(1, 0)
    s1, t1, _ = o.query(xyz, nthreads=8)
    return np.abs(s1 - s0), np.abs(t1 - t0)


def choose(recs, order):
    """indices of KEEP candidates: greedily, until every branch of the pool has two representatives (or all it has)"""
    feats = [pc.features(pc.decode(r)) for r in recs]
    need = {}
    for i in order:
        for b in feats[i]:
            need[b] = min(2, need.get(b, 0) + 1)
    kept = []
    while len(kept) < KEEP and any(v > 0 for v in need.values()):
        best = max((i for i in order if i not in kept), key=lambda i: sum(need.get(b, 0) > 0 for b in feats[i]))
        if not any(need.get(b, 0) > 0 for b in feats[best]):
            break
        kept.append(best)
        for b in feats[best]:
            if need.get(b, 0) > 0:
                need[b] -= 1
    assert not any(v > 0 for v in need.values()), need
    kept += [i for i in order if i not in kept][:KEEP - len(kept)]
    assert len(kept) == KEEP
    return sorted(kept)


def main():
    trajectories = {}
    for tn, tj in TRAJ.items():
        x = pc.backward_T(tj["T"]) + [v for w in tj["q"] for v in w]
        rows, durs = pc.coefficients(tj["head"], tj["tail"], x)
        trajectories[tn] = dict(head=tj["head"], tail=tj["tail"], x=x, T=durs, coeffs=rows)
    cases, pool_total, dropped_total = [], 0, 0
    pool_tab = {}
    with pc.executor() as ex:
        todo = case_list()
        Rs = [radius(c) for c in todo]
        knees = list(ex.map(_knees, [(c, trajectories[c["traj"]]["coeffs"], trajectories[c["traj"]]["T"], R, 500 + k)
                                     for k, (c, R) in enumerate(zip(todo, Rs))]))
        for k, (c, R) in enumerate(zip(todo, Rs)):
            tj = trajectories[c["traj"]]
            pts = candidates(tj["coeffs"], tj["T"], R, 9000 + k) + knees[k]
            ds, dt = trig_mode_gap(c, tj, pts)
            ok = [i for i in range(len(pts)) if ds[i] <= 5e-9 and dt[i] <= 5e-7]
            pool_total += len(pts)
            dropped_total += len(pts) - len(ok)
            pts = [pts[i] for i in ok]
            got = pc.census_points(ex, dict(c, points=pts), tj["coeffs"], tj["T"], [[p[0], p[1], 0.0] for p in pts])
            recs = [g[1] for g in got]
            for r in recs:
                for b in pc.features(pc.decode(r)):
                    pool_tab.setdefault(b, {}).setdefault(c["shape"], 0)
                    pool_tab[b][c["shape"]] += 1
            keep = choose(recs, list(range(len(pts))))
            c["points"] = [pts[i] for i in keep]
            c["pool"], c["dropped"] = len(ds), len(ds) - len(ok)
            res = pc.evaluate(ex, c, tj["head"], tj["tail"], tj["x"])
            assert res["rec"] == [recs[i] for i in keep] and res["per_point"] == [got[i][0] for i in keep]
            assert res["T"] == tj["T"]
            c.update(per_point=res["per_point"], rec=res["rec"], n_solves=res["n_solves"], cost=res["cost"],
                     costs3=res["costs3"], grad=res["grad"], tau_le0=[i for i in range(len(tj["T"])) if tj["x"][i] <= 0.0])
            cases.append(c)
            print(c["id"], "pool", c["pool"], "dropped", c["dropped"], "cost", c["cost"], "solves", c["n_solves"], flush=True)
    share = dropped_total / pool_total
    print("dropped by the trig-mode rule: %d of %d (%.3f %%)" % (dropped_total, pool_total, 100 * share))
    assert share < 0.02
    doc = dict(generator="tests/golden/make_census.py (tests/path_census.py over make_golden's restatement)",
               pool=pool_total, dropped=dropped_total, trajectories=trajectories, cases=cases)
    tab = pc.check_requirements(doc)
    doc["never_required"] = {b: sum(tab[b].values()) for b in pc.NEVER_REQUIRED}
    print("pool counts of the branches that are not required:", {b: sum(pool_tab.get(b, {}).values()) for b in pc.NEVER_REQUIRED})
    print("census (points per branch, shapes that show it):")
    for b in pc.ALL_BRANCHES:
        print("  %-20s %5d points, %2d shapes, least %s" % (b, sum(tab[b].values()), len(tab[b]),
                                                          min(tab[b].values()) if len(tab[b]) == 17 else 0))
    out = os.path.join(HERE, "golden_census.json")
    json.dump(doc, open(out, "w"), separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 229249


if __name__ == "__main__":
    main()
