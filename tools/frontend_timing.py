"""Time the resident front-end map and the batched successor test beside the route a caller had before them.

On the reference's star demo map (resolution 1, kernels 17 / 18, margin 0.5) and on a synthetic 1024 x 1024 map at 30 %
occupancy:
  - frontend_set_map (bitmap upload, byte kernels, yaw-free table),
  - astar_successors for 1, 64 and 4096 parents,
  - the host route for the same edges, given the child yaws: OccupancyMap.gather per child, then one
    check_sub_sw_collision over all of them (it covers step 4 only: the yaws come from astar_successors here).
Then the search itself (--search-maps): astar_search start -> end on the three demo scenarios (each with its own shape) and
corner to corner on the synthetic map, beside the route a caller had before it -- a Python open-set loop over
astar_successors with one parent per call (the parent of each call depends on the result of the one before).  Both routes
must return the same cells and counters.
Median of --steps runs after --warmup.  Prints one line per measurement; nothing else is asserted.

    python tools/frontend_timing.py [--steps 20] [--warmup 3] [--maps star synthetic] [--search-maps star sdHorseshoe sdHeart synthetic]
"""
import argparse
import heapq
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "implicit-svsdf-planner_amd")]

import numpy as np  # noqa: E402

import svsdf_amd  # noqa: E402
from svsdf_amd import workload  # noqa: E402

KS, KC, MARGIN = 17, 18, 0.5


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _synthetic_cloud(n, rng):
    g = rng.random((n, n)) < 0.3
    ii, jj = np.nonzero(g)
    c = np.column_stack([ii + 0.5, jj + 0.5, np.full(len(ii), 0.5)])
    return np.vstack([[[0.0, 0.0, 0.0], [float(n), float(n), 1.0]], c]).astype(np.float32)


def _host_route(ctx, om, info, ij, yaw, cyaw, stage):
    """What the same edges cost without the resident map: one gather per child, one batched collision check."""
    bmin = info["bmin"]
    half = [float(KS // 2 + 1)] * 2 + [0.0]
    sel = np.argwhere((stage == 0) | (stage == 4))

    def run():
        fs, cs, pts = [], [], []
        for p, s in sel:
            vi, vj = ij[p, 0] + s // 3 - 1, ij[p, 1] + s % 3 - 1
            c = np.array([vi + 0.5 + bmin[0], vj + 0.5 + bmin[1], 0.0])
            pts.append(om.gather(c[None], half)[:, :2])
            fs.append([ij[p, 0] + 0.5 + bmin[0], ij[p, 1] + 0.5 + bmin[1], yaw[p]])
            cs.append([c[0], c[1], cyaw[p, s]])
        if fs:
            ctx.check_sub_sw_collision(np.array(fs), np.array(cs), pts)
    return run, len(sel)


def _heu(i, j, gi, gj):
    dx, dy = abs(i - gi), abs(j - gj)
    return (math.sqrt(3) * 0 + math.sqrt(2) * min(dx, dy) + (max(dx, dy) - min(dx, dy))) * (1 + 1.0 / 1000)


def _loop_search(ctx, X, Y, start, goal, start_yaw=0.0):
    """AstarPathSearch (front_end_Astar.hpp:243-365) on the host, one astar_successors call per expanded node: the
    separate start node, pop by (key, insertion number), the three id branches with the stale key of the id == 1 one."""
    nid = np.zeros((X, Y), dtype=np.int8)
    g = np.zeros((X, Y))
    yaw = np.zeros((X, Y))
    father = {}
    heap, seq = [(_heu(*start, *goal), 0, -2)], 1
    nid[start] = 1
    cnt = dict(expansions=0, pushes=1, relaxed_open=0, reopened=0)
    while heap:
        _, _, cur = heapq.heappop(heap)
        ci, cj = start if cur == -2 else divmod(cur, Y)
        fy, gcur = (start_yaw, 0.0) if cur == -2 else (yaw[ci, cj], g[ci, cj])
        if cur != -2:
            nid[ci, cj] = -1
        if (ci, cj) == goal:
            cells = []
            while cur != -2:
                cells.append(divmod(cur, Y))
                cur = father[cur]
            return "FOUND", [start] + cells[::-1], cnt
        ok, cy, _ = ctx.astar_successors([[ci, cj]], [fy])
        cnt["expansions"] += 1
        for s in np.nonzero(ok[0])[0]:
            i, j = s // 3 - 1, s % 3 - 1
            v = (ci + i, cj + j)
            tg = math.sqrt(i * i + j * j) + gcur
            was = nid[v]
            if was == 0:
                yaw[v] = cy[0, s]
            elif not tg < g[v]:
                continue
            father[v[0] * Y + v[1]] = cur
            g[v] = tg
            if was == 1:
                cnt["relaxed_open"] += 1
                continue
            nid[v] = 1
            heapq.heappush(heap, (tg + _heu(*v, *goal), seq, v[0] * Y + v[1]))
            seq += 1
            cnt["pushes"] += 1
            cnt["reopened"] += int(was == -1)
    return "EXHAUSTED", [], cnt


def _time_search(name, a, rng):
    assets = workload._assets()
    shape = "star" if name == "synthetic" else name
    cloud = _synthetic_cloud(1024, rng) if name == "synthetic" else np.array(assets["maps"][name], dtype=np.float32)
    om = svsdf_amd.OccupancyMap(cloud, resolution=1.0)
    info = om.info()
    X, Y = info["dims"][:2]
    bmin = info["bmin"]
    if name == "synthetic":
        start, end = [0.5, 0.5, 0.5], [X - 0.5, Y - 0.5, 0.5]
    else:
        start, end = assets["scenarios"][name]["start"], assets["scenarios"][name]["end"]
    cell = lambda p: (min(int(math.floor(p[0] - bmin[0])), X - 1), min(int(math.floor(p[1] - bmin[1])), Y - 1))
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0)
    ctx.frontend_set_map(om, KS, KC, MARGIN)
    r = ctx.astar_search(start, end)
    ms = _median_ms(lambda: ctx.astar_search(start, end), a.steps, a.warmup)
    status, cells, cnt = _loop_search(ctx, X, Y, cell(start), cell(end))
    same = status == r["status"] and [tuple(c) for c in r["cells"]] == cells and all(cnt[k] == r[k] for k in cnt)
    lms = _median_ms(lambda: _loop_search(ctx, X, Y, cell(start), cell(end)), max(1, a.steps // 4), 1)
    eps = r["expansions"] / (ms * 1e-3) if ms > 0 else float("nan")
    print(f"{name} {X} x {Y} search: {r['status']}, {r['path_len']} cells, {r['expansions']} expansions, {r['launches']} launches: "
          f"astar_search {ms:.3f} ms ({eps:.0f} expansions / s); loop over astar_successors {lms:.3f} ms "
          f"({r['expansions'] / (lms * 1e-3):.0f} expansions / s); same result: {same}", flush=True)
    if a.slices and r["expansions"] > 1:
        for sl in a.slices:
            sms = _median_ms(lambda: ctx.astar_search(start, end, slice=sl), a.steps, a.warmup)
            print(f"{name} slice {sl}: astar_search {sms:.3f} ms", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", nargs="*", default=["star", "synthetic"])
    ap.add_argument("--host-max", type=int, default=64, help="largest parent batch the host route is timed for")
    ap.add_argument("--search-maps", nargs="*", default=["star", "sdHorseshoe", "sdHeart", "synthetic"])
    ap.add_argument("--slices", nargs="*", type=int, default=[], help="also time astar_search with these slice sizes")
    a = ap.parse_args()
    rng = np.random.default_rng(20240607)
    hand_out = [2 * 3.1415926536 * k / KC - 3.1415926536 for k in range(KC)]
    ctx = svsdf_amd.SvsdfContext(shape="star", device=0)
    for name in a.maps:
        cloud = np.array(workload._assets()["maps"]["star"], dtype=np.float32) if name == "star" else _synthetic_cloud(1024, rng)
        om = svsdf_amd.OccupancyMap(cloud, resolution=1.0)
        info = om.info()
        X, Y = info["dims"][:2]
        ms = _median_ms(lambda: ctx.frontend_set_map(om, KS, KC, MARGIN), a.steps, a.warmup)
        free = ctx.yaw_free()
        print(f"{name} {X} x {Y}: frontend_set_map {ms:.3f} ms; cells with a free yaw {int((free != 0).sum())} of {free.size}",
              flush=True)
        for n in (1, 64, 4096):
            ij = np.column_stack([rng.integers(0, X, n), rng.integers(0, Y, n)]).astype(np.int32)
            yaw = np.array([hand_out[k] for k in rng.integers(0, KC, n)])
            ms = _median_ms(lambda: ctx.astar_successors(ij, yaw), a.steps, a.warmup)
            ok, cyaw, stage = ctx.astar_successors(ij, yaw)
            hist = np.bincount(stage.ravel(), minlength=5).tolist()
            line = f"{name} {n} parents: astar_successors {ms:.3f} ms; stages 0..4 {hist}"
            if n <= a.host_max:
                run, edges = _host_route(ctx, om, info, ij, yaw, cyaw, stage)
                hms = _median_ms(run, a.steps, a.warmup)
                line += f"; host gather + check_sub_sw_collision of the {edges} edges with a yaw {hms:.3f} ms"
            print(line, flush=True)
    ctx.close()
    for name in a.search_maps:
        _time_search(name, a, rng)


if __name__ == "__main__":
    main()
