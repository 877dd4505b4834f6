"""Time the query-point producer: the host route beside the device route, in one process.

  host route    svsdf_map_create + svsdf_frontend_set_map + svsdf_map_gather + svsdf_set_points
  device route  svsdf_map_build_device + svsdf_frontend_set_map_device + svsdf_set_points_from_map

on the three demo maps (resolution 1, the scenario's waypoints, half extents kernel_size * resolution / 3) and on one fine
map: a 4 M-point cloud uniform over (30.5, 75, 2) at resolution 0.05 (610 x 1500 x 40 cells), 23 waypoints along the
sdHorseshoe scenario's path, half extents 17 / 3 m.  Median of --steps runs after --warmup, every run ending in a device
synchronise (the calls synchronise themselves).  Both routes must leave the same cloud behind: the gathered lists and the
shard indices are compared once per map.  Per stage: the three calls of each route, and the device route's own build_ms /
gather_ms (svsdf_map_device_info) and setup_ms.  One JSON line per map; nothing else is asserted.

    python tools/producer_timing.py [--steps 10] [--warmup 2] [--maps star sdHorseshoe sdHeart fine] [--device-only]

--device-only skips the host route (for a kernel trace of the device route alone).  The counting kernel moves 12 bytes in
and one 4-byte atomic out per cloud point: `count_bytes` in the output is that total, to divide by the kernel's traced time.
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
KS, KC, MARGIN = 17, 18, 0.5


def _case(name):
    if name == "fine":
        rng = np.random.default_rng(4_000_000)
        cloud = (rng.random((4_000_000, 3)) * np.array([30.5, 75.0, 2.0])).astype(np.float32)
        sc = ASSETS["scenarios"]["sdHorseshoe"]
        centres = workload.waypoints(sc["start"][:2], sc["end"][:2], 24)       # 23 interior waypoints
        return "sdHorseshoe", cloud, 0.05, centres, np.full(3, 17 * 1.0 / 3.0)
    sc = ASSETS["scenarios"][name]
    cloud = np.array(ASSETS["maps"][name], dtype=np.float32)
    centres = workload.waypoints(sc["start"][:2], sc["end"][:2], 8)
    return name, cloud, sc["occupancy_resolution"], centres, np.full(3, sc["kernel_size"] * sc["occupancy_resolution"] / 3.0)


def _timed(fns, steps, warmup):
    """fns: list of (label, callable) run in order; returns {label: median ms, "total": median ms of the sum}."""
    rows = []
    for it in range(warmup + steps):
        row = []
        for _, fn in fns:
            t0 = time.perf_counter()
            fn()
            row.append((time.perf_counter() - t0) * 1e3)
        if it >= warmup:
            rows.append(row)
    a = np.array(rows)
    out = {label: float(np.median(a[:, k])) for k, (label, _) in enumerate(fns)}
    out["total"] = float(np.median(a.sum(axis=1)))
    return out


def run(name, steps, warmup, device_only):
    shape, cloud, res, centres, halfbd = _case(name)
    out = {"map": name, "n_cloud": len(cloud), "resolution": res, "centres": len(centres), "steps": steps, "warmup": warmup,
           "count_bytes": 16 * len(cloud)}
    dev = svsdf_amd.SvsdfContext(shape=shape, device=0)
    extra = {}

    def d_gather():
        dev.set_points_from_map(centres, halfbd)
        mi = dev.map_info()
        for k in ("build_ms", "gather_ms"):
            extra.setdefault(k, []).append(mi[k])

    out["device"] = _timed([("map_build", lambda: dev.map_build(cloud, res, 1)),
                            ("frontend_set_map_resident", lambda: dev.frontend_set_map_resident(KS, KC, MARGIN)),
                            ("set_points_from_map", d_gather)], steps, warmup)
    mi = dev.map_info()
    out.update(dims=list(mi["dims"]), occupied=mi["occupied"], gathered=mi["gathered"])
    out["device"].update({k: float(np.median(v[warmup:])) for k, v in extra.items()})
    if not device_only:
        host = svsdf_amd.SvsdfContext(shape=shape, device=0)
        st = {}

        def h_create():
            st["m"] = svsdf_amd.OccupancyMap(cloud, res, 1)

        def h_gather():
            st["pts"] = st["m"].gather(centres, halfbd)

        out["host"] = _timed([("map_create", h_create), ("frontend_set_map", lambda: host.frontend_set_map(st["m"], KS, KC, MARGIN)),
                              ("map_gather", h_gather), ("set_points", lambda: host.set_points(st["pts"]))], steps, warmup)
        same = (np.array_equal(dev.map_points(), st["pts"]) and np.array_equal(dev.shard_indices(), host.shard_indices())
                and np.array_equal(dev.yaw_free(), host.yaw_free()))
        out["same_result"] = bool(same)
        out["speedup"] = out["host"]["total"] / out["device"]["total"]
        host.close()
    dev.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maps", nargs="*", default=["star", "sdHorseshoe", "sdHeart", "fine"])
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    for name in a.maps:
        run(name, a.steps, a.warmup, a.device_only)


if __name__ == "__main__":
    main()
