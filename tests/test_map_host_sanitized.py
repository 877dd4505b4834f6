"""The host half of the device producer (csrc/svsdf_points.hpp: GridGeometry::centre_boxes, path_waypoints) compiled for the
host alone with the address and undefined-behaviour sanitizers and run once (tests/cpp/mapgeom_host.cpp), on the bounds of
cloud S1 of tests/test_map_device_gpu.py.  The boxes it prints are compared with a numpy restatement of projInMap
(PCSmap_manager.h:128-135) + getGridIndex (Gridmap3D.cpp:137-177)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _index(p, bmin, bmax, res, dims):
    if (p < bmin).any() or (p > bmax).any():
        return [0, 0, 0]
    i = np.floor((p - bmin) / res).astype(int)
    return list(np.minimum(np.maximum(i, 0), dims - 1))


def _boxes(centres, halfbd, bmin, bmax, res, dims):
    out, last = [], np.array([999.0, 999.0, 999.0])
    for c in centres:
        row = []
        for ctr in (c, last):
            a = np.minimum(np.maximum(ctr - halfbd, bmin), bmax)
            b = np.minimum(np.maximum(ctr + halfbd, bmin), bmax)
            row += _index(a, bmin, bmax, res, dims) + _index(b, bmin, bmax, res, dims)
        out.append([int(v) for v in row])
        last = c
    return out


def test_centre_boxes_and_waypoints_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mapgeom_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "mapgeom_host.cpp")])
    rng = np.random.default_rng(20240807)
    cloud = (rng.random((700, 3)) * np.array([12.0, 20.0, 3.0])).astype(np.float32).astype(np.float64)    # S1
    bmin, bmax, res = cloud.min(axis=0), cloud.max(axis=0), 1.0
    r = subprocess.run([exe] + [repr(float(v)) for v in bmin] + [repr(float(v)) for v in bmax] + [repr(res)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    lines = out.strip().split("\n")
    assert lines[-1] == "all checks passed"
    assert lines[0] == "dims 12 20 3 cells 720"
    ex = np.array([12.0, 20.0, 3.0])
    centres = np.array([[f * ex[0], f * ex[1], 0.4] for f in (0.1, 0.3, 0.3, 0.55, 0.8)] + [[ex[0] + 5, ex[1] + 5, 0.4]])
    got = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("box")]
    assert got == _boxes(centres, np.full(3, 17 * res / 3), bmin, bmax, res, np.array([12, 20, 3]))
    assert got[2][:6] == got[2][6:]            # the repeated centre: its box is the previous one's
    assert int([ln for ln in lines if ln.startswith("gathered")][0].split()[1]) > 100
