"""The trajectory intake on the host (csrc/svsdf_traj_host.hpp: check_traj, the duration rule, scan_times, cull_table,
motion_bounds, piece_time_mode), compiled for the host alone with the address and undefined-behaviour sanitizers and run
once (tests/cpp/traj_host.cpp).  The exact cull's table is compared by memcmp with the loop upload_traj carried before the
header existed, written out in the program; motion_bounds bit for bit with values recorded through svsdf_motion_bounds
from the library of the commit named in tests/golden/motion_bounds_parent.json, which had its own copy of the bound."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_traj_host_under_sanitizers(tmp_path):
    gold = json.load(open(os.path.join(HERE, "golden", "motion_bounds_parent.json")))
    assert len(gold["parent_commit"]) == 40
    trajs = gold["trajectories"]
    data = str(tmp_path / "traj_host.txt")
    with open(data, "w") as f:          # per trajectory: N | T | coeffs (column-major, as the C ABI takes them) | stale dur | n | n x (ta tb V W)
        for t in trajs:
            assert len(t["coeffs"]) == 18 * len(t["T"]) and len(t["intervals"]) >= 10
            f.write(" ".join([str(len(t["T"]))] + t["T"] + t["coeffs"] + [t["stale_dur"], str(len(t["intervals"]))]
                             + [v for row in t["intervals"] for v in row]) + "\n")
    exe = str(tmp_path / "traj_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "traj_host.cpp")])
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    lines = out.strip().split("\n")
    assert lines[-1] == "all checks passed"
    # every recorded interval was compared, on N = 1, 5 (generic), 32 (dyadic 2.5 s) and the tail trajectory
    bounds = [ln.split() for ln in lines if ln.startswith("bounds")]
    assert [int(b[4].rstrip(":")) for b in bounds] == [len(t["T"]) for t in trajs] and [len(t["T"]) for t in trajs][:3] == [1, 5, 32]
    assert [(int(b[5]), int(b[7])) for b in bounds] == [(len(t["intervals"]),) * 2 for t in trajs]
    # the cull table: each trajectory in the regular regime, with and without a tail chunk; one more under a stale duration
    cull = [dict(zip(ln.split()[1::2], ln.split()[2::2])) for ln in lines if ln.startswith("cull")]
    regular = [c for c in cull if c["ok"] == "1"]
    stale = [c for c in cull if c["ok"] == "0"]
    assert len(regular) == len(trajs) and len(stale) >= 1
    assert all(c["finite"] == c["chunks"] for c in regular) and all(c["finite"] == "0" for c in stale)
    assert {c["tail"] for c in regular} == {"0", "1"}
    assert [sum(ln.startswith(k) for ln in lines) for k in ("piece_time", "scan", "check ")] == [5, 3, 11]
