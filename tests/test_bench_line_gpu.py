"""bench.py on one GPU: a plain run prints the headline alone; --full adds the other measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("full_callback_ms", "roofline", "generic_durations", "cpu_baseline", "north_star", "reference_scale")


def _bench(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_line_is_the_headline(built, tmp_path):
    r = _bench(["--config", "C2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r["metric"] == "SVSDF query-points/sec (cost+grad) per optimizer evaluation"
    assert r["unit"] == "query-points/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - r["config"]["points_total"] / (r["ms_per_step"] * 1e-3)) <= 1e-9 * r["value"]
    assert not [k for k in FULL_ONLY if k in r]
    # nothing but the settle, warm-up and timed evaluations ran on the headline workload
    assert r["evaluations_in_this_run"] == r["setup"]["settle_evaluations"] + 1 + 3
    assert np.load(tmp_path / "grad_coeffs.npy").shape == (6 * r["config"]["pieces"], 3)


@pytest.mark.gpu
def test_bench_full_line_keeps_the_other_measurements(built):
    r = _bench(["--config", "C2", "--steps", "3", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline"])
    assert r["full_callback_ms"] > 0 and r["roofline"]["kernel_ms_per_step"] > 0
    assert r["generic_durations"]["ms_per_step"] > 0
    assert r["evaluations_in_this_run"] > r["setup"]["settle_evaluations"] + 1 + 3
