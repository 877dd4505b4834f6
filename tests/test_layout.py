"""The four packed blobs of the host layer around the hot path (csrc/svsdf_layout.hpp: sub-swept batch, successor batch, A*
blob, Polygon blob): every offset and total equals the index arithmetic the host code carried before each layout was written
once.  Compiled for the host alone, with the address and undefined-behaviour sanitizers (tests/cpp/layout_host.cpp)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_layouts_equal_the_former_index_arithmetic(tmp_path):
    exe = str(tmp_path / "layout_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "layout_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    lines = out.strip().split("\n")
    assert lines[-1] == "all layouts equal"
    # 3 x 3 sub-swept, 3 successor, 3 A*, 2 x 2 Polygon cases ran
    assert [sum(ln.startswith(k) for ln in lines) for k in ("subsw", "succ", "astar", "poly")] == [9, 3, 3, 4]
