"""Register and scratch budget of the shipped hot-path kernels, read from the gfx950 code objects of the built library.

The code object notes (llvm-readelf --notes, as tools/slice_regs.sh reads them for one slice) give every kernel's
.private_segment_fixed_size (scratch bytes per lane), .vgpr_spill_count and .vgpr_count.  A library holds one offload
bundle per translation unit in its .hip_fatbin section; the bundles are split here by their header
(__CLANG_OFFLOAD_BUNDLE__, entry count, then offset / size / target triple per entry) and the gfx950 entries are read.

Held here:
  * no k_round has scratch (two k_round builds with scratch faulted the device) -- except an
    8-byte private segment that no instruction touches in k_round<Polygon, 8, 1 .. 3> (ROUND_UNUSED_SCRATCH below);
  * k_tail<., ., 2> (the latency instantiation, launch_tail) has the bytes it has today: none for the analytic shapes, 12 B
    for the two Polygon ids in the scanning bound modes (svsdf_kernels.hpp, k_tail);
  * k_tail<., ., 3> and k_solve stay at or below today's scratch bytes and spilled VGPRs, kernel by kernel.

SVSDF_CHECK_LIB=<path to a libsvsdf_hip*.so> checks another build (a variant made with build.build(extra_flags=...,
out=...)) instead of the in-tree one; `python tests/test_kernel_resources.py [lib]` prints the per-family table.
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = b"hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# the rigid instantiations only: k_solve and k_classify end in a parameter pack that is empty (JE) for the rigid kernel and
# holds ScaleDev for the scaled one (tests/test_scale_schedule.py has those)
NAME_RE = re.compile(r"(k_solve|k_round|k_tail|k_classify)I((?:Li\d+E)+)(?:JE)?E")

# Ceilings of today's build, kernel by kernel: shape id -> (scratch bytes per lane, spilled VGPRs) for MODE 0 .. 3 of
# k_tail<S, MODE, 3>, and for G = 1, 2, 4, 8, 16, 32 of k_solve<S, G, 1>.  Shape 17 is the Polygon with its edges in LDS.
TAIL3_CEIL = {
    0: [(268, 87), (292, 93), (296, 94), (296, 100)],
    1: [(260, 83), (292, 93), (296, 94), (296, 100)],
    2: [(268, 87), (308, 101), (288, 90), (296, 92)],
    3: [(260, 83), (292, 93), (296, 94), (296, 100)],
    4: [(268, 87), (292, 93), (288, 94), (304, 100)],
    5: [(260, 83), (292, 93), (288, 94), (296, 96)],
    6: [(272, 84), (300, 93), (296, 98), (304, 104)],
    7: [(260, 83), (292, 93), (288, 94), (296, 100)],
    8: [(284, 89), (308, 101), (304, 100), (316, 106)],
    9: [(264, 82), (292, 93), (288, 94), (296, 96)],
    10: [(268, 87), (308, 101), (288, 90), (296, 92)],
    11: [(268, 87), (308, 101), (288, 98), (296, 92)],
    12: [(268, 87), (292, 93), (288, 94), (296, 100)],
    13: [(260, 83), (292, 93), (288, 94), (304, 100)],
    14: [(260, 83), (292, 93), (288, 94), (304, 100)],
    15: [(276, 85), (300, 97), (296, 98), (304, 104)],
    16: [(416, 143), (420, 173), (412, 160), (408, 157)],
    17: [(416, 144), (404, 156), (412, 168), (412, 168)],
}
SOLVE_CEIL = {
    0: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    1: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    2: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    3: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    4: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    5: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    6: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    7: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    8: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    9: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    10: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    11: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    12: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    13: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    14: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    15: [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    16: [(76, 24), (64, 21), (36, 12), (36, 12), (36, 12), (36, 12)],
    17: [(96, 35), (64, 21), (52, 16), (44, 14), (44, 14), (52, 16)],
}
# k_tail<S, MODE, 2>: 12 B (two spilled VGPRs) for the Polygon ids in the scanning modes 1 .. 3, every other one 0
TAIL2_BYTES = {(s, m): 12 for s in (16, 17) for m in (1, 2, 3)}
# k_round<Polygon (edges in global memory), 8 lanes, MODE 1 .. 3>: 8 B of private segment and no instruction that reads or
# writes scratch.  The kernels spill ~ 200 SGPRs into VGPR lanes (as every k_round does); in these three one 4-byte spill
# slot outlives the lowering of those spills without a single access left (MIR before prologue / epilogue insertion:
# `stack:` holds one spill-slot, referenced nowhere), and a frame with a live-looking object gets the register scavenger's
# 4-byte emergency slot on top -- 8 B reserved, never addressed.  Removing it means moving the register allocation of the
# three kernels; the guard instead pins exactly these kernels at exactly this size AND checks their code for scratch access
# (test_allowed_round_scratch_is_never_addressed), so a real spill into it fails like any other k_round scratch.
ROUND_UNUSED_SCRATCH = {("k_round", 16, 8, m): 8 for m in (1, 2, 3)}
SCRATCH_ACCESS = re.compile(r"\b(scratch_(load|store)|buffer_(load|store)|buffer_atomic)\w*|src_private_base|flat_scratch")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"),):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if p is None:
        raise RuntimeError(f"{name} not found (ROCm's LLVM tools are needed to read the code objects)")
    return p


def code_objects(lib):
    """gfx950 code objects (ELF bytes) of every offload bundle in the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(td, "copy")],
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        data = open(fat, "rb").read()
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        off = pos + len(MAGIC) + 8
        for _ in range(n):
            o, size, tlen = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + tlen]
            off += tlen
            if triple == TARGET and size:
                out.append(data[pos + o:pos + o + size])
        pos = data.find(MAGIC, pos + 1)
    return out


def _kernel_notes(co):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        txt = subprocess.run([_tool("llvm-readelf"), "--notes", f.name], check=True, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE).stdout.decode()
    kernels, cur = [], None
    for line in txt.splitlines():
        if line.startswith("  - "):          # a kernel entry of amdhsa.kernels
            cur = {}
            kernels.append(cur)
            line = "    " + line[4:]
        elif not line.startswith("    ") or cur is None:
            if not line.startswith(" "):
                cur = None
            continue
        m = re.match(r"^    \.(\w+):\s+(\S+)", line)   # kernel-level keys only (arguments are nested deeper)
        if m:
            cur[m.group(1)] = m.group(2)
    return kernels


def hot_kernels(lib):
    """{(family, template args...): {"scratch", "spill", "vgpr"}} of the shape-templated hot-path kernels."""
    res = {}
    for co in code_objects(lib):
        for k in _kernel_notes(co):
            m = NAME_RE.search(k.get("name", ""))
            if not m:
                continue
            args = tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(2)))
            key = (m.group(1),) + args
            res[key] = {"scratch": int(k["private_segment_fixed_size"]), "spill": int(k.get("vgpr_spill_count", 0)),
                        "vgpr": int(k["vgpr_count"]), "symbol": k["name"], "co": co}
    return res


def _lib():
    p = os.environ.get("SVSDF_CHECK_LIB")
    if p:
        return p
    import __graft_entry__ as ge
    ge.build()
    import svsdf_amd
    return svsdf_amd.lib_path()


@pytest.fixture(scope="module")
def kernels():
    ks = hot_kernels(_lib())
    assert ks, "no hot-path kernels found in the library's gfx950 code objects"
    return ks


def test_every_shape_id_is_instantiated(kernels):
    """18 compiled shape ids x (6 k_solve widths, 8 k_round, 8 k_tail) + 17 k_classify: the set the tables below cover."""
    for s in range(18):
        for g in (1, 2, 4, 8, 16, 32):
            assert ("k_solve", s, g, 1) in kernels, (s, g)
        for lp in (8, 32):
            for mode in range(4):
                assert ("k_round", s, lp, mode) in kernels, (s, lp, mode)
        for mode in range(4):
            for w in (2, 3):
                assert ("k_tail", s, mode, w) in kernels, (s, mode, w)
    for s in range(17):
        assert ("k_classify", s) in kernels, s


def test_no_k_round_has_scratch(kernels):
    bad = sorted(f"k_round<{k[1]}, {k[2]}, {k[3]}>: {v['scratch']} B, {v['spill']} spilled VGPRs"
                 for k, v in kernels.items() if k[0] == "k_round" and v["scratch"] > ROUND_UNUSED_SCRATCH.get(k, 0))
    assert not bad, "k_round kernels with scratch: " + "; ".join(bad)


def disassembly(kernel):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(kernel["co"])
        f.flush()
        return subprocess.run([_tool("llvm-objdump"), "-d", f"--disassemble-symbols={kernel['symbol']}", f.name], check=True,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout.decode()


def test_allowed_round_scratch_is_never_addressed(kernels):
    for key in ROUND_UNUSED_SCRATCH:
        text = disassembly(kernels[key])
        assert text.count("s_endpgm") >= 1, key        # the kernel's code was found
        hits = sorted({m.group(0) for m in SCRATCH_ACCESS.finditer(text)})
        assert not hits, (key, hits)


def test_latency_tail_keeps_todays_bytes(kernels):
    got = {(k[1], k[2]): v["scratch"] for k, v in kernels.items() if k[0] == "k_tail" and k[3] == 2}
    want = {(s, m): TAIL2_BYTES.get((s, m), 0) for s in range(18) for m in range(4)}
    diff = sorted(f"k_tail<{s}, {m}, 2>: {got.get((s, m))} B, expected {want[(s, m)]} B"
                  for (s, m) in want if got.get((s, m)) != want[(s, m)])
    assert not diff, "; ".join(diff)


def _over(kernels, family, table, args_of):
    bad = []
    for s, row in table.items():
        for i, (cap_b, cap_sp) in enumerate(row):
            key = (family, s) + args_of(i)
            v = kernels[key]
            if v["scratch"] > cap_b or v["spill"] > cap_sp:
                bad.append(f"{family}<{', '.join(map(str, key[1:]))}>: {v['scratch']} B / {v['spill']} spilled VGPRs "
                           f"(ceiling {cap_b} B / {cap_sp})")
    return bad


def test_throughput_tail_within_todays_scratch(kernels):
    assert sorted(TAIL3_CEIL) == list(range(18))
    bad = _over(kernels, "k_tail", TAIL3_CEIL, lambda i: (i, 3))
    assert not bad, "; ".join(bad)


def test_solve_within_todays_scratch(kernels):
    assert sorted(SOLVE_CEIL) == list(range(18))
    bad = _over(kernels, "k_solve", SOLVE_CEIL, lambda i: ((1, 2, 4, 8, 16, 32)[i], 1))
    assert not bad, "; ".join(bad)


def table(kernels):
    """Per family: kernels, kernels with scratch, scratch bytes range, spilled VGPRs range, VGPRs range."""
    fams = {}
    for k, v in kernels.items():
        f = k[0] + ("<., ., %d>" % k[3] if k[0] == "k_tail" else "<., %d, .>" % k[2] if k[0] == "k_round" else "")
        fams.setdefault(f, []).append(v)
    lines = [f"{'family':<22}{'kernels':>8}{'w/ scratch':>11}{'scratch B':>12}{'spilled':>10}{'VGPRs':>10}"]
    for f in sorted(fams):
        vs = fams[f]
        rng = lambda key: f"{min(v[key] for v in vs)}-{max(v[key] for v in vs)}"
        lines.append(f"{f:<22}{len(vs):>8}{sum(v['scratch'] > 0 for v in vs):>11}{rng('scratch'):>12}{rng('spill'):>10}"
                     f"{rng('vgpr'):>10}")
    return "\n".join(lines)


if __name__ == "__main__":
    ks = hot_kernels(sys.argv[1] if len(sys.argv) > 1 else _lib())
    print(table(ks))
    if "--ceilings" in sys.argv:
        for fam, args_of, n in (("k_tail", lambda i: (i, 3), 4), ("k_solve", lambda i: ((1, 2, 4, 8, 16, 32)[i], 1), 6)):
            print(fam)
            for s in range(18):
                print(f"    {s}: [" + ", ".join("(%d, %d)" % (ks[(fam, s) + args_of(i)]["scratch"], ks[(fam, s) + args_of(i)]["spill"])
                                                for i in range(n)) + "],")
    if "--scratch" in sys.argv:
        for k, v in sorted(ks.items()):
            if v["scratch"]:
                print(k, v)
