"""Time-varying robot scale (svsdf_set_scale), host side and code objects -- no GPU needed.

  * set / get round trip and every refusal on a SVSDF_FLAG_HOST_ONLY context, through the C ABI (ctypes), the Python
    TrajOptimizer mirror and the C++ mirror (include/svsdf_traj_optimizer.hpp, compiled here with g++);
  * the per-evaluation arithmetic restated in plain Python: S^-1 as Eigen's 3x3 inverse() forms it (cofactors times
    1 / det), u = (Rt^T S^-1)(p - x); hand-checked values, and c = 1, A = 0 reducing to the rigid u bit for bit;
  * the built library holds a scaled kernel for every compiled shape id, no scaled GSIP-round kernel exists, and the scaled
    solve kernels keep the scratch / spill counts pinned below.
"""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "implicit-svsdf-planner_amd")
EXAMPLE = {"c": (0.8, 0.8), "amp": (0.6, 0.4), "omega": (1.5, 1.8), "phase": (-1.0, 0.0)}


def _host_ctx():
    import svsdf_amd
    return svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)


# ---------------------------------------------------------------- interface
def test_round_trip_c_abi(built):
    from svsdf_amd.binding import Scale, EXAMPLE_SCALE
    ctx = _host_ctx()
    assert ctx.get_scale() is None                    # no schedule: the rigid path
    ctx.set_scale(**EXAMPLE_SCALE)
    assert ctx.get_scale() == {k: tuple(v) for k, v in EXAMPLE_SCALE.items()}
    # raw struct through the C ABI: every field as given
    s = Scale()
    s.struct_size = C.sizeof(Scale)
    assert ctx.L.svsdf_get_scale(ctx.ctx, C.byref(s)) == 0
    assert s.enabled == 1 and list(s.c) == [0.8, 0.8] and list(s.phase) == [-1.0, 0.0]
    ctx.set_scale(None)                                # NULL restores the rigid path
    assert ctx.get_scale() is None
    ctx.set_scale(**EXAMPLE_SCALE)
    ctx.set_scale(c=(2.0, 2.0), enabled=False)         # so does enabled = 0
    assert ctx.get_scale() is None
    s = Scale()
    s.struct_size = C.sizeof(Scale)
    assert ctx.L.svsdf_get_scale(ctx.ctx, C.byref(s)) == 0
    assert s.enabled == 0 and list(s.c) == [1.0, 1.0] and list(s.amp) == [0.0, 0.0]   # the identity
    ctx.set_scale(c=(1.5, 0.5))                        # a constant scale: A = 0
    assert ctx.get_scale()["c"] == (1.5, 0.5)
    ctx.close()


@pytest.mark.parametrize("bad, what", [
    (dict(c=(0.8, 0.8), amp=(0.8, 0.4)), "can reach 0"),      # c_x - |A_x| = 0: the singular scale (SWM:493)
    (dict(c=(0.8, 0.3), amp=(0.6, -0.4)), "can reach 0"),     # |A| counts, not A
    (dict(c=(-1.0, 1.0)), "can reach 0"),
    (dict(c=(1.0, float("nan"))), "non-finite"),
    (dict(c=(1.0, 1.0), omega=(float("inf"), 1.0)), "non-finite"),
    (dict(c=(1.0, 1.0), phase=(0.0, -float("inf"))), "non-finite"),
    (dict(c=(1.0, 1.0), amp=(float("nan"), 0.0)), "non-finite"),
    (dict(c=(1.0, 1.0), struct_size=8), "struct_size"),
])
def test_refusals(built, bad, what):
    from svsdf_amd import SvsdfError
    from svsdf_amd.binding import EXAMPLE_SCALE
    ctx = _host_ctx()
    ctx.set_scale(**EXAMPLE_SCALE)
    with pytest.raises(SvsdfError, match=what):
        ctx.set_scale(**bad)
    assert ctx.get_scale() == {k: tuple(v) for k, v in EXAMPLE_SCALE.items()}   # a refused call changes nothing
    ctx.close()


def test_get_scale_checks_struct_size(built):
    from svsdf_amd.binding import Scale
    ctx = _host_ctx()
    s = Scale()
    s.struct_size = 4
    assert ctx.L.svsdf_get_scale(ctx.ctx, C.byref(s)) == 1      # SVSDF_ERR_INVALID
    assert ctx.L.svsdf_set_scale(None, None) == 1
    ctx.close()


def test_python_traj_optimizer_mirror(built):
    from svsdf_amd import SvsdfError
    from svsdf_amd.traj_optimizer import TrajOptimizer
    opt = TrajOptimizer()
    assert opt.getScale() is None
    opt.setScale(EXAMPLE)
    assert opt.getScale() == EXAMPLE
    with pytest.raises(SvsdfError, match="can reach 0"):
        opt.setScale({"c": (0.5, 1.0), "amp": (0.5, 0.0), "omega": (1.0, 1.0), "phase": (0.0, 0.0)})
    assert opt.getScale() == EXAMPLE
    opt.setScale(None)
    assert opt.getScale() is None


CPP = r'''
#include <cmath>
#include <cstdio>
#include "svsdf_traj_optimizer.hpp"
int main() {
  svsdf::TrajOptimizerHip opt;
  svsdf_scale s{}, g{};
  s.struct_size = (int)sizeof(svsdf_scale); s.enabled = 1;
  s.c[0] = 0.8; s.c[1] = 0.8; s.amp[0] = 0.6; s.amp[1] = 0.4; s.omega[0] = 1.5; s.omega[1] = 1.8; s.phase[0] = -1.0;
  g.struct_size = (int)sizeof(svsdf_scale);
  int r0 = opt.getScale(&g);
  std::printf("%d %d %.17g\n", r0, g.enabled, g.c[0]);
  int r1 = opt.setScale(&s);
  g = svsdf_scale{}; g.struct_size = (int)sizeof(svsdf_scale);
  opt.getScale(&g);
  std::printf("%d %d %.17g %.17g %.17g %.17g\n", r1, g.enabled, g.c[0], g.amp[1], g.omega[1], g.phase[0]);
  svsdf_scale bad = s; bad.amp[0] = 0.8;                       // c - |A| = 0
  svsdf_scale nf = s; nf.omega[1] = NAN;
  svsdf_scale sz = s; sz.struct_size = 8;
  std::printf("%d %d %d\n", opt.setScale(&bad), opt.setScale(&nf), opt.setScale(&sz));
  g = svsdf_scale{}; g.struct_size = (int)sizeof(svsdf_scale);
  opt.getScale(&g);
  std::printf("%d %.17g\n", g.enabled, g.amp[0]);              // unchanged by the refusals
  std::printf("%d ", opt.setScale(nullptr));
  g = svsdf_scale{}; g.struct_size = (int)sizeof(svsdf_scale);
  opt.getScale(&g);
  std::printf("%d\n", g.enabled);
  return 0;
}
'''


def test_cpp_mirror(built):
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "scale.cpp"), os.path.join(td, "scale")
        open(src, "w").write(CPP)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                               "-L", PKG, "-lsvsdf_hip", "-Wl,-rpath," + PKG])
        lines = subprocess.check_output([exe]).decode().splitlines()
    assert lines[0].split() == ["0", "0", "1"]
    assert lines[1].split() == ["0", "1", "0.80000000000000004", "0.40000000000000002", "1.8", "-1"]
    assert lines[2].split() == ["1", "1", "1"]
    assert lines[3].split() == ["1", "0.59999999999999998"]
    assert lines[4].split() == ["0", "0"]


# ---------------------------------------------------------------- arithmetic restated
def s_of(sc, t):
    """s_x(t), s_y(t) = c + sin(w t + phi) A, operation for operation (libm sin)."""
    return tuple(sc["c"][a] + math.sin(sc["omega"][a] * t + sc["phase"][a]) * sc["amp"][a] for a in (0, 1))


def inv_eigen(sx, sy):
    """Eigen's 3x3 inverse() of diag(sx, sy, 1): cofactors of column 0 -> det = sum(cof0 .* col0), invdet = 1 / det,
    row 0 = cof0 * invdet, (1, 1) = cofactor(1, 1) * invdet."""
    cof00 = sy * 1.0 - 0.0 * 0.0
    det = (cof00 * sx + (0.0 * 0.0 - 1.0 * 0.0) * 0.0) + (0.0 * 0.0 - 0.0 * sy) * 0.0
    invdet = 1.0 / det
    return cof00 * invdet, (1.0 * sx - 0.0 * 0.0) * invdet


def u_scaled(cs, sn, x, y, px, py, i00, i11):
    """(Rt^T S^-1) formed as a matrix, then times (p - x) (SWM:528-535)."""
    dx, dy = px - x, py - y
    return (cs * i00) * dx + (sn * i11) * dy, ((-sn) * i00) * dx + (cs * i11) * dy


def u_rigid(cs, sn, x, y, px, py):
    dx, dy = px - x, py - y
    return cs * dx + sn * dy, (-sn) * dx + cs * dy


def test_inverse_form_hand_values():
    assert inv_eigen(2.0, 0.5) == (0.5, 2.0)                 # det 1
    assert inv_eigen(4.0, 2.0) == (0.25, 0.5)                 # det 8, invdet 0.125: 2 * 0.125, 4 * 0.125
    i00, i11 = inv_eigen(3.0, 7.0)
    assert i00 == 7.0 * (1.0 / 21.0) and i11 == 3.0 * (1.0 / 21.0)
    # the cofactor form is not 1 / s: the two differ in the last bit for some scales (so the form is a real assumption)
    rng = np.random.default_rng(3)
    diff = 0
    for sx, sy in rng.uniform(0.2, 1.4, (2000, 2)):
        a, b = inv_eigen(float(sx), float(sy))
        diff += (a != 1.0 / sx) + (b != 1.0 / sy)
        assert abs(a * sx - 1.0) <= 4e-16 and abs(b * sy - 1.0) <= 4e-16
    assert diff > 0
    assert inv_eigen(1.0, 1.0) == (1.0, 1.0)


def test_example_schedule_hand_values():
    sx, sy = s_of(EXAMPLE, 0.0)
    assert sx == 0.8 + math.sin(-1.0) * 0.6 and sy == 0.8          # sin(1.8 * 0 + 0) = 0: s_y = 0.8 exactly
    assert abs(sx - (0.8 - 0.6 * 0.8414709848078965)) < 1e-15
    # phase -1.0 reproduces the reference's "1.5 * t - 1.0" and phase 0 its "1.8 * t" bit for bit
    for t in np.linspace(0.0, 40.0, 4001):
        t = float(t)
        assert 1.5 * t + (-1.0) == 1.5 * t - 1.0 and 1.8 * t + 0.0 == 1.8 * t
        rx, ry = s_of(EXAMPLE, t)
        assert rx == 0.8 + math.sin(1.5 * t - 1.0) * 0.6 and ry == math.sin(1.8 * t) * 0.4 + 0.8
        assert rx >= 0.8 - 0.6 and ry >= 0.8 - 0.4
    # u by hand: yaw 0 (cs = 1, sn = 0), S = diag(2, 0.5): u = (0.5 dx, 2 dy)
    i00, i11 = inv_eigen(2.0, 0.5)
    assert u_scaled(1.0, 0.0, 1.0, 2.0, 3.0, 5.0, i00, i11) == (1.0, 6.0)
    # yaw 90 deg (cs = 0, sn = 1): u = (i11 dy, -i00 dx)
    assert u_scaled(0.0, 1.0, 0.0, 0.0, 3.0, 5.0, i00, i11) == (10.0, -1.5)


def test_identity_schedule_reduces_to_rigid_bit_for_bit():
    ident = {"c": (1.0, 1.0), "amp": (0.0, 0.0), "omega": (1.3, -0.7), "phase": (0.2, 5.0)}
    rng = np.random.default_rng(11)
    for _ in range(3000):
        t = float(rng.uniform(0, 60))
        sx, sy = s_of(ident, t)
        assert sx == 1.0 and sy == 1.0
        i00, i11 = inv_eigen(sx, sy)
        assert i00 == 1.0 and i11 == 1.0
        yaw = float(rng.uniform(-7, 7))
        cs, sn = math.cos(yaw), math.sin(yaw)
        x, y, px, py = (float(v) for v in rng.uniform(-30, 30, 4))
        assert u_scaled(cs, sn, x, y, px, py, i00, i11) == u_rigid(cs, sn, x, y, px, py)
        # the assembly's -(S^-1)^T R g with i = 1 is the rigid (-c g0 + s g1, -s g0 - c g1)
        g0, g1 = (float(v) for v in rng.uniform(-1, 1, 2))
        assert ((-i00) * cs) * g0 + ((-i00) * (-sn)) * g1 == (-cs) * g0 + sn * g1
        assert ((-i11) * sn) * g0 + ((-i11) * cs) * g1 == (-sn) * g0 + (-cs) * g1


# ---------------------------------------------------------------- code objects
def _kr():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# a scaled kernel is the instantiation whose trailing template parameter pack holds ScaleDev (rigid: an empty pack or none)
SCALED_RE = re.compile(r"(k_solve|k_classify|k_debug_sdf_at|k_round|k_tail)I((?:Li\d+E)+)JNS_8ScaleDevEE")
# k_solve<S, G, 1, ScaleDev>, G = 4, 8, 32: (scratch bytes per lane, spilled VGPRs) of today's build
SOLVE_SC_CEIL = {s: {4: (0, 0), 8: (0, 0), 32: (0, 0)} for s in range(16)}
SOLVE_SC_CEIL[16] = {4: (44, 14), 8: (44, 14), 32: (44, 14)}   # (the Polygon: like its rigid k_solve, a few spilled VGPRs)
SOLVE_SC_CEIL[17] = {4: (52, 16), 8: (52, 16), 32: (52, 16)}


@pytest.fixture(scope="module")
def scaled_kernels():
    kr = _kr()
    lib = kr._lib()
    res = {}
    for co in kr.code_objects(lib):
        for k in kr._kernel_notes(co):
            m = SCALED_RE.search(k.get("name", ""))
            if m:
                key = (m.group(1),) + tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(2)))
                res[key] = {"scratch": int(k["private_segment_fixed_size"]), "spill": int(k.get("vgpr_spill_count", 0))}
        for k in kr._kernel_notes(co):
            if k.get("name", "").startswith("_ZN5svsdf8k_reduceIJNS_8ScaleDevEE"):
                res[("k_reduce",)] = {"scratch": int(k["private_segment_fixed_size"]), "spill": 0}
    return res


def test_every_shape_id_has_scaled_kernels(scaled_kernels):
    """18 compiled shape ids (17 = the Polygon with its edges in LDS) x k_solve<S, G, 1, ScaleDev> for G = 4, 8, 32;
    k_classify<S, ScaleDev> and k_debug_sdf_at<S, ScaleDev> for the 17 shapes; one k_reduce<ScaleDev>."""
    for s in range(18):
        for g in (4, 8, 32):
            assert ("k_solve", s, g, 1) in scaled_kernels, (s, g)
    for s in range(17):
        assert ("k_classify", s) in scaled_kernels, s
        assert ("k_debug_sdf_at", s) in scaled_kernels, s
    assert ("k_reduce",) in scaled_kernels


def test_no_scaled_round_kernel_and_no_new_scratch(scaled_kernels):
    """The scaled path runs the launch chain with the rigid k_round (its GSIP rounds do no S(t) arithmetic): no round-type
    scaled kernel exists, so none can have scratch.  The scaled solves stay at today's scratch and spill counts."""
    assert not [k for k in scaled_kernels if k[0] in ("k_round", "k_tail")]
    bad = []
    for (fam, *args), v in scaled_kernels.items():
        if fam == "k_solve":
            cs, cv = SOLVE_SC_CEIL[args[0]][args[1]]
            if v["scratch"] > cs or v["spill"] > cv:
                bad.append(f"k_solve<{args[0]}, {args[1]}, 1, ScaleDev>: {v['scratch']} B, {v['spill']} spilled (ceiling {cs}, {cv})")
        elif fam in ("k_classify", "k_debug_sdf_at", "k_reduce") and v["scratch"] > 0:
            bad.append(f"{fam}{tuple(args)}: {v['scratch']} B")
    assert not bad, "; ".join(bad)
