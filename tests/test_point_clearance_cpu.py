"""svsdf_point_clearance without a device: the documented defaults, the order of the argument checks on a host-only context,
and the order-preserving key its per-point minima rest on (csrc/svsdf_ordkey.hpp), compiled for the host alone with the
address and undefined-behaviour sanitizers (tests/cpp/ordkey_host.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _traj(rng, N):
    """The recipe of test_clearance_cpu.py."""
    import svsdf_amd
    T = rng.uniform(0.4, 3.0, N)
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3))
    hs[:2, 0] = rng.uniform(0, 10, 2); ts[:2, 0] = hs[:2, 0] + rng.uniform(-10, 10, 2)
    q = np.column_stack([np.linspace(hs[0, 0], ts[0, 0], N + 1)[1:-1], np.linspace(hs[1, 0], ts[1, 0], N + 1)[1:-1],
                         rng.uniform(-2.5, 2.5, N - 1)])
    return svsdf_amd.minco_coeffs(hs, ts, q, T), T


def test_params_default(built):
    import svsdf_amd
    from svsdf_amd import binding
    prm = binding.PointClearanceParams()
    svsdf_amd.lib().svsdf_point_clearance_params_default(C.byref(prm))
    assert prm.struct_size == C.sizeof(binding.PointClearanceParams) == 48
    assert prm.eps == 1e-3 and prm.cap == np.inf and prm.target != prm.target
    assert prm.max_evals == 0 and prm.pair_capacity == 0
    assert C.sizeof(binding.PointClearanceResult) == 120
    svsdf_amd.lib().svsdf_point_clearance_params_default(None)          # a null pointer is ignored
    assert binding.POINT_STATE == ["CONVERGED", "FAR", "SAFE", "UNSAFE", "OPEN"]


def test_argument_checks_on_a_host_only_context(built):
    """null arguments, struct_size, eps, cap -- each SVSDF_ERR_INVALID with this entry's name -- and only then
    SVSDF_ERR_NO_DEVICE."""
    import svsdf_amd
    from svsdf_amd import binding
    L = svsdf_amd.lib()
    dp = C.POINTER(C.c_double)
    coeffs, T = _traj(np.random.default_rng(2), 4)
    cm = np.asfortranarray(coeffs).ravel(order="F").copy()
    p = lambda a: a.ctypes.data_as(dp)
    ctx = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY)
    res = binding.PointClearanceResult()

    def call(prm=None, coeffs_p=p(cm), T_p=p(T), out=C.byref(res), handle=ctx.ctx):
        rc = L.svsdf_point_clearance(handle, 4, coeffs_p, T_p, None if prm is None else C.byref(prm), None, None, None, None, out)
        return rc, L.svsdf_last_error_string(handle).decode()

    def params(**kw):
        prm = binding.PointClearanceParams()
        L.svsdf_point_clearance_params_default(C.byref(prm))
        for k, v in kw.items():
            setattr(prm, k, v)
        return prm

    for kw in (dict(coeffs_p=None), dict(T_p=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("svsdf_point_clearance: null argument"), (kw, rc, msg)
    assert call(handle=None)[0] == 1
    # every check below comes before the device is asked for: a bad value AND a host-only context answers INVALID
    rc, msg = call(params(struct_size=8, eps=-1.0))
    assert rc == 1 and "struct_size" in msg and msg.startswith("svsdf_point_clearance:"), msg
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        rc, msg = call(params(eps=eps, cap=float("nan")))
        assert rc == 1 and "eps" in msg and msg.startswith("svsdf_point_clearance:"), (eps, msg)
    rc, msg = call(params(cap=float("nan")))
    assert rc == 1 and "cap" in msg and msg.startswith("svsdf_point_clearance:"), msg
    for prm in (None, params(), params(cap=0.5, target=0.0), params(cap=-np.inf)):
        assert call(prm)[0] == 2                                         # SVSDF_ERR_NO_DEVICE
    # and the Python mirror raises the same
    with pytest.raises(svsdf_amd.SvsdfError, match=r"svsdf_point_clearance failed \(2\)"):
        ctx.point_clearance(coeffs, T)
    with pytest.raises(svsdf_amd.SvsdfError, match=r"failed \(1\).*cap"):
        ctx.point_clearance(coeffs, T, cap=float("nan"))
    ctx.close()


def test_order_preserving_key(tmp_path):
    exe = str(tmp_path / "ordkey_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "ordkey_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    lines = out.strip().split("\n")
    assert lines[0] == "random pairs 1000000" and lines[1].startswith("specials ") and lines[-1] == "ordkey ok", out
