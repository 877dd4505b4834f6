"""The C oracle's time-varying robot scale (orc_set_scale; the reference's useScale path, DESIGN.md sections 2 and 4c) -- no GPU.

  * Against the pure-Python restatement (tests/scale_restatement.py) under the reference's example schedule and under an
    anisotropic one with s > 1, on star, sdHorseshoe, sdHeart and the star.obj Polygon outline, clouds with interior (GSIP)
    points: the oracle of record (libm trig, the reference's piece location) on the restatement's own coefficients gives the
    restatement's per-point sdf, t* and gradient and its full callback to 1e-12 -- the bound the rigid oracle is held to
    against make_golden.py.
  * The identity schedule (c = 1, A = 0, any omega / phase) on all 17 shapes, libm and device trig: the bits of a context
    that never had a schedule, and so does a cleared one.
  * A constant schedule: the body-frame point is the hand formula with Eigen's cofactor inverse bit for bit -- not 1 / s.
  * The seed stays rigid: under a schedule the descent still starts from choiceTInit's rigid seed.
"""
import ctypes
import ctypes.util
import math
import os

import numpy as np
import pytest

from oracle import orc
from scale_restatement import EXAMPLE, HEAD, Q, T, TAIL, _points, _x, restated_cost_function

NT = min(16, os.cpu_count() or 1)
SCHEDULE_B = dict(c=(1.1, 0.9), amp=(0.35, 0.3), omega=(0.9, 2.3), phase=(0.4, -2.0))   # anisotropic, s_x up to 1.45
SHAPES = orc.SHAPES
OFFSETS = {"sdCutDisk": (0.0, -0.6, 0.0), "sdHeart": (0.3, -0.4, 25.0), "sdArc": (-0.4, 0.5, -140.0),
           "star": (0.5, 0.2, 10.0), "sdTrapezoid": (0.2, 0.1, 70.0)}
OUTLINE = np.array([[1.6, 0.0], [0.7, 1.1], [-0.5, 1.3], [-1.4, 0.2], [-0.9, -1.1], [0.8, -1.2]])
RESTATED = {"star": (0.7, 64), "sdHorseshoe": (0.7, 64), "sdHeart": (0.8, 64), "Polygon": (0.7, 24)}   # safety_hor, points


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _rel(a, b):
    """largest |a - b| relative to max(1, |b|)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("sched", ["A", "B"])
@pytest.mark.parametrize("shape", list(RESTATED))
def test_oracle_matches_the_restatement(built, shape, sched):
    from svsdf_amd import workload
    sc = EXAMPLE if sched == "A" else SCHEDULE_B
    safety_hor, n = RESTATED[shape]
    verts = [tuple(map(float, v)) for v in workload.mesh_outline("star")] if shape == "Polygon" else None
    pts = _points(shape, n, 140 + len(shape))
    x = _x()
    f_ref, g_ref, _, rows, Tv, per, _, main_f = restated_cost_function(shape, verts, pts, safety_hor, sc, x)
    per = np.array(per)
    n_in = int((np.array(main_f) <= 0).sum())
    assert n_in >= 8, f"the cloud needs interior points (GSIP): {n_in}"
    hs, ts = np.array(HEAD).T, np.array(TAIL).T
    o = orc.Oracle(shape, safety_hor=safety_hor, weight_p=60.0, rho=3.8, polygon=np.array(verts) if verts else None,
                   head_state=hs, tail_state=ts)          # modes (0, 0): the oracle of record
    xyz = np.array([[p[0], p[1], 0.0] for p in pts])
    o.set_traj(np.array(rows), Tv)
    rigid = o.penalty(xyz, nthreads=NT, per_point=True)
    o.set_scale(**sc)
    # per point, on the restatement's own trajectory coefficients
    _, _, _, sdf, tst, _ = o.penalty(xyz, nthreads=NT, per_point=True)
    grad = o.query(xyz, nthreads=NT)[2]
    d = (_rel(sdf, per[:, 0]), _rel(tst, per[:, 1]), _rel(grad, per[:, 2:4]))
    print(f"{shape} schedule {sched}: {n_in} interior of {n}; per point sdf {d[0]:.1e} t* {d[1]:.1e} grad {d[2]:.1e}")
    assert max(d) <= 1e-12, d
    assert (_bits(sdf) != _bits(rigid[3])).sum() > n // 4, "the schedule must visibly act"
    # the full callback
    f, g, _ = o.cost_function(xyz, np.array(x), nthreads=NT)
    g_ref = np.array(g_ref)
    df, dg = abs(f - f_ref) / abs(f_ref), np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref)
    print(f"{shape} schedule {sched}: callback f {df:.1e} g {dg:.1e}")
    assert df <= 1e-12 and dg <= 1e-12, (df, dg)
    o.set_scale(None)
    f0, _, _ = o.cost_function(xyz, np.array(x), nthreads=NT)
    assert abs(f0 - f_ref) > 1e-6 * abs(f_ref), "the rigid callback is another number"


# ---------------------------------------------------------------- identity / cleared schedule
def _case(shape, seed=0):
    """4 generic-duration pieces (tests/test_scale_gpu.py::_case, with the oracle's MINCO)"""
    rng = np.random.default_rng(9100 + SHAPES.index(shape) + 100 * seed)
    Tv = np.array([1.3, 2.2, 0.9, 1.7]) * rng.uniform(0.9, 1.1, 4)
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:, 0] = [0.0, 0.0, 0.4]
    ts[:, 0] = [14.0, 5.0, -1.2]
    q = np.array([[4.0, 3.0, 1.1], [8.0, 1.5, -0.6], [11.0, 4.5, 0.8]]) + rng.uniform(-0.5, 0.5, (3, 3))
    coeffs = orc.minco_coeffs(hs, ts, q, Tv)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, poly_params=OFFSETS.get(shape, (0.0, 0.0, 0.0)),
              polygon=OUTLINE if shape == "Polygon" else None, head_state=hs, tail_state=ts)
    return kw, coeffs, Tv


def _radius(o):
    """circumradius of the shape's zero set about the body origin, from a 0.1 m grid"""
    ax = np.arange(-9.0, 9.01, 0.1)
    xy = np.array([(a, b) for a in ax for b in ax])
    sdf = o.shape_eval(xy)
    return float(np.sqrt((xy[sdf <= 0] ** 2).sum(axis=1)).max())


def _cloud(o, Tv, n, R, seed):
    """n points around the path out to sqrt(1.6) R: about a third inside the swept volume"""
    rng = np.random.default_rng(seed)
    tt = rng.uniform(0.0, Tv.sum(), n)
    pos = np.array([o.pos(t)[:2] for t in tt])
    ang, rad = rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.6, n))
    pts = np.zeros((n, 3))
    pts[:, 0] = pos[:, 0] + rad * np.cos(ang)
    pts[:, 1] = pos[:, 1] + rad * np.sin(ang)
    return pts


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_schedule_is_the_rigid_oracle(built, shape):
    kw, coeffs, Tv = _case(shape)
    fresh, o = orc.Oracle(shape, **kw), orc.Oracle(shape, **kw)
    fresh.set_traj(coeffs, Tv)
    o.set_traj(coeffs, Tv)
    pts = _cloud(fresh, Tv, 300, _radius(fresh), 300 + SHAPES.index(shape))
    for trig in (0, 1):
        fresh.set_modes(trig, 0)
        o.set_modes(trig, 0)
        o.set_scale(None)
        want = fresh.penalty(pts, nthreads=NT, per_point=True) + fresh.query(pts, nthreads=NT)
        assert (want[3] <= 0).sum() >= 30, "the cloud needs interior points (GSIP)"
        o.set_scale(c=(1.0, 1.0), amp=(0.0, 0.0), omega=(1.5, -2.7), phase=(-1.0, 0.3))
        got = o.penalty(pts, nthreads=NT, per_point=True) + o.query(pts, nthreads=NT)
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(a), _bits(b)), (shape, trig, "identity schedule", k)
        # a schedule that acts, then cleared: the bits of the context that never had one
        o.set_scale(**EXAMPLE)
        acted = o.penalty(pts, nthreads=NT, per_point=True)
        assert (_bits(acted[3]) != _bits(want[3])).sum() > len(pts) // 4
        o.set_scale(None)
        got = o.penalty(pts, nthreads=NT, per_point=True) + o.query(pts, nthreads=NT)
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(a), _bits(b)), (shape, trig, "cleared schedule", k)


def test_set_scale_refuses_a_singular_schedule(built):
    o = orc.Oracle("star")
    for bad in (dict(c=(0.8, 0.8), amp=(0.8, 0.4)), dict(c=(1.0, float("nan"))), dict(c=(1.0, 1.0), omega=(float("inf"), 0.0))):
        with pytest.raises(ValueError):
            o.set_scale(**bad)


# ---------------------------------------------------------------- the inverse's form
def test_constant_schedule_is_the_cofactor_inverse(built):
    """c = (0.7, 1.3), A = 0 (no sine enters): u of orc_rel_at_time is the hand formula with i00 = s_y (1 / (s_y s_x)),
    i11 = s_x (1 / (s_y s_x)), bit for bit, and the 1 / s_x, 1 / s_y form gives other bits at some pairs.  (The same on the
    device: test_scale_restatement_gpu.py::test_inverse_form_is_pinned_on_the_device.)"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))    # the oracle's own sincos(): sin() / cos() may differ in the last bit
    libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    libm.sincos.restype = None
    kw, coeffs, Tv = _case("star")
    o = orc.Oracle("star", **kw)
    o.set_traj(coeffs, Tv)
    rng = np.random.default_rng(5)
    n = 512
    pxy = np.column_stack([rng.uniform(-2, 16, n), rng.uniform(-3, 8, n)])
    tt = rng.uniform(0, Tv.sum(), n)
    sx, sy = 0.7, 1.3
    o.set_scale(c=(sx, sy), omega=(1.5, 1.8), phase=(-1.0, 0.0))
    out = o.rel_at_time(pxy, tt)
    inv = 1.0 / (sy * sx)
    i00, i11 = sy * inv, sx * inv
    differs = 0
    for k in range(n):
        x, y, yaw = o.pos(tt[k])
        sn, cs = ctypes.c_double(), ctypes.c_double()
        libm.sincos(yaw, ctypes.byref(sn), ctypes.byref(cs))
        sn, cs = sn.value, cs.value
        dx, dy = pxy[k, 0] - x, pxy[k, 1] - y
        ux = (cs * i00) * dx + (sn * i11) * dy
        uy = ((-sn) * i00) * dx + (cs * i11) * dy
        assert _bits(ux) == _bits(out[k, 1]) and _bits(uy) == _bits(out[k, 2]), (k, ux, uy, out[k])
        assert _bits(out[k, 0]) == _bits(o.shape_eval([[ux, uy]])[0]) == _bits(o.sdf_at_time(pxy[k, 0], pxy[k, 1], tt[k]))
        wx = (cs * (1.0 / sx)) * dx + (sn * (1.0 / sy)) * dy
        wy = ((-sn) * (1.0 / sx)) * dx + (cs * (1.0 / sy)) * dy
        differs += int(wx != ux or wy != uy)
    assert differs > 0, "the scales chosen do not tell the two forms apart"
    # without a schedule the entry gives the rigid body-frame point
    o.set_scale(None)
    rig = o.rel_at_time(pxy, tt)
    assert (rig[:, 1] != out[:, 1]).all()
    assert all(_bits(rig[k, 0]) == _bits(o.sdf_at_time(pxy[k, 0], pxy[k, 1], tt[k])) for k in range(n))


def test_schedule_sine_and_operation_order(built):
    """s_a(t) = c_a + sin(w_a t + phi_a) A_a in that order with libm's sin (mode 0): u restated in Python from the pose."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    libm.sincos.restype = None
    kw, coeffs, Tv = _case("sdHorseshoe")
    o = orc.Oracle("sdHorseshoe", **kw)
    o.set_traj(coeffs, Tv)
    rng = np.random.default_rng(6)
    n = 512
    pxy = np.column_stack([rng.uniform(-2, 16, n), rng.uniform(-3, 8, n)])
    tt = rng.uniform(0, Tv.sum(), n)
    for sc in (EXAMPLE, SCHEDULE_B):
        o.set_scale(**sc)
        out = o.rel_at_time(pxy, tt)
        for k in range(n):
            t = float(tt[k])
            sx = sc["c"][0] + math.sin(sc["omega"][0] * t + sc["phase"][0]) * sc["amp"][0]
            sy = sc["c"][1] + math.sin(sc["omega"][1] * t + sc["phase"][1]) * sc["amp"][1]
            inv = 1.0 / (sy * sx)
            i00, i11 = sy * inv, sx * inv
            x, y, yaw = o.pos(t)
            sn, cs = ctypes.c_double(), ctypes.c_double()
            libm.sincos(yaw, ctypes.byref(sn), ctypes.byref(cs))
            dx, dy = pxy[k, 0] - x, pxy[k, 1] - y
            ux = (cs.value * i00) * dx + (sn.value * i11) * dy
            uy = ((-sn.value) * i00) * dx + (cs.value * i11) * dy
            assert _bits(ux) == _bits(out[k, 1]) and _bits(uy) == _bits(out[k, 2]), (k, t)


# ---------------------------------------------------------------- the seed
def _rigid_seed(o, px, py, dur):
    """choiceTInit (SWM:538-581) restated on the RIGID oracle's evaluation: four layers, accumulated t += dt, strict <"""
    min_dis, seed, dt, term, t = 1e9, 0.0, 0.15, dur, 0.0
    for layer in range(1, 5):
        if layer > 1:
            t = max(0.0, seed - 10 * dt)
            term = min(dur, seed + 10 * dt)
        while t <= term:
            dis = o.sdf_at_time(px, py, t)
            if dis < min_dis:
                seed, min_dis = t, dis
            t += dt
        dt *= 0.1
    return seed


def test_the_seed_stays_rigid(built):
    """choiceTInit calls the non-scale overloads (SWM:567-570): under a schedule the descent starts from the rigid seed and
    is confined to seed -+ 3.4 s.  The schedule here grows slowly and monotonically over the whole trajectory, so far outside
    the path the scaled distance falls all the way to the end: the scaled descent leaves the rigid seed, runs into the
    window's end and stops ON it, t* = seed + 3.4 exactly -- the rigid seed, restated here on a context without a schedule --
    although the scaled value is smaller later on, where a scaled scan would have put the seed."""
    hs, ts = np.array(HEAD).T, np.array(TAIL).T
    coeffs = orc.minco_coeffs(hs, ts, np.array(Q), np.array(T))
    dur = float(np.sum(T))                      # 9.3 s: longer than the window
    slow = dict(c=(0.8, 0.8), amp=(0.6, 0.6), omega=(0.25, 0.25), phase=(-1.0, -1.0))   # w t + phi in [-1, 1.33]: s rises
    rigid = orc.Oracle("sdHorseshoe", head_state=hs, tail_state=ts)
    scaled = orc.Oracle("sdHorseshoe", head_state=hs, tail_state=ts)
    rigid.set_traj(coeffs, T)
    scaled.set_traj(coeffs, T)
    scaled.set_scale(**slow)
    rng = np.random.default_rng(12)
    on_the_end = moved = 0
    for _ in range(24):
        a, r = rng.uniform(0, 2 * np.pi), rng.uniform(25.0, 60.0)
        px, py = 8.0 + r * math.cos(a), 5.0 + r * math.sin(a)
        seed = _rigid_seed(rigid, px, py, dur)
        _, t_r, _ = rigid.sdf_swept(px, py)
        f_s, t_s, _ = scaled.sdf_swept(px, py)
        assert abs(t_r - seed) < 0.01                               # the rigid descent stays at its seed's minimum
        tmin, tmax = max(0.0, seed - 3.4), min(seed + 3.4, dur)
        assert tmin <= t_s <= tmax, (px, py, seed, t_s)
        assert f_s > 0 and scaled.true_sdf(px, py)[1] == t_s       # an exterior point: the main solve is the answer
        moved += int(abs(t_s - t_r) > 1.0)
        if tmax < dur:
            assert t_s == tmax, (px, py, seed, t_s, tmax)           # seed + 3.4, to the bit
            assert scaled.sdf_at_time(px, py, dur) < f_s - 1e-3     # smaller still where the window does not reach
            on_the_end += 1
    assert moved >= 5, "rigid and scaled t* must differ"
    assert on_the_end >= 5, on_the_end
