"""The reference's useScale arithmetic restated in pure Python: shared by the tests of the scaled path.

tests/golden/make_golden.py's reference path (libm trig, no FMA, written from the reference sources) with S(t) put where
the reference's `useScale = true` puts it -- and nowhere else:
  * choiceTInit stays rigid (SWM:567-570 call the non-scale overloads);
  * gradientDescent evaluates getSDFAtTimeStamp<true> and getSDF_DOTAtTimeStamp<true>: u = (Rt^T S(t)^-1)(p - x(t)),
    S^-1 as Eigen's 3x3 inverse() forms it (cofactors times 1 / det), Rt^T S^-1 formed first (SWM:528-535, 799-806);
  * the exterior gradient is getonlyGrad1 at the scaled u at t* (SWM:779-797);
  * grad_cost_p_sw takes -(S(t*)^-1)^T R g for the position gradient, the rigid yaw term (BEO:1050, 1062).
Used by test_scale_restatement_gpu.py (the library against it) and test_oracle_scale.py (the C oracle against it).

The restatement is slow (pure Python, every GSIP sample a full solve); its points run in spawned worker processes.
"""
import concurrent.futures as cf
import ctypes
import ctypes.util
import importlib.util
import math
import multiprocessing as mp
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = dict(c=(0.8, 0.8), amp=(0.6, 0.4), omega=(1.5, 1.8), phase=(-1.0, 0.0))
HEAD = [[2.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]     # rows: pos, vel, acc (make_golden.main)
TAIL = [[14.0, 9.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
Q = [[5.0, 2.5, 0.4], [8.5, 6.0, -0.3], [11.0, 7.0, 0.5]]
T = [2.2, 2.6, 2.4, 2.1]
CASES = {   # shape -> (safety_hor, points)
    "star": (0.7, 48), "sdHorseshoe": (0.7, 48), "sdHeart": (0.8, 40), "Polygon": (0.7, 20),
}


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden_scaled", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _mg()

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None


def sincos(a):
    """(sin a, cos a) of the yaw rotation as the reference's g++ -O3 build computes them: Eigen's AngleAxis takes sin(angle)
    and cos(angle), which the compiler merges into ONE libm sincos() call -- and for about one argument in a thousand its
    results differ from sin() / cos() called alone in the last bit (the C oracle calls sincos() too).
    Under a schedule that bit moved the t* of a point on a flat stretch by 7e-10 and its gradient by 3e-8
    (tests/test_oracle_scale.py).  The schedule's own sine is a call of its own: math.sin."""
    sn, cs = ctypes.c_double(), ctypes.c_double()
    _libm.sincos(a, ctypes.byref(sn), ctypes.byref(cs))
    return sn.value, cs.value


def scale_inv(sc, t):
    """S(t)^-1 of diag(s_x, s_y, 1) as Eigen's inverse() forms it: cof0 = (s_y, 0, 0), det = s_y s_x, invdet = 1 / det,
    i00 = cof00 invdet, i11 = cofactor(1, 1) invdet = s_x invdet."""
    sx = sc["c"][0] + math.sin(sc["omega"][0] * t + sc["phase"][0]) * sc["amp"][0]
    sy = sc["c"][1] + math.sin(sc["omega"][1] * t + sc["phase"][1]) * sc["amp"][1]
    invdet = 1.0 / (sy * sx)
    return sy * invdet, sx * invdet


class ScaledSwept(mg.Swept):
    """SweptVolumeManager with useScale = true and getScale = the schedule `sc`."""

    def __init__(self, shape, traj, sc):
        super().__init__(shape, traj)
        self.sc = sc

    def _u(self, px, py, t):   # posEva2Rel(pos_eva, xt, Rt, St) (SWM:528-535)
        xt = self.traj.pos(t)
        s, c = sincos(xt[2])
        i00, i11 = scale_inv(self.sc, t)
        dx, dy = px - xt[0], py - xt[1]
        return (c * i00) * dx + (s * i11) * dy, ((-s) * i00) * dx + (c * i11) * dy

    def sdf_at_sc(self, px, py, t):   # getSDFAtTimeStamp<true>
        return self.shape.sdf(*self._u(px, py, t))

    def sdf_dot_sc(self, px, py, t):   # getSDF_DOTAtTimeStamp<true>: the finite difference (returns at SWM:806)
        t1 = max(0.0, t - 0.000001)
        t2 = min(self.dur, t + 0.000001)
        return (self.sdf_at_sc(px, py, t2) - self.sdf_at_sc(px, py, t1)) * 500000

    def gradient_descent(self, tmin, tmax, x0, px, py):   # SWM:1249-1325 with <useScale>
        alpha, tol = 0.01, 1e-16
        x, prev, it, stop, fx = x0, 10000000.0, 0, False, 0.0
        while it < 1000 and not stop and abs(x - prev) > tol:
            if it == 0:
                fx = self.sdf_at_sc(px, py, x)
            tau = alpha
            prev = x
            g = self.sdf_dot_sc(px, py, x)   # (re-evaluated per trial in the reference: x is fixed inside the ladder)
            for div in range(1, 30):
                it += 1
                change = -tau * (int(g > 0) - int(g < 0))
                xc = max(min(x + change, tmax), tmin)
                fc = self.sdf_at_sc(px, py, xc)
                if (fc - fx) < 0:
                    x, fx = xc, fc
                    break
                tau = 0.5 * tau
                if div == 29:
                    stop = True
        return fx, x

    def solve(self, px, py):   # getSDFofSweptVolume<false, true> with <useScale>: rigid seed, scaled descent and gradient
        self.n_solves += 1
        ts = self.choice_t_init(px, py, 0.15)   # rigid (SWM:567-570)
        tmin, tmax = max(0.0, ts - 3.4), min(ts + 3.4, self.dur)
        f, t = self.gradient_descent(tmin, tmax, ts, px, py)
        g = self.shape.grad(*self._u(px, py, t))   # getGradPrelAtTimeStamp<true> (SWM:779-797)
        return f, t, (g[0], g[1])


def penalty_sc(sw, rows, durs, points, safety_hor, weight_p, per_point=None):
    """make_golden.penalty with grad_cost_p_sw's St = S(t*) (BEO:827-834, 1050); per_point: precomputed true_sdf results."""
    N = len(durs)
    cost, gradT = 0.0, [0.0] * N
    gradC = [[0.0, 0.0, 0.0] for _ in range(6 * N)]
    per = []
    for k, p in enumerate(points):
        px, py = p[0], p[1]
        sdf, tstar, g = per_point[k] if per_point is not None else sw.true_sdf(px, py)
        per.append([sdf, tstar, g[0], g[1]])
        i, s1 = sw.traj.locate(tstar)
        s2 = s1 * s1; s3 = s2 * s1; s4 = s2 * s2; s5 = s4 * s1
        b0 = [1.0, s1, s2, s3, s4, s5]
        b1 = [0.0, 1.0, 2.0 * s1, 3.0 * s2, 4.0 * s3, 5.0 * s4]
        pos = [sum(rows[6 * i + k2][d] * b0[k2] for k2 in range(6)) for d in range(3)]
        vel = [sum(rows[6 * i + k2][d] * b1[k2] for k2 in range(6)) for d in range(3)]
        yaw = pos[2]
        sy, cy = sincos(yaw)
        gr = [g[0], g[1]]
        if sdf < 0:  # BEO:832
            gr = [cy * g[0] + sy * g[1], (-sy) * g[0] + cy * g[1]]
        ok, L, dL = mg.smoothed_l1(safety_hor - sdf, 0.01)
        gx = gy = gyaw = pena = 0.0
        if ok and L > 0:
            i00, i11 = scale_inv(sw.sc, tstar)   # St = getScale(time_seed_f), time_seed_f = t* (BEO:795, 827)
            sgx = -dL * (((-i00) * cy) * gr[0] + ((-i00) * (-sy)) * gr[1])
            sgy = -dL * (((-i11) * sy) * gr[0] + ((-i11) * cy) * gr[1])
            dx, dy = px - pos[0], py - pos[1]
            v0 = (-sy) * dx + cy * dy
            v1 = (-cy) * dx + (-sy) * dy
            gyv = (-dL * gr[0]) * v0 + (-dL * gr[1]) * v1   # the rigid yaw term (BEO:1062)
            gx, gy, gyaw, pena = weight_p * sgx, weight_p * sgy, weight_p * gyv, weight_p * L
        cost += pena
        for k2 in range(6):
            gradC[6 * i + k2][0] += b0[k2] * gx
            gradC[6 * i + k2][1] += b0[k2] * gy
            gradC[6 * i + k2][2] += b0[k2] * gyaw
        gdT = -((gx * vel[0] + gy * vel[1]) + gyaw * vel[2])
        for j in range(i):
            gradT[j] += gdT
    return cost, gradT, gradC, per


def _x():
    tau = [(math.sqrt(2.0 * t - 1.0) - 1.0) if t > 1.0 else (1.0 - math.sqrt(2.0 / t - 1.0)) for t in T]   # BEO:228-241
    return tau + [v for w in Q for v in w]


def _true_sdf_chunk(args):
    """worker (spawned process): true_sdf of some points under the schedule"""
    shape, verts, rows, durs, sc, pts = args
    sw = ScaledSwept(mg.Shape(shape, (0.0, 0.0, 0.0), verts), mg.Traj(rows, durs), sc)
    # (with the main solve's value: <= 0 is an interior point, whose GSIP result may end either side of 0)
    return [(sw.true_sdf(p[0], p[1]), sw.solve(p[0], p[1])[0]) for p in pts]


def restated_cost_function(shape, verts, points, safety_hor, sc, x):
    """make_golden.cost_function under the schedule; the points' true_sdf run in parallel first, then the serial sums."""
    N = len(T)
    tau = x[:N]
    Tv = [((0.5 * t + 1.0) * t + 1.0) if t > 0.0 else 1.0 / ((0.5 * t - 1.0) * t + 1.0) for t in tau]
    q = [x[N + 3 * i:N + 3 * i + 3] for i in range(N - 1)]
    rows, _, _ = mg.minco(HEAD, TAIL, q, Tv)
    nw = max(1, min(15, (os.cpu_count() or 2) - 1))
    chunks = [points[k::nw] for k in range(nw)]
    with cf.ProcessPoolExecutor(max_workers=nw, mp_context=mp.get_context("spawn")) as ex:
        res = list(ex.map(_true_sdf_chunk, [(shape, verts, rows, Tv, sc, c) for c in chunks]))
    per_point, main_f = [None] * len(points), [None] * len(points)
    for k in range(nw):
        for j, (r, f0) in enumerate(res[k]):
            per_point[k + j * nw], main_f[k + j * nw] = r, f0
    saved = mg.penalty
    mg.penalty = lambda sw, rows_, durs, pts, sh, wp: penalty_sc(sw, rows_, durs, pts, sh, wp, per_point)
    try:
        # (cost_function builds a rigid Swept for its penalty; penalty_sc only reads its trajectory and our per-point results)
        orig = mg.Swept
        mg.Swept = lambda shape_, traj: ScaledSwept(shape_, traj, sc)
        try:
            return mg.cost_function(shape, (0.0, 0.0, 0.0), verts, HEAD, TAIL, x, [[p[0], p[1], 0.0] for p in points],
                                    safety_hor, 60.0, 3.8) + (main_f,)
        finally:
            mg.Swept = orig
    finally:
        mg.penalty = saved


def _points(shape, n, seed):
    """points around the path, about a third of them inside the swept volume"""
    rows, _, _ = mg.minco(HEAD, TAIL, Q, T)
    tr = mg.Traj(rows, T)
    rng = np.random.default_rng(seed)
    R = {"star": 2.8, "sdHorseshoe": 2.3, "sdHeart": 4.3, "Polygon": 2.9}[shape]
    out = []
    for t, a, r in zip(rng.uniform(0, sum(T), n), rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.7, n))):
        p = tr.pos(float(t))
        out.append((p[0] + float(r) * math.cos(float(a)), p[1] + float(r) * math.sin(float(a))))
    return out
