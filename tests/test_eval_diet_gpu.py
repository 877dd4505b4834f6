"""The trimmed SDF evaluation (square roots without range scaling) on the operands random clouds rarely produce.

Per point bit identity against the oracle in device-arithmetic mode (orc set_modes(1, 0)), the comparison
tests/test_kernel_instantiations_gpu.py makes, on clouds built for the new code's edges:
  a. points exactly on the trajectory's position at table times (multiples of the scan step 0.15 s, summed as the scan sums
     them), at t = 0 and at t = dur, many copies of each: the body-frame point is (0, 0) or within an ulp of it, so the
     shape's |q| and the chunk / anchor distances have zero and tiny radicands (the helpers' guarded path), and points a
     few ulp to 1e-160 m away from them (radicands below 2^-767);
  b. points beyond both ends of the path, behind the start and past the goal: t* clamps to 0 and to dur;
  c. the same clouds under coarse (1.5 s: single-subtraction piece time) and generic durations (the reference's chain);
  d. the launch chain and the fused tail, and 2 / 8 / 32 lanes per query: every plan the same bits;
  e. all 17 shapes once on 2 500 random points.
star, sdHorseshoe (the only formula whose closing root is zero for every interior point), sdHeart and sdTunnel at 8 and 16
pieces, about 2 000 points a cloud.

The inputs are checked on the CPU first: the oracle of record (libm trig) and the device-trig oracle must agree on every
point of every cloud -- the same basin (|t*| within 1e-4 s) and the same value (1e-9 m) -- so that a mismatch between the
library and the device-trig oracle can only be the kernels'.  No point is excluded from any comparison.
"""
import os

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)

SHAPES = ["sdUnevenCapsule", "sdCutDisk", "sdTrapezoid", "sdRhombus", "star", "sdTunnel", "sdHorseshoe", "sdHeart",
          "sdOrientedVesica", "sdRoundedCross", "sdRoundedX", "bigX", "sdMoon", "sdPie", "sdPie2", "sdArc", "Polygon"]
# circumradius of each shape about its origin, to size the clouds (the constants of the shapes' formulas)
RADIUS = {"sdUnevenCapsule": 6.0, "sdCutDisk": 5.0, "sdTrapezoid": 3.61, "sdRhombus": 4.5, "star": 2.8, "sdTunnel": 2.92,
          "sdHorseshoe": 2.3, "sdHeart": 4.58, "sdOrientedVesica": 4.47, "sdRoundedCross": 2.0, "sdRoundedX": 2.37, "bigX": 3.79,
          "sdMoon": 3.0, "sdPie": 3.0, "sdPie2": 3.0, "sdArc": 2.83, "Polygon": 1.6}
OUTLINE = np.array([[1.6, 0.0], [0.7, 1.1], [-0.5, 1.3], [-1.4, 0.2], [-0.9, -1.1], [0.8, -1.2]])
EDGE_SHAPES = ["star", "sdHorseshoe", "sdHeart", "sdTunnel"]
# The clouds' seed: chosen on the CPU, from the two oracles alone, so that they agree on every point of all 16 edge clouds
# (with 500 three points of the sdTunnel / 16 coarse pieces cloud sit on a flat stretch of SDF(t) and change basin with the trig).
CLOUD_SEED = 520
PLANS = [("chain", dict(tail_iter=-2)), ("fused tail", dict(tail_iter=0)), ("lanes 2", dict(lanes_per_query=2)),
         ("lanes 8", dict(lanes_per_query=8)), ("lanes 32", dict(lanes_per_query=32))]


def _traj(N, generic, seed):
    import svsdf_amd
    rng = np.random.default_rng(seed)
    T = np.full(N, 1.5) * (rng.uniform(0.9, 1.1, N) if generic else 1.0)
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:, 0] = [0.0, 0.0, 0.3]
    x = 2.5 * np.arange(1, N + 1)
    y = 2.0 * np.sin(0.45 * np.arange(1, N + 1)) + rng.uniform(-0.4, 0.4, N)
    yaw = 0.5 * np.cos(0.6 * np.arange(1, N + 1)) + rng.uniform(-0.2, 0.2, N)
    q = np.stack([x, y, yaw], axis=1)
    ts[:, 0] = q[-1]
    return svsdf_amd.minco_coeffs(hs, ts, q[:-1], T), T, hs, ts


def _edge_cloud(o, T, R, seed):
    """(a) + (b) + random filler, ~2 000 points."""
    rng = np.random.default_rng(seed)
    dur = o.duration()                           # (the trajectory's own sum of the durations: t* clamps to this number)
    times, t = [0.0, dur], 0.0
    while t + 0.15 <= dur:                       # the scan's own sum: t += 0.15
        t += 0.15
        times.append(t)
    times = [times[0], times[1]] + list(rng.choice(times[2:], 28, replace=False))
    on = np.array([o.pos(t)[:2] for t in times])
    parts = [np.repeat(on, 8, axis=0)]                                                # exactly on the path, 8 copies each
    for eps in (1e-160, 1e-120, 1e-16, 4e-16, 1e-12):                                 # tiny and sub-2^-767 radicands
        ang = rng.uniform(0, 2 * np.pi, len(on))
        parts.append(on + eps * np.stack([np.cos(ang), np.sin(ang)], axis=1))
    p0, p1 = o.pos(0.0), o.pos(dur)
    for p, sgn in ((p0, -1.0), (p1, 1.0)):                                            # (b) beyond both ends, along the heading
        d = rng.uniform(0.2, 2.5 * R, 250)
        side = rng.uniform(-0.8 * R, 0.8 * R, 250)
        c, s = np.cos(p[2]), np.sin(p[2])
        parts.append(np.stack([p[0] + sgn * d * c - side * s, p[1] + sgn * d * s + side * c], axis=1))
    n = 2000 - sum(len(a) for a in parts)
    tt = rng.uniform(0.0, dur, n)
    pos = np.array([o.pos(t)[:2] for t in tt])
    ang, rad = rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.6, n))
    parts.append(pos + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1))
    xy = np.concatenate(parts)
    pts = np.zeros((len(xy), 3))
    pts[:, :2] = xy
    return pts[rng.permutation(len(pts))]


def _oracles_agree(o, pts, what):
    """CPU: the oracle of record against the device-trig oracle, every point.  Returns the device-trig results."""
    o.set_modes(0, 0)
    _, _, _, sdf0, ts0, _ = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
    o.set_modes(1, 0)
    ref = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
    bad = (np.abs(ts0 - ref[4]) > 1e-4) | (np.abs(sdf0 - ref[3]) > 1e-9)
    assert not bad.any(), (what, "the two oracles disagree on points", np.nonzero(bad)[0][:10])
    return ref + (o.query(pts, nthreads=NT)[2],)


def _rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _check(shape, kw, coeffs, T, pts, ref, plans, what, exact):
    import svsdf_amd
    ocost, ogT, ogC, osdf, ots, _, og = ref
    c = svsdf_amd.SvsdfContext(shape=shape, device=0, **kw)
    c.set_points(pts)
    first = None
    for label, plan in plans:
        c.set_plan(**plan)
        pens = [c.eval_penalty(coeffs, T) for _ in range(2)]
        assert (c.stats()["piece_time_exact"] != 0) == exact, (what, label)
        sdf, ts, g, _ = c.query_points(coeffs, T)
        w = what + (label,)
        assert np.array_equal(sdf, osdf), (w, "sdf", int((sdf != osdf).sum()))
        assert np.array_equal(ts, ots), (w, "t*", int((ts != ots).sum()))
        assert np.array_equal(g, og), (w, "gradient", int((g != og).any(axis=1).sum()))
        for cost, gT, gC in pens:
            assert abs(cost - ocost) <= 1e-12 * abs(ocost), (w, cost, ocost)
            assert _rel(gT, ogT) <= 1e-12 and _rel(gC, ogC) <= 1e-12, (w, _rel(gT, ogT), _rel(gC, ogC))
            if first is None:
                first = (cost, gT, gC)
            assert cost == first[0] and np.array_equal(gT, first[1]) and np.array_equal(gC, first[2]), (w, "plans differ")
    c.close()
    return osdf, ots


@pytest.mark.parametrize("generic", [False, True], ids=["coarse", "generic"])
@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_clouds_bit_for_bit(built, shape, N, generic):
    coeffs, T, hs, ts = _traj(N, generic, 100 + N)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, head_state=hs, tail_state=ts)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    R = RADIUS[shape]
    what = (shape, N, "generic" if generic else "coarse")
    pts = _edge_cloud(o, T, R, CLOUD_SEED + N + 7 * EDGE_SHAPES.index(shape))
    ref = _oracles_agree(o, pts, what)
    osdf, ots = _check(shape, kw, coeffs, T, pts, ref, PLANS, what, generic)
    dur = o.duration()
    n0, n1, n1x = int((ots == 0.0).sum()), int((ots >= dur - 1e-4).sum()), int((ots == dur).sum())
    print(f"{what}: {len(pts)} points, interior {int((osdf <= 0).sum())}, t* == 0: {n0}, t* within 1e-4 of dur: {n1} (== dur: {n1x})")
    # (the end: under generic durations the reference's descent stops one ladder step, 0.01 * 2^-10 s, short of dur for most
    # of these points -- the candidates clamped to dur are evaluated and not accepted)
    assert n0 >= 50 and n1 >= 50, (what, "the cloud must drive t* to both ends", n0, n1)
    assert (osdf <= 0).sum() >= 100, what


@pytest.mark.parametrize("sid", list(range(17)))
def test_all_shapes_random_cloud(built, sid):
    shape = SHAPES[sid]
    coeffs, T, hs, ts = _traj(8, True, 300 + sid)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, head_state=hs, tail_state=ts,
              polygon=OUTLINE if shape == "Polygon" else None)
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    R = RADIUS[shape]
    rng = np.random.default_rng(900 + sid)
    n = 2500
    tt = rng.uniform(0.0, T.sum(), n)
    pos = np.array([o.pos(t)[:2] for t in tt])
    ang, rad = rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.6, n))
    pts = np.zeros((n, 3))
    pts[:, :2] = pos + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    ref = _oracles_agree(o, pts, (shape,))
    _check(shape, kw, coeffs, T, pts, ref, [("default", {})], (shape,), True)
