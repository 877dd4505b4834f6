"""The device at the inputs where shape formulas break.

test_gpu_sdf_at.py draws its query points from a normal distribution; the shape code never sees the origin, signed zeros,
points on a symmetry axis or on a branch surface, a point where an inner sqrt operand is exactly 0 or denormal (the slow
path of sqrt_nz / sqrt_z, chosen per wave), points on the zero set, or points 1e9 m away.  Here it does:
debug_sdf_at on a rest trajectory (one piece, zero boundary states: the body-frame point is the query point and the value
is the raw shape function as k_solve inlines it) over shape_restatement.edge_set -- features(shape) with their ulp
neighbours, signed zeros and both axes, 200 traced zero-set points with their neighbours, radii 1e3 / 1e6 / 1e9 m,
coordinates of 1e-300 and 5e-324, 1 000 generic points -- for the sixteen analytic shapes at three poses, and Polygon
(workload.star_outline()) on its own vertices and edge midpoints.

Each set is evaluated in two layouts: grouped (the edge points in waves of their own, padded to whole waves) and shuffled
among the generic points -- a mixed wave takes another sqrt path than a pure one.  Expected: d[:, 0] bit-identical to the
oracle in device-arithmetic mode (set_modes(1, 0)), every point, both layouts, and within 1e-13 max(1, |x|, |y|) of
FLOAT mode of the second reading (the gate of test_shape_restatement.py).  No finite input of the set makes a NaN in the
oracle (asserted here and, on the CPU, in test_shape_restatement.py::test_oracle_at_edge_inputs), so there is no NaN point
to pin.

What it found: on 11 of 150 queries on the star outline's own edges the device had the other sign of a +-1e-16 value than
the oracle's device-arithmetic mode, which had left Polygon's isCrossRayOnXDir (SHP:1370-1383) on libm's atan2 while the
kernels' slow path calls the device library's; the mode now takes the device algorithm there as well (oracle/svsdf_oracle.c,
pinned on the CPU by test_shape_restatement.py::test_polygon_device_mode_takes_the_device_atan2).

test_edge_inputs_through_the_hot_path runs k_solve / k_round / k_tail on them: the features, zero-set points and axes of
each shape translated onto the first waypoint (yaw 0) of a 3-piece trajectory with generic durations, mixed with corridor
points, about 600 points per shape at the pinned pose: per-point sdf, t* and gradient bit-identical to the oracle in
device-arithmetic mode, cost and gradients to 1e-12 (the gate of test_differential_fuzz_bit_identical_in_device_arithmetic_mode).
The radii >= 1e6 m and the denormal coordinates stay with debug_sdf_at: a translation rounds them away.
"""
import importlib.util
import os

import numpy as np
import pytest

import shape_restatement as sr
from oracle import orc

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)
POSES = sr.poses()
REST = (np.zeros((6, 3)), np.array([1.0]))
_Z = {}


def _zero_pts(name):
    if name not in _Z:
        _Z[name] = sr.trace_zero_set(orc.Oracle(name).shape_eval)      # sample sites only (checked in test_shape_geometry.py)
    return _Z[name]


def _bits_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _layouts(edge, generic, rng):
    """(label, points) of the grouped and of the shuffled layout."""
    pad = (-len(edge)) % 64
    grouped = np.concatenate([edge, edge[:pad], generic])
    mixed = np.concatenate([edge, generic])
    perm = rng.permutation(len(mixed))
    return [("grouped", grouped), ("shuffled", mixed[perm])]


def _check_device(ctx, o, xy, float_f, tag):
    d = ctx.debug_sdf_at(REST[0], REST[1], xy, np.zeros(len(xy)))
    ref = np.array([o.sdf_at_time(float(x), float(y), 0.0) for x, y in xy])
    assert np.isfinite(ref).all(), (tag, xy[~np.isfinite(ref)][:3])
    bad = np.nonzero(~_bits_equal(d[:, 0], ref))[0]
    assert len(bad) == 0, (tag, len(bad), xy[bad[:3]], d[bad[:3], 0], ref[bad[:3]])
    fl = np.array([float_f(float(x), float(y)) for x, y in xy])
    err = np.abs(d[:, 0] - fl) / np.maximum(1.0, np.abs(xy).max(axis=1))
    k = int(err.argmax())
    assert err.max() <= 1e-13, (tag, xy[k], d[k, 0], fl[k])


@pytest.mark.parametrize("ipose", range(len(POSES)))
@pytest.mark.parametrize("name", sr.ANALYTIC)
def test_edge_inputs_bit_identical(built, name, ipose):
    import svsdf_amd
    pp = POSES[ipose]
    edge, generic = sr.edge_set(name, pp, _zero_pts(name), 9000 + ipose)
    assert len(edge) + len(generic) <= 3200
    ctx = svsdf_amd.SvsdfContext(shape=name, device=0, poly_params=pp)
    o = orc.Oracle(name, poly_params=pp)
    o.set_traj(*REST)
    o.set_modes(1, 0)
    sh = sr.Shape(name, pp)
    rng = np.random.default_rng(77 + ipose)
    for label, xy in _layouts(edge, generic, rng):
        _check_device(ctx, o, xy, sh.at_rest, (name, pp, label))
    ctx.close()


def test_polygon_on_its_own_vertices_and_edges(built):
    import svsdf_amd
    from svsdf_amd import workload
    poly = workload.star_outline()
    nxt = np.roll(poly, -1, axis=0)
    own = np.concatenate([poly, 0.5 * (poly + nxt), poly + 0.25 * (nxt - poly)])
    far = sr.edge_set("star", (0.0, 0.0, 0.0), np.zeros((0, 2)), 5)[0][-(52 + 48):]     # the radii and the tiny coordinates
    edge = np.concatenate([sr.ulp_neighbours(own), sr.signed_zeros_and_axes(), far])
    rng = np.random.default_rng(78)
    generic = rng.normal(0.0, 3.0, (1000, 2))
    spec = importlib.util.spec_from_file_location("make_golden_poly", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    old = mg.Shape("Polygon", verts=[tuple(v) for v in poly.tolist()])
    ctx = svsdf_amd.SvsdfContext(shape="Polygon", device=0, polygon=poly)
    o = orc.Oracle("Polygon", polygon=poly)
    o.set_traj(*REST)
    o.set_modes(1, 0)
    for label, xy in _layouts(edge, generic, rng):
        _check_device(ctx, o, xy, lambda x, y: old.sdf(1.0 * x + 0.0 * y, (-0.0) * x + 1.0 * y), ("Polygon", label))
    ctx.close()


@pytest.mark.parametrize("name", sr.ANALYTIC)
def test_edge_inputs_through_the_hot_path(built, name):
    import svsdf_amd
    pp = sr.PINNED_POSE
    rng = np.random.default_rng(300 + sr.ANALYTIC.index(name))
    N = 3
    T = rng.uniform(0.8, 2.5, N)
    hs = np.zeros((3, 3)); ts = np.zeros((3, 3))
    hs[:2, 0] = (2.0, 1.0); ts[:2, 0] = (11.0, 7.0)
    hs[2, 0] = 0.4; ts[2, 0] = -0.6
    q = np.array([[5.0, 2.5, 0.0], [8.5, 6.0, 0.7]])         # first waypoint: yaw 0, the body frame is a translation there
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    Z = _zero_pts(name)
    Z = Z[rng.choice(len(Z), 60, replace=False)]
    body = np.concatenate([sr.ulp_neighbours(sr.to_world(pp, sr.features(name))), sr.to_world(pp, Z),
                           sr.to_world(pp, sr.signed_zeros_and_axes())])
    if len(body) > 400:
        body = body[rng.choice(len(body), 400, replace=False)]
    anchors = np.vstack([hs[:2, 0], q[:, :2], ts[:2, 0]])
    corridor = anchors[rng.integers(0, len(anchors), 200)] + rng.normal(0, 2.5, (200, 2))
    pts = np.zeros((len(body) + 200, 3))
    pts[:, :2] = np.concatenate([body + q[0, :2], corridor])
    pts = pts[rng.permutation(len(pts))]
    kw = dict(safety_hor=0.7, weight_p=60.0, rho=3.8, poly_params=pp, head_state=hs, tail_state=ts)
    ctx = svsdf_amd.SvsdfContext(shape=name, device=0, **kw)
    ctx.set_points(pts)
    cost, gT, gC = ctx.eval_penalty(coeffs, T)
    sdf, tstar, g, _ = ctx.query_points(coeffs, T)
    o = orc.Oracle(name, **kw)
    o.set_traj(coeffs, T)
    o.set_modes(1, 0)
    ocost, ogT, ogC, osdf, ots, _ = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
    og = o.query(pts, nthreads=NT)[2]
    bad = np.nonzero(~(_bits_equal(sdf, osdf) & _bits_equal(tstar, ots) & _bits_equal(g, og).all(axis=1)))[0]
    print(f"{name}: {len(pts)} points, {int((osdf <= 0).sum())} interior, {len(bad)} per-point mismatches")
    assert len(bad) == 0, (name, len(bad), pts[bad[:3]], sdf[bad[:3]], osdf[bad[:3]], tstar[bad[:3]], ots[bad[:3]])
    rel = lambda a, b: float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))
    assert ocost > 0.0 and abs(cost - ocost) <= 1e-12 * abs(ocost), (cost, ocost)
    assert rel(gC, ogC) <= 1e-12 and rel(gT, ogT) <= 1e-12, (rel(gC, ogC), rel(gT, ogT))
    ctx.close()
