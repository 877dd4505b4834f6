"""Every shipped hot-path kernel instantiation, bit for bit against the oracle in device-arithmetic mode.

One case per compiled shape id (0 ... 16, and 17 = the Polygon with its edges in LDS; id 16 runs the Polygon with its edges
in global memory, SVSDF_POLY_LDS=0).  Each case builds one trajectory with generic piece durations (the reference's chain
of subtractions locates the piece) and three clouds sized from the device's CU count:
  R  ~ 150 points: solo k_solve, k_tail<., ., 2> (a wave slot per point), both half-waves on a point, one-block reduce;
  M  the tail's point count in (8, 12] points per CU: k_tail<., ., 3> with one point per wave;
  L  above 12 points per CU: k_tail<., ., 3> with two points per wave.
Each cloud's oracle runs once (orc set_modes(1, 0): the device library's trig, the reference's piece location); every
configuration of the launch plan (bound mode x tail start, lanes per query) and of the switches read at context creation
must then reproduce the oracle's per-point SVSDF, t* and gradient bit for bit, its cost and gradients to 1e-12, and the
same cost / gradient bits as every other configuration of the cloud.  Which instantiation ran is read from the launch
record (svsdf_last_launches), never inferred from the size rules; each case ends by checking that the union of its records
holds every instantiation of its shape id.
"""
import os

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)

SHAPES = ["sdUnevenCapsule", "sdCutDisk", "sdTrapezoid", "sdRhombus", "star", "sdTunnel", "sdHorseshoe", "sdHeart",
          "sdOrientedVesica", "sdRoundedCross", "sdRoundedX", "bigX", "sdMoon", "sdPie", "sdPie2", "sdArc", "Polygon"]
OFFSETS = {"sdCutDisk": (0.0, -0.6, 0.0), "sdHeart": (0.3, -0.4, 25.0), "sdArc": (-0.4, 0.5, -140.0),
           "star": (0.5, 0.2, 10.0), "sdTrapezoid": (0.2, 0.1, 70.0)}
OUTLINE = np.array([[1.6, 0.0], [0.7, 1.1], [-0.5, 1.3], [-1.4, 0.2], [-0.9, -1.1], [0.8, -1.2]])   # cheap 6-vertex outline
WIDTHS = (1, 2, 4, 8, 16, 32)
PLANS = [(bm, ti) for bm in range(4) for ti in (0, 2, -2)]


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _setup(sid):
    import svsdf_amd
    shape = SHAPES[min(sid, 16)]
    rng = np.random.default_rng(7100 + sid)
    T = np.array([1.3, 2.2, 0.9, 1.7]) * rng.uniform(0.9, 1.1, 4)     # generic durations: the chained piece location
    hs, ts = np.zeros((3, 3)), np.zeros((3, 3))
    hs[:, 0] = [0.0, 0.0, 0.4]
    ts[:, 0] = [14.0, 5.0, -1.2]
    q = np.array([[4.0, 3.0, 1.1], [8.0, 1.5, -0.6], [11.0, 4.5, 0.8]]) + rng.uniform(-0.5, 0.5, (3, 3))
    coeffs = svsdf_amd.minco_coeffs(hs, ts, q, T)
    kw = dict(safety_hor=0.6, weight_p=60.0, rho=3.8, poly_params=OFFSETS.get(shape, (0.0, 0.0, 0.0)),
              polygon=OUTLINE if shape == "Polygon" else None, head_state=hs, tail_state=ts)
    env = {"SVSDF_POLY_LDS": 0} if sid == 16 else {}
    return shape, kw, coeffs, T, env


def _clouds(shape, kw, coeffs, T, env, n_cu):
    """R, M, L clouds: interior points (inside the swept volume) and exterior ones drawn around the trajectory; which is
    which is read from one plain evaluation of a larger pool."""
    import svsdf_amd
    o = orc.Oracle(shape, **kw)
    o.set_traj(coeffs, T)
    rng = np.random.default_rng(11 + SHAPES.index(shape))
    c = _with_env(env, lambda: svsdf_amd.SvsdfContext(shape=shape, device=0, **kw))
    R = c.shape_bound()[0]
    want = {"R": (90, 60), "M": (int(0.8 * 10 * n_cu) - 51, 600), "L": (int(0.8 * 16 * n_cu), 900)}
    need_in = sum(v[0] for v in want.values())
    inner, outer = np.zeros((0, 3)), np.zeros((0, 3))
    for _ in range(20):
        n = 8000
        tt = rng.uniform(0.0, T.sum(), n)
        pos = np.array([o.pos(t)[:2] for t in tt])
        ang, rad = rng.uniform(0, 2 * np.pi, n), R * np.sqrt(rng.uniform(0, 1.6, n))
        pts = np.zeros((n, 3))
        pts[:, 0] = pos[:, 0] + rad * np.cos(ang)
        pts[:, 1] = pos[:, 1] + rad * np.sin(ang)
        c.set_points(pts)
        sdf = c.query_points(coeffs, T)[0]
        inner = np.concatenate([inner, pts[sdf <= 0]])
        outer = np.concatenate([outer, pts[sdf > 0]])
        if len(inner) >= need_in and len(outer) >= 1600:
            break
    c.close()
    assert len(inner) >= need_in and len(outer) >= 1600, (shape, len(inner), len(outer))
    out, i0, e0 = {}, 0, 0
    for k, (ni, ne) in want.items():
        pts = np.concatenate([inner[i0:i0 + ni], outer[e0:e0 + ne]])
        out[k] = pts[rng.permutation(len(pts))]
        i0 += ni
        e0 += ne
    return o, out


def _configs(cls):
    """(label, env read at context creation, plan) of one cloud class."""
    cfg = [(f"mode {bm} tail {ti}", {}, dict(bound_mode=bm, tail_iter=ti)) for bm, ti in PLANS]
    cfg.append(("SVSDF_SCAN_ANCHORS=0", {"SVSDF_SCAN_ANCHORS": 0}, dict(bound_mode=3, tail_iter=0)))
    cfg.append(("SVSDF_TAIL_LOCAL=0", {"SVSDF_TAIL_LOCAL": 0}, dict(bound_mode=3, tail_iter=0)))
    if cls == "R":
        cfg += [(f"lanes {g}", {}, dict(lanes_per_query=g, tail_iter=-2)) for g in WIDTHS]
        cfg += [("default", {}, {}),
                ("SVSDF_TAIL_DUO=0", {"SVSDF_TAIL_DUO": 0}, dict(bound_mode=1, tail_iter=0)),
                ("SVSDF_TAIL_LATENCY=0", {"SVSDF_TAIL_LATENCY": 0}, dict(bound_mode=3, tail_iter=0)),
                ("SVSDF_G=32", {"SVSDF_G": 32}, {}),          # (no plan: svsdf_set_plan would reset the width to its rule)
                ("SVSDF_ASSUME_NOT_LIPSCHITZ=1", {"SVSDF_ASSUME_NOT_LIPSCHITZ": 1}, dict(bound_mode=3, tail_iter=0))]
    if cls == "L":
        cfg += [("SVSDF_ROUND_BPC=1", {"SVSDF_ROUND_BPC": 1}, dict(bound_mode=3, tail_iter=-2)),
                ("SVSDF_ROUND_BPC=16", {"SVSDF_ROUND_BPC": 16}, dict(bound_mode=1, tail_iter=-2))]
    return cfg


def _key(r):
    k = r["kernel"]
    if k == "solve":
        return ("solve", r["shape"], r["targ"][0]) + (("solo",) if r["solo"] else ())
    if k == "round":
        return ("round", r["shape"], r["targ"][0], r["targ"][1])
    if k == "tail":
        return ("tail", r["shape"], r["targ"][0], r["targ"][1], r["points_per_wave"])
    if k == "classify":
        return ("classify", r["shape"])
    return (k,)


def _required(sid):
    req = {("solve", sid, g) for g in WIDTHS} | {("solve", sid, 32, "solo")}
    req |= {("round", sid, lp, m) for lp in (8, 32) for m in range(4)}
    req |= {("tail", sid, m, w, ppw) for m in range(4) for (w, ppw) in ((2, 1), (3, 1), (3, 2))}
    req.add(("classify", min(sid, 16)))
    return req


def _rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("sid", list(range(18)))
def test_every_instantiation_matches_the_device_arithmetic_oracle(built, sid):
    import svsdf_amd
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    shape, kw, coeffs, T, env0 = _setup(sid)
    o, clouds = _clouds(shape, kw, coeffs, T, env0, n_cu)
    o.set_modes(1, 0)                     # the device library's sin / cos / atan2; the reference's piece location
    covered = set()
    for cls, pts in clouds.items():
        ocost, ogT, ogC, osdf, ots, _ = o.penalty(pts, nthreads=NT, sum_mode=1, per_point=True)
        sub = np.arange(len(pts)) if len(pts) <= 4000 else np.random.default_rng(sid).choice(len(pts), 3000, replace=False)
        og = o.query(pts[sub], nthreads=NT)[2]
        first = None
        for label, env, plan in _configs(cls):
            what = (shape, sid, cls, label)

            def make():
                c = svsdf_amd.SvsdfContext(shape=shape, device=0, **kw)
                c.set_points(pts)
                if plan:
                    c.set_plan(**plan)
                return c
            c = _with_env(dict(env0, **env), make)
            recs = []
            pens = []
            for _ in range(2):            # the second evaluation sizes its grids from the first one's counts
                pens.append(c.eval_penalty(coeffs, T))
                recs.append(c.last_launches())
            st = c.stats()
            sdf, ts, g, _ = c.query_points(coeffs, T)
            recs.append(c.last_launches())
            c.close()
            assert st["piece_time_exact"] != 0, what
            for rr in recs:
                covered |= {_key(r) for r in rr}
            # per point: bit for bit
            assert np.array_equal(sdf, osdf), (what, int((sdf != osdf).sum()))
            assert np.array_equal(ts, ots), (what, int((ts != ots).sum()))
            assert np.array_equal(g[sub], og), (what, int((g[sub] != og).any(axis=1).sum()))
            # reduced: the oracle to summation order, every configuration the same bits
            for cost, gT, gC in pens:
                assert abs(cost - ocost) <= 1e-12 * abs(ocost), (what, cost, ocost)
                assert _rel(gT, ogT) <= 1e-12 and _rel(gC, ogC) <= 1e-12, (what, _rel(gT, ogT), _rel(gC, ogC))
            if first is None:
                first = pens[0]
            for cost, gT, gC in pens:
                assert cost == first[0] and np.array_equal(gT, first[1]) and np.array_equal(gC, first[2]), what
            # the launch record shows what the class and the configuration are for
            second = recs[1]
            tails = [r for r in second if r["kernel"] == "tail"]
            if plan.get("tail_iter") == 0:
                assert tails, what
                for r in tails:
                    if cls == "R":
                        want = (1, 3 if env.get("SVSDF_TAIL_LATENCY") == 0 else 2, 0 if env.get("SVSDF_TAIL_DUO") == 0 else 1)
                        assert (r["points_per_wave"], r["targ"][1], r["duo"]) == want, (what, r)
                    else:
                        assert (r["points_per_wave"], r["targ"][1]) == ((1, 3) if cls == "M" else (2, 3)), (what, r)
                    assert r["local_state"] == (0 if env.get("SVSDF_TAIL_LOCAL") == 0 else 1), (what, r)
            if plan.get("tail_iter") == -2:
                assert not tails and any(r["kernel"] == "round" for r in second), what
            if "bound_mode" in plan:
                mode = 1 if (env.get("SVSDF_ASSUME_NOT_LIPSCHITZ") and plan["bound_mode"] == 3) else plan["bound_mode"]
                assert st["gsip_bound_mode"] == mode, (what, st["gsip_bound_mode"])
                assert all(r["targ"][0 if r["kernel"] == "tail" else 1] == mode for r in second
                           if r["kernel"] in ("tail", "round")), what
                if mode == 3:
                    anchors = 0 if env.get("SVSDF_SCAN_ANCHORS") == 0 else 1
                    assert all(r["anchors"] == anchors for r in second if r["kernel"] in ("tail", "round")), what
            if cls == "R":
                main = [r for r in second if r["kernel"] == "solve" and r["iter"] == 0]
                assert len(main) == 1, what
                pinned = "lanes_per_query" in plan or "SVSDF_G" in env     # a pinned width turns the solo pass off
                assert (main[0]["targ"][0], main[0]["solo"]) == ((plan.get("lanes_per_query", 32), 0) if pinned else (32, 1)), (what, main)
                red = [r for r in second if r["kernel"] == "reduce"]
                assert red and all(r["grid"] == 1 and r["fused"] == 1 for r in red), (what, red)   # (a second one: the slow path)
            if label.startswith("SVSDF_ROUND_BPC="):
                bpc = int(label.split("=")[1])
                assert all(r["grid"] <= n_cu * bpc for r in second if r["kernel"] == "round"), what
                assert {r["targ"][0] for r in second if r["kernel"] == "round"} == {8, 32}, what
    need = _required(sid)
    hot = {k for k in covered if k[0] in ("solve", "round", "tail", "classify")}
    print(f"shape id {sid} ({shape}{', edges in global memory' if sid == 16 else ''}): "
          f"{len(need & hot)} of {len(need)} required instantiations covered: " + " ".join("/".join(map(str, k)) for k in sorted(hot, key=str)))
    assert need <= covered, sorted(need - covered, key=str)
