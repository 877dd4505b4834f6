"""The sixteen analytic shape functions are the geometry they claim -- checked on the C oracle (orc.Oracle.shape_eval, the
batch form of orc.shape_sdf) and on FLOAT mode of tests/shape_restatement.py alike, at zero offset.

* Foot point.  For a probe p with value v and central-difference gradient g (h = 1e-6): | |g| - 1 | <= 1e-6 and
  |f(p - v g)| <= 1e-6 -- "f is the exact distance to its own zero set", stated locally; no boundary tracing, so no
  corner-sampling error.  Probes: 4 000 uniform over +-8.5 m plus 1 500 interior ones (f < 0, by rejection from the same
  box), fixed seed.  Probes on the medial axis, where the gradient jumps, may fail: at most 0.5 % of a probe set.
  The measured shares stand in the table above test_foot_point.

  sdRoundedX and bigX are NOT exact inside: their formula (SHP:988-994, 1024-1030) is the distance to the nearer diagonal
  segment minus r, and where the two arms overlap (near the centre, and on the far side of an arm's centre line) the
  nearest rim point belongs to the other arm or to the corner between them: `- r` is then a bound, not the distance.
  Their eikonal norm holds everywhere.  For these two the +-8.5 m set and its exterior probes are held to the same
  0.5 %; the interior set only to the eikonal norm, to the sign (against the plain description "within r of either
  diagonal segment") and to soundness below.

* Soundness, all sixteen.  Zero-set points are traced by sign changes on a 0.05 m grid over +-9 m and bisected to
  |f| < 1e-12; then |f(p)| <= |p - z| (1 + 1e-9) + 1e-12 for every probe p and traced point z (the allowances k_rbound
  uses).  Sampling the zero set can only make this weaker, never wrong.

* Two-sided mesh agreement.  For the 13 shapes with a mesh in tests/golden/reference_assets.json: the z = 0 section
  of the reference's mesh (svsdf_mesh_section, host code) against the traced zero set, both directed Hausdorff distances
  (section sampled every 0.01 m; the traced set's own spacing, up to 0.07 m along the rim, is part of the number).
  HAUSDORFF below holds the measured pair per shape; each gate is its number rounded up to the next 0.01 m, and none may
  exceed 0.17 m, the decimation tolerance test_oracle_shapes.py states -- except where the table says why.
"""
import json
import math
import os

import numpy as np
import pytest

import shape_restatement as sr
from oracle import orc

ASSETS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_assets.json")))
MESHED = sorted(ASSETS["shapes"].keys())
IMPLS = ["oracle", "float"]
X_SHAPES = {"sdRoundedX": 3.0, "bigX": 5.0}
H = 1e-6

_FV, _PROBES, _ZEROS = {}, {}, {}


def fv(impl, name):
    if (impl, name) not in _FV:
        if impl == "oracle":
            o = orc.Oracle(name)
            _FV[(impl, name)] = lambda xy, o=o: o.shape_eval(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
        else:
            sh = sr.Shape(name)
            _FV[(impl, name)] = lambda xy, sh=sh: np.array([sh.sdf(float(x), float(y)) for x, y in np.asarray(xy).reshape(-1, 2)])
    return _FV[(impl, name)]


def probes(name):
    """(4 000 uniform over +-8.5 m, 1 500 interior ones): the same draws for both implementations."""
    if name not in _PROBES:
        rng = np.random.default_rng(4100 + sr.ANALYTIC.index(name))
        wide = rng.uniform(-8.5, 8.5, (4000, 2))
        f = fv("oracle", name)
        inner = np.zeros((0, 2))
        while len(inner) < 1500:
            c = rng.uniform(-8.5, 8.5, (20000, 2))
            inner = np.concatenate([inner, c[f(c) < 0.0]])
        _PROBES[name] = (wide, inner[:1500])
    return _PROBES[name]


def zeros(impl, name):
    if (impl, name) not in _ZEROS:
        _ZEROS[(impl, name)] = sr.trace_zero_set(fv(impl, name))
    return _ZEROS[(impl, name)]


def foot(f, p):
    """(value, eikonal failure mask, foot-point failure mask) of the probes p."""
    v = f(p)
    ex, ey = np.array([H, 0.0]), np.array([0.0, H])
    g = np.column_stack([f(p + ex) - f(p - ex), f(p + ey) - f(p - ey)]) / (2.0 * H)
    eik = np.abs(np.hypot(g[:, 0], g[:, 1]) - 1.0) > 1e-6
    ft = np.abs(f(p - v[:, None] * g)) > 1e-6
    return v, eik, ft


# Measured share of probes that fail the foot test (oracle and FLOAT mode give the same figures):
#                      +-8.5 m set   interior set   eikonal norm alone
#   sdRoundedX           0.2250 %      6.3333 %        0 / 0
#   bigX                 0.1000 %      3.2667 %        0 / 0
#   the other fourteen   0             0               0 / 0        (nothing fails at 1e-6; the condition allows 0.5 %)


def _x_inside(w, p):
    """|p| within r = 0.25 of either diagonal segment of half-length w / 2 per axis: the plain description of the X shapes."""
    a = np.abs(p)
    t = np.clip(0.5 * (a[:, 0] + a[:, 1]), 0.0, 0.5 * w)
    return np.hypot(a[:, 0] - t, a[:, 1] - t) < 0.25


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", sr.ANALYTIC)
def test_foot_point(name, impl):
    f = fv(impl, name)
    wide, inner = probes(name)
    vw, eik_w, ft_w = foot(f, wide)
    vi, eik_i, ft_i = foot(f, inner)
    share_w, share_i = float((eik_w | ft_w).mean()), float((eik_i | ft_i).mean())
    print(f"{name} {impl}: foot-test failures {share_w:.4%} of the +-8.5 m set, {share_i:.4%} of the interior set; "
          f"eikonal alone {eik_w.mean():.4%} / {eik_i.mean():.4%}")
    assert (vi < 0.0).all()
    assert share_w <= 0.005
    ext = vw > 0.0
    assert float((eik_w | ft_w)[ext].mean()) <= 0.005
    if name in X_SHAPES:
        assert float(eik_i.mean()) <= 0.005
        assert _x_inside(X_SHAPES[name], inner).all()
        assert np.array_equal(_x_inside(X_SHAPES[name], wide), vw < 0.0)
    else:
        assert share_i <= 0.005


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", sr.ANALYTIC)
def test_sound_against_traced_zero_set(name, impl):
    f = fv(impl, name)
    Z = zeros(impl, name)
    assert len(Z) >= 100 and np.abs(f(Z)).max() < 1e-12
    worst = -np.inf
    for p in probes(name):
        v = np.abs(f(p))
        for k in range(0, len(p), 500):
            d = np.hypot(p[k:k + 500, None, 0] - Z[None, :, 0], p[k:k + 500, None, 1] - Z[None, :, 1]).min(axis=1)
            worst = max(worst, float((v[k:k + 500] - (d * (1.0 + 1e-9) + 1e-12)).max()))
    print(f"{name} {impl}: {len(Z)} traced zero-set points, max |f(p)| - bound = {worst:.3e}")
    assert worst <= 0.0


# Measured directed Hausdorff distances [m] between the z = 0 section of the reference's mesh and the traced zero set,
# oracle and FLOAT mode alike; the gate is each number rounded up to the next 0.01 m.
#                      section -> zero set   zero set -> section
HAUSDORFF = {
    "sdArc":            (0.032448, 0.001141),
    "sdCutDisk":        (0.403221, 0.402552),
    "sdHeart":          (0.035337, 0.015269),
    "sdHorseshoe":      (0.075468, 0.086315),
    "sdOrientedVesica": (0.038547, 0.072507),
    "sdPie":            (0.074417, 0.063489),
    "sdPie2":           (0.029539, 0.003840),
    "sdRhombus":        (0.025591, 0.019474),
    "sdRoundedCross":   (0.031100, 0.099750),
    "sdRoundedX":       (0.091837, 0.088676),
    "sdTunnel":         (0.050037, 0.040666),
    "sdUnevenCapsule":  (0.068059, 0.064466),
    "star":             (0.064676, 0.043348),
}
# sdCutDisk.obj is a 0.92-scaled copy of the coded shape (r 4.6 / h 1.84 in the mesh, r 5 / h 2 in SHP:682-683): its arc
# sits 0.40 m inside the coded one, which is what the 0.40 m above are.  Not a finding; the section divided by 0.92 is
# measured as well and held to the decimation tolerance like every other mesh:
HAUSDORFF_ABOVE_TOLERANCE = {"sdCutDisk": "the mesh is a 0.92-scaled copy of the coded shape (SHP:682-683)"}
HAUSDORFF_RESCALED = {
    "sdCutDisk":        (0.92, 0.033001, 0.002775),
}


def _gate(x):
    return math.ceil(x * 100.0 - 1e-9) / 100.0


def test_hausdorff_gates_follow_their_rule():
    assert sorted(HAUSDORFF) == MESHED
    for name, pair in HAUSDORFF.items():
        for x in pair:
            assert _gate(x) <= 0.17 or name in HAUSDORFF_ABOVE_TOLERANCE, (name, x)
    for name, (_, a, b) in HAUSDORFF_RESCALED.items():
        assert _gate(a) <= 0.17 and _gate(b) <= 0.17, name


def _section_segments(built, name):
    import svsdf_amd
    V = np.array(ASSETS["shapes"][name], dtype=np.float64)
    F = np.array(ASSETS["mesh_faces"][name], dtype=np.int32)
    xy, sizes = svsdf_amd.mesh_section(V, F)
    A, B, o = [], [], 0
    for n in sizes:
        loop = xy[o:o + n]
        A.append(loop); B.append(np.roll(loop, -1, axis=0))
        o += n
    return np.concatenate(A), np.concatenate(B)


def _dist_to_segments(P, A, B):
    d = B - A
    L2 = (d * d).sum(axis=1)
    out = np.full(len(P), np.inf)
    for k in range(0, len(P), 400):
        w = P[k:k + 400, None, :] - A[None, :, :]
        t = np.clip((w * d[None]).sum(axis=2) / L2[None], 0.0, 1.0)
        c = w - t[:, :, None] * d[None]
        out[k:k + 400] = np.sqrt((c * c).sum(axis=2)).min(axis=1)
    return out


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", MESHED)
def test_mesh_section_and_zero_set_agree_both_ways(built, name, impl):
    A, B = _section_segments(built, name)
    Z = zeros(impl, name)
    s2z, z2s = _hausdorff(A, B, Z)
    print(f"{name} {impl}: section -> zero set {s2z:.6f} m, zero set -> section {z2s:.6f} m ({len(Z)} traced points)")
    assert s2z <= _gate(HAUSDORFF[name][0])
    assert z2s <= _gate(HAUSDORFF[name][1])
    if name in HAUSDORFF_RESCALED:
        k, a, b = HAUSDORFF_RESCALED[name]
        s2z, z2s = _hausdorff(A / k, B / k, Z)
        print(f"{name} {impl}, section / {k}: section -> zero set {s2z:.6f} m, zero set -> section {z2s:.6f} m")
        assert s2z <= _gate(a)
        assert z2s <= _gate(b)


def _hausdorff(A, B, Z):
    S = []
    for a, b in zip(A, B):
        n = max(1, int(math.ceil(np.hypot(*(b - a)) / 0.01)))
        S.append(a[None] + np.linspace(0.0, 1.0, n, endpoint=False)[:, None] * (b - a)[None])
    S = np.concatenate(S)
    s2z = 0.0
    for k in range(0, len(S), 500):
        s2z = max(s2z, float(np.hypot(S[k:k + 500, None, 0] - Z[None, :, 0], S[k:k + 500, None, 1] - Z[None, :, 1]).min(axis=1).max()))
    z2s = float(_dist_to_segments(Z, A, B).max())
    return s2z, z2s
