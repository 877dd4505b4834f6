"""A second reading of the sixteen analytic shapes of the reference's Shape.hpp (SHP), in pure Python.

Every function below restates one `getonlySDF(pos_rel)` from the reference's text, citing its SHP lines.  The module was
written from that text alone, BEFORE looking at how oracle/svsdf_oracle.c or csrc/svsdf_shapes.hpp spell the same shape:
its worth is that it is a second reading, so that a misreading shared by the oracle and the kernels (which were written
together, from one reading) does not pass the suite.  tests/golden/make_golden.py holds an older restatement of four of
the shapes; test_shape_restatement.py asserts that this module returns the same bits for those four.

Each shape is written ONCE, over a small arithmetic namespace `A`, and runs in two modes:
  FLOAT  Python floats and `math`: IEEE doubles, the reference's operation order, nothing contracted.  Constants are taken
         the way the reference takes them (the 12-digit k1 literals of `star`, cos(20.5) in radians, ...).  std::max /
         std::min are spelled with their C++ definitions (`a < b ? b : a`, `b < a ? b : a`).
  MP     mpmath.mpf at 50 digits; decimal literals are the doubles the compiler makes of them, the trig and sqrt
         constants are evaluated in mp.  Imported lazily: FLOAT mode (all the GPU tests use) does not need mpmath.

`Shape(name, poly_params, A)` applies the shape's own trans / Rotate (SHP:281-294, row vector times matrix) and
`Shape.at_rest(x, y)` the pose transform of a robot at rest at the origin in front of it (posEva2Rel, SWM:521-526, as
make_golden.Swept.sdf_at spells it) -- this is what orc.shape_sdf and debug_sdf_at on a rest trajectory evaluate.
The z column of the reference's 3x3 product adds 0*0 to both coordinates; it is left out, as in make_golden.py.

`features(name)` lists, per shape, the body-frame points at which its formula is special: arc and circle centres,
vertices and tips, a point on each branch surface of each if / max / clip, and for each norm / sqrt a point that makes its
operand exactly 0 where one exists.  They were listed by reading the formula, and are computed in plain doubles -- where
a surface has no representable point the +-1 ulp neighbours the tests add straddle it.
"""
import math

import numpy as np

PI = 3.14159265358979323846  # SHP:31

ANALYTIC = ["sdUnevenCapsule", "star", "sdTunnel", "sdCutDisk", "sdTrapezoid", "sdRhombus", "sdHorseshoe", "sdHeart",
            "sdRoundedX", "bigX", "sdRoundedCross", "sdOrientedVesica", "sdMoon", "sdPie", "sdPie2", "sdArc"]

PINNED_POSE = (-0.2825779765147789, 0.7125194778521649, -72.4229346429489)     # test_gpu_sdf_at.py


def poses(seed=20250611):
    """The three poses of the tests: zero offset, the pinned one, one seeded random one."""
    rng = np.random.default_rng(seed)
    rnd = (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), float(rng.uniform(-180, 180)))
    return [(0.0, 0.0, 0.0), PINNED_POSE, rnd]


# ------------------------------------------------------------------------------------------------ the two arithmetics
class _Float:
    name = "float"
    c = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    cos = staticmethod(math.cos)
    sin = staticmethod(math.sin)
    abs = staticmethod(abs)

    @staticmethod
    def max(a, b):          # std::max(a, b)
        return b if a < b else a

    @staticmethod
    def min(a, b):          # std::min(a, b)
        return b if b < a else a

    @staticmethod
    def signbit(v):
        return math.copysign(1.0, v) < 0.0

    @staticmethod
    def copysign1(v):       # std::copysign(1.0, v)
        return math.copysign(1.0, v)


FLOAT = _Float()
_MP = None


def MP():
    """The 50-digit namespace (made on first use; needs mpmath)."""
    global _MP
    if _MP is None:
        import mpmath
        ctx = mpmath.mp.clone()
        ctx.dps = 50
        one = ctx.mpf(1)

        class _Mp:
            name = "mp"
            c = staticmethod(ctx.mpf)
            sqrt = staticmethod(ctx.sqrt)
            cos = staticmethod(ctx.cos)
            sin = staticmethod(ctx.sin)
            abs = staticmethod(abs)
            max = staticmethod(_Float.max)
            min = staticmethod(_Float.min)

            @staticmethod
            def signbit(v):
                return v < 0

            @staticmethod
            def copysign1(v):
                return -one if v < 0 else one
        _MP = _Mp()
    return _MP


def _norm(A, x, y):         # Eigen's norm() of a 2-vector: sqrt(x*x + y*y)
    return A.sqrt(x * x + y * y)


def _clip(A, v, lo, hi):    # the reference's clip(): std::max(std::min(value, max_val), min_val)
    return A.max(A.min(v, hi), lo)


# ------------------------------------------------------------------------------------------------ the sixteen shapes
def f_sdUnevenCapsule(A, px, py):           # SHP:531-543, constants SHP:516-518
    r1, r2, h = A.c(2.0), A.c(1.0), A.c(5.0)
    px = A.abs(px)
    b = (r1 - r2) / h
    a = A.sqrt(A.c(1.0) - b * b)
    k = px * (-b) + py * a
    if k < 0.0:
        return _norm(A, px, py) - r1
    if k > a * h:
        return _norm(A, px - A.c(0.0), py - h) - r2
    return (px * a + py * b) - r1


def f_star(A, px, py):                      # SHP:584-601, constants SHP:565-566
    r, rf = A.c(2.8), A.c(0.6)
    k1x, k1y = A.c(0.809016994375), A.c(-0.587785252292)
    k2x, k2y = -k1x, k1y
    px = A.abs(px)
    m = A.c(2.0) * A.max(k1x * px + k1y * py, A.c(0.0))
    px, py = px - m * k1x, py - m * k1y
    m = A.c(2.0) * A.max(k2x * px + k2y * py, A.c(0.0))
    px, py = px - m * k2x, py - m * k2y
    px = A.abs(px)
    py = py - r
    bax, bay = rf * (-k1y) - A.c(0.0), rf * k1x - A.c(1.0)
    h = _clip(A, (px * bax + py * bay) / (bax * bax + bay * bay), A.c(0.0), r)
    return _norm(A, px - bax * h, py - bay * h) * A.copysign1(py * bax - px * bay)


def f_sdTunnel(A, px, py):                  # SHP:642-656, wh SHP:627
    whx, why = A.c(2.5), A.c(1.5)
    px = A.abs(px)
    py = -py
    qx, qy = px - whx, py - why
    mx = A.max(qx, A.c(0.0))
    d1 = mx * mx + qy * qy                  # std::pow(., 2) is the exact square
    qx = qx if py > 0.0 else A.sqrt(px * px + py * py) - whx
    my = A.max(qy, A.c(0.0))
    d2 = qx * qx + my * my
    d = A.sqrt(A.min(d1, d2))
    return -d if A.max(qx, qy) < 0.0 else d


def f_sdCutDisk(A, px, py):                 # SHP:698-709, constants SHP:682-683
    r, h = A.c(5.0), A.c(2.0)
    w = A.sqrt(r * r - h * h)
    px = A.abs(px)
    s = A.max((h - r) * px * px + w * w * (h + r - A.c(2.0) * py), h * px - w * py)
    if s < 0.0:
        return _norm(A, px, py) - r
    if px < w:
        return h - py
    return _norm(A, px - w, py - h)


def f_sdTrapezoid(A, px, py):               # SHP:754-764, constants SHP:733-735
    r1, r2, he = A.c(1.0), A.c(3.0), A.c(2.0)
    k1x, k1y = r2, he
    k2x, k2y = r2 - r1, A.c(2.0) * he
    px = A.abs(px)
    cax = A.max(A.c(0.0), px - (r1 if py < 0.0 else r2))
    cay = A.abs(py) - he
    t = _clip(A, ((k1x - px) * k2x + (k1y - py) * k2y) / (k2x * k2x + k2y * k2y), A.c(0.0), A.c(1.0))
    cbx, cby = (px - k1x) + k2x * t, (py - k1y) + k2y * t
    s = A.c(-1.0) if (cbx < 0.0 and cay < 0.0) else A.c(1.0)
    return s * A.sqrt(A.min(cax * cax + cay * cay, cbx * cbx + cby * cby))


def f_sdRhombus(A, px, py):                 # SHP:809-824 with ndot SHP:808, b SHP:790
    bx, by = A.c(1.0), A.c(4.5)
    px, py = A.abs(px), A.abs(py)
    mx, my = bx - A.c(2.0) * px, by - A.c(2.0) * py
    dp = bx * bx + by * by
    h = _clip(A, (mx * bx - my * by) / dp, A.c(-1.0), A.c(1.0))
    hx, hy = A.c(0.5) * bx, A.c(0.5) * by
    d = _norm(A, px - hx * (A.c(1.0) - h), py - hy * (A.c(1.0) + h))
    sign = A.c(-1.0) if A.signbit(px * by + py * bx - bx * by) else A.c(1.0)
    return d * sign


def f_sdHorseshoe(A, px, py):               # SHP:870-891, constants SHP:854-856 (20.5 is in radians)
    r, wx, wy = A.c(1.5), A.c(1.55), A.c(0.20)
    cx, cy = A.cos(A.c(20.5)), A.sin(A.c(20.5))
    px = A.abs(px)
    l = _norm(A, px, py)
    nx = -cx * px + cy * py
    ny = cy * px + cx * py
    first = nx
    if first <= 0 and ny <= 0:
        nx = l * A.copysign1(-cx)
    if first <= 0:
        ny = l
    nx = nx - wx
    ny = A.abs(ny - r) - wy
    return _norm(A, A.max(nx, A.c(0.0)), A.max(ny, A.c(0.0))) + A.min(A.c(0.0), A.max(nx, ny))


def f_sdHeart(A, px, py):                   # SHP:939-952
    px, py = px / A.c(4.0), py / A.c(4.0)
    px = A.abs(px)
    if py + px > 1.0:
        ax, ay = px - A.c(0.25), py - A.c(0.75)
        return 4 * (A.sqrt(ax * ax + ay * ay) - A.sqrt(A.c(2.0)) / A.c(4.0))
    ax, ay = px - A.c(0.0), py - A.c(1.0)
    v1 = ax * ax + ay * ay
    t = A.max(px + py, A.c(0.0))
    bx, by = px - A.c(0.5) * t, py - A.c(0.5) * t
    v2 = bx * bx + by * by
    return 4 * (A.sqrt(A.min(v1, v2)) * A.copysign1(px - py))


def _rounded_x(A, px, py, w, r):            # SHP:988-994 and, letter for letter, SHP:1024-1030
    ax, ay = A.abs(px), A.abs(py)
    m = (w * A.c(0.5)) if ax + ay > w else (ax + ay) * A.c(0.5)
    return _norm(A, ax - m, ay - m) - r


def f_sdRoundedX(A, px, py):                # SHP:988-994, constants SHP:974-975
    return _rounded_x(A, px, py, A.c(3.0), A.c(0.25))


def f_bigX(A, px, py):                      # SHP:1024-1030, constants SHP:1010-1011
    return _rounded_x(A, px, py, A.c(5.0), A.c(0.25))


def f_sdRoundedCross(A, px, py):            # SHP:1062-1075, h SHP:1046
    h = A.c(1.0)
    px, py = px / A.c(2.0), py / A.c(2.0)
    k = A.c(0.5) * (h + A.c(1.0) / h)
    ax, ay = A.abs(px), A.abs(py)
    if ax < 1.0 and ay < ax * (k - h) + h:
        ux, uy = ax - A.c(1.0), ay - k
        return 2 * (k - A.sqrt(ux * ux + uy * uy))
    ux, uy = ax - A.c(0.0), ay - h
    vx, vy = ax - A.c(1.0), ay - A.c(0.0)
    return 2 * A.sqrt(A.min(ux * ux + uy * uy, vx * vx + vy * vy))


def f_sdOrientedVesica(A, px, py):          # SHP:1115-1146, constants SHP:1097-1099
    ax_, ay_, bx_, by_, w = A.c(2.0), A.c(4.0), A.c(-2.0), A.c(-4.0), A.c(0.8)
    px, py = px / A.c(1.0), py / A.c(1.0)
    ex, ey = bx_ - ax_, by_ - ay_
    r = A.c(0.5) * _norm(A, ex, ey)
    d = A.c(0.5) * (r * r - w * w) / w
    vx, vy = ex / r, ey / r
    cx, cy = A.c(0.5) * (bx_ + ax_), A.c(0.5) * (by_ + ay_)
    dx, dy = px - cx, py - cy
    # rotation << v.y, v.x, -v.x, v.y: Eigen's comma initialiser fills ROWS
    qx = A.c(0.5) * A.abs(vy * dx + vx * dy)
    qy = A.c(0.5) * A.abs((-vx) * dx + vy * dy)
    if r * qx < d * (qy - r):
        hx, hy, hz = A.c(0.0), r, A.c(0.0)
    else:
        hx, hy, hz = -d, A.c(0.0), d + w
    return A.c(1.0) * (_norm(A, qx - hx, qy - hy) - hz)


def f_sdMoon(A, px, py):                    # SHP:1202-1214, constants SHP:1187-1189
    d, ra, rb = A.c(0.8), A.c(3.0), A.c(2.4)
    qx, qy = px, A.abs(py)
    a = (ra * ra - rb * rb + d * d) / (A.c(2.0) * d)
    b = A.sqrt(A.max(ra * ra - a * a, A.c(0.0)))
    cond = d * (qx * b - qy * a) > d * d * A.max(b - qy, A.c(0.0))
    dist1 = _norm(A, qx - a, qy - b)
    dist2 = A.max(_norm(A, qx, qy) - ra, -_norm(A, qx - d, qy - A.c(0.0)) + rb)
    return dist1 if cond else dist2


def _pie(A, px, py, ang):                   # SHP:1253-1260 and, letter for letter, SHP:1294-1301
    cx, cy = A.cos(A.c(ang)), A.sin(A.c(ang))
    r = A.c(3.0)
    px = A.abs(px)
    l = _norm(A, px, py) - r
    t = _clip(A, px * cx + py * cy, A.c(0.0), r)
    m = _norm(A, px - cx * t, py - cy * t)
    return A.max(l, m * A.copysign1(cy * px - cx * py))


def f_sdPie(A, px, py):                     # SHP:1253-1260, c = (cos 43, sin 43) in radians SHP:1235
    return _pie(A, px, py, 43.0)


def f_sdPie2(A, px, py):                    # SHP:1294-1301, c = (cos 1, sin 1) in radians SHP:1276
    return _pie(A, px, py, 1.0)


def f_sdArc(A, px, py):                     # SHP:1334-1343, sc = (sin 20, cos 20) in radians SHP:1320-1322
    scx, scy = A.sin(A.c(20.0)), A.cos(A.c(20.0))
    ra, rb = A.c(2.3333), A.c(0.5)
    px = A.abs(px)
    cond = scy * px > scx * py
    dist1 = _norm(A, px - scx * ra, py - scy * ra)
    dist2 = A.abs(_norm(A, px, py) - ra)
    return (dist1 if cond else dist2) - rb


BODY = {n: globals()["f_" + n] for n in ANALYTIC}


class Shape:
    """getonlySDF(pos_rel) of one analytic shape with its own trans / Rotate (SHP:281-294), in arithmetic A."""

    def __init__(self, name, poly_params=(0.0, 0.0, 0.0), A=FLOAT):
        self.name, self.A, self.f = name, A, BODY[name]
        self.tx, self.ty = A.c(poly_params[0]), A.c(poly_params[1])
        yaw = A.c(poly_params[2]) * A.c(PI) / A.c(180.0)        # SHP:288
        self.R = [[A.cos(yaw), -A.sin(yaw)], [A.sin(yaw), A.cos(yaw)]]      # SHP:289-293
        self.c1, self.s0 = A.c(1.0), A.c(0.0)

    def local(self, x, y):      # ((pos_rel - trans) * Rotate).head(2): row vector times matrix
        dx, dy = x - self.tx, y - self.ty
        return dx * self.R[0][0] + dy * self.R[1][0], dx * self.R[0][1] + dy * self.R[1][1]

    def sdf(self, x, y):
        A = self.A
        px, py = self.local(A.c(x), A.c(y))
        return self.f(A, px, py)

    def at_rest(self, x, y):
        """The shape value at world point (x, y) for a robot at rest at the origin with yaw 0: posEva2Rel (SWM:521-526)
        with sin 0 = 0, cos 0 = 1 spelled out (it mangles signed zeros, as the oracle and the kernels do), then sdf."""
        A = self.A
        s, c = self.s0, self.c1
        dx, dy = A.c(x) - self.s0, A.c(y) - self.s0
        return self.sdf(c * dx + s * dy, (-s) * dx + c * dy)


def to_world(pp, pts):
    """Body-frame points -> the points whose Shape(pp).local() is (up to rounding) the given ones."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    yaw = pp[2] * PI / 180.0
    c, s = math.cos(yaw), math.sin(yaw)
    # local = d R with R = [[c, -s], [s, c]]  =>  d = local R^T
    return np.column_stack([pts[:, 0] * c - pts[:, 1] * s + pp[0], pts[:, 0] * s + pts[:, 1] * c + pp[1]])


# ------------------------------------------------------------------------------------------------ special points
def _rot(p, ang):
    c, s = math.cos(ang), math.sin(ang)
    return (c * p[0] - s * p[1], s * p[0] + c * p[1])


def _mirror_x(pts):
    return list(pts) + [(-x, y) for x, y in pts if x != 0.0]


def features(name):
    """Body-frame points at which the shape's formula is special (see the module docstring), as an (n, 2) array."""
    P = [(0.0, 0.0)]
    if name == "sdUnevenCapsule":
        b = (2.0 - 1.0) / 5.0
        a = math.sqrt(1.0 - b * b)
        P += [(0.0, 5.0), (0.0, -2.0), (0.0, 6.0), (2.0, 0.0), (1.0, 5.0)]               # centres, poles, equators
        P += [(2.0 * a, 2.0 * b), (a, 5.0 + b)]                                          # tangent points: k == 0, k == a h
        P += [(a, b), (4.0 * a, 4.0 * b), (3.0 * a, 5.0 + 3.0 * b), (0.5 * a, 5.0 + 0.5 * b)]     # on the two branch lines
        P = _mirror_x(P)
    elif name == "star":
        k1 = (0.809016994375, -0.587785252292)
        ba = (0.6 * (-k1[1]), 0.6 * k1[0] - 1.0)
        tip, inner = (0.0, 2.8), (ba[0] * 2.8, 2.8 + ba[1] * 2.8)
        mid = (0.5 * inner[0], 0.5 * (tip[1] + inner[1]))                                # on an edge: the norm's operand is 0
        for k in range(5):
            ang = 2.0 * PI * k / 5.0
            P += [_rot(tip, ang), _rot(inner, ang), _rot((-inner[0], inner[1]), ang), _rot(mid, ang)]
            P += [_rot((0.0, 1.0), ang), _rot((0.0, 4.0), ang)]                          # the folds' own axes
            P += [_rot((-k1[1], k1[0]), ang), _rot((-3.0 * k1[1], 3.0 * k1[0]), ang)]    # k1 . p == 0
        # clip surfaces of h: the normals of the edge at its two ends
        n = (-ba[1], ba[0])
        P += [(tip[0] + n[0], tip[1] + n[1]), (inner[0] + n[0], inner[1] + n[1]), (inner[0] - 0.3 * n[0], inner[1] - 0.3 * n[1])]
        P = _mirror_x(P)
    elif name == "sdTunnel":
        P += [(2.5, -1.5), (2.5, 0.0), (0.0, 2.5), (0.0, -1.5), (1.0, 0.0), (3.0, 0.0), (4.0, 0.0)]
        P += [(1.0, -1.5), (3.0, -1.5), (2.5, -1.0), (2.5, -3.0), (2.5, 1.0), (2.0, -1.0), (1.5, -0.5)]
        P += [(0.0, 1.0), (0.0, -1.0), (0.0, -3.0), (1.5, 2.0), (2.5 * 0.6, 2.5 * 0.8)]
        P = _mirror_x(P)
    elif name == "sdCutDisk":
        w = math.sqrt(5.0 * 5.0 - 2.0 * 2.0)
        P += [(0.0, 5.0), (0.0, 2.0), (w, 2.0), (w, 0.0), (w, 3.0), (0.5 * w, 1.0), (2.0 * w, 4.0), (0.0, 3.5)]
        P += [(1.0, 2.0), (6.0, 2.0), (3.0, 4.0), (0.0, 1.0), (0.0, 6.0), (0.0, -1.0)]
        P += [(2.0, (2.0 + 5.0 - (5.0 - 2.0) * 4.0 / (w * w)) / 2.0)]                     # on the parabola of s
        P = _mirror_x(P)
    elif name == "sdTrapezoid":
        P += [(3.0, 2.0), (1.0, -2.0), (0.0, 2.0), (0.0, -2.0), (2.0, 0.0), (0.5, 0.0), (4.0, 0.0)]
        P += [(1.0, -1.0), (1.0, -3.0), (3.0, 3.0), (3.0, 1.0), (0.5, 2.0), (5.0, 2.0), (0.5, -2.0), (4.0, -2.0)]
        P += [(5.0, 1.0), (1.0, 3.0), (3.0, -3.0), (0.5, -1.75), (2.5, 1.0), (1.5, -1.0)]
        P = _mirror_x(P)
    elif name == "sdRhombus":
        P += [(1.0, 0.0), (0.0, 4.5), (0.5, 2.25), (0.25, 3.375), (5.5, 1.0), (4.5, 5.5), (0.5, 0.0), (0.0, 2.0),
              (2.0, 0.0), (0.0, 6.0), (0.25, 1.0), (1.0, 2.25)]
        P = _mirror_x(P)
        P += [(x, -y) for x, y in P if y != 0.0]
    elif name == "sdHorseshoe":
        cx, cy = math.cos(20.5), math.sin(20.5)
        for X in (0.0, 0.5, 1.55, 2.0, -0.5):           # frame coordinates after [-cx cy; cy cx], which is its own inverse
            for Y in (0.0, 1.3, 1.5, 1.7, 2.0):
                P.append((-cx * X + cy * Y, cy * X + cx * Y))
        P += [(0.0, 1.5), (0.0, -1.5), (0.0, 1.3), (0.0, 1.7), (0.0, -1.3), (0.0, -1.7), (1.5, 0.0), (1.3, 0.0), (1.7, 0.0)]
        P = _mirror_x(P)
    elif name == "sdHeart":
        s2 = math.sqrt(2.0)
        P += [(0.0, 4.0), (1.0, 3.0), (2.0, 2.0), (4.0, 0.0), (1.0, 1.0), (3.0, 3.0), (1.0, -1.0), (2.0, -2.0)]
        P += [(1.0, 3.0 + s2), (1.0 + s2, 3.0), (0.0, 2.0), (0.0, 5.0), (0.0, -1.0), (3.0, 1.0), (0.5, 3.5), (2.0, 4.0)]
        P = _mirror_x(P)
    elif name in ("sdRoundedX", "bigX"):
        w = 3.0 if name == "sdRoundedX" else 5.0
        P += [(0.5 * w, 0.5 * w), (1.0, 1.0), (w, 0.0), (0.0, w), (1.0, w - 1.0), (w, w), (0.25, 0.0), (0.0, 0.25)]
        P += [(0.5 * w + 0.25, 0.5 * w), (0.5 * w, 0.5 * w + 0.25), (0.5, 0.0), (0.0, 0.5), (2.0, 1.0), (0.5 * w + 1.0, 0.5 * w + 1.0)]
        P = _mirror_x(P)
        P += [(x, -y) for x, y in P if y != 0.0]
    elif name == "sdRoundedCross":
        s2 = math.sqrt(2.0)
        P += [(2.0, 2.0), (2.0, 0.0), (0.0, 2.0), (2.0, 1.0), (1.0, 2.0), (3.0, 3.0), (1.0, 1.0), (3.0, 0.0), (0.0, 3.0)]
        P += [(2.0 - s2, 2.0 - s2), (1.0, 0.0), (0.0, 1.0), (2.0, 3.0), (3.0, 1.0), (4.0, 4.0)]
        P = _mirror_x(P)
        P += [(x, -y) for x, y in P if y != 0.0]
    elif name == "sdOrientedVesica":
        r = 0.5 * math.sqrt(16.0 + 64.0)
        w = 0.8
        d = 0.5 * (r * r - w * w) / w
        ux, uy = (-4.0 / r) * 0.5, (-8.0 / r) * 0.5
        e1, e2 = (uy, ux), (-ux, uy)                      # q = (|e1 . p|, |e2 . p|)

        def back(qx, qy):
            return (qx * e1[0] + qy * e2[0], qx * e1[1] + qy * e2[1])
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                P += [back(0.0, sy * r), back(sx * d, 0.0), back(sx * w, 0.0), back(sx * d / r, sy * (r + 1.0)),
                      back(sx * 2.0 * d / r, sy * (r + 2.0)), back(0.0, sy * (r + 1.0)), back(sx * 0.4, sy * 0.5 * r),
                      back(sx * 1.0, 0.0), back(0.0, sy * 1.0)]
        P += [(2.0, 4.0), (-2.0, -4.0), (2.0, -4.0), (-2.0, 4.0)]
    elif name == "sdMoon":
        d, ra, rb = 0.8, 3.0, 2.4
        a = (ra * ra - rb * rb + d * d) / (2.0 * d)
        b = math.sqrt(max(ra * ra - a * a, 0.0))
        P += [(d, 0.0), (a, b), (-3.0, 0.0), (d - rb, 0.0), (3.0, 0.0), (d + rb, 0.0), (-2.3, 0.0), (1.5 * a, 1.5 * b),
              (0.5 * a, 0.5 * b), (0.5 * (a + d), 0.5 * b), (a, 0.0), (0.0, b), (4.0, b), (0.0, 3.0), (-1.0, 0.0), (2.0, 0.0)]
        P += [(x, -y) for x, y in P if y != 0.0]
    elif name in ("sdPie", "sdPie2"):
        ang = 43.0 if name == "sdPie" else 1.0
        cx, cy = math.cos(ang), math.sin(ang)
        P += [(3.0 * cx, 3.0 * cy), (1.5 * cx, 1.5 * cy), (4.0 * cx, 4.0 * cy), (0.0, 3.0), (0.0, -3.0), (0.0, 1.0), (0.0, -1.0),
              (0.0, 4.0), (0.0, -4.0), (-2.0 * cy, 2.0 * cx), (2.0 * cy, -2.0 * cx), (3.0 * cx - cy, 3.0 * cy + cx),
              (3.0 * cx + cy, 3.0 * cy - cx), (3.0, 0.0), (1.0, 0.0)]
        P = _mirror_x(P)
    elif name == "sdArc":
        scx, scy = math.sin(20.0), math.cos(20.0)
        ra, rb = 2.3333, 0.5
        P += [(scx * ra, scy * ra), (0.0, ra), (0.0, ra + rb), (0.0, ra - rb), (0.0, -ra), (0.0, -ra - rb), (0.0, -ra + rb)]
        P += [(scx * t, scy * t) for t in (1.0, ra - rb, ra + rb, 4.0)]
        P += [(ra, 0.0), (ra + rb, 0.0), (ra - rb, 0.0), (scx * ra + rb, scy * ra), (scx * ra, scy * ra - rb), (0.0, 1.0), (0.0, -1.0)]
        P = _mirror_x(P)
    else:
        raise KeyError(name)
    return np.array(P, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ sample-set helpers
def ulp_neighbours(pts):
    """The points with their +-1 ulp neighbours in x and in y (5 points each)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    out = [pts]
    for ax in (0, 1):
        for to in (np.inf, -np.inf):
            q = pts.copy()
            q[:, ax] = np.nextafter(q[:, ax], to)
            out.append(q)
    return np.concatenate(out)


def signed_zeros_and_axes():
    z = [(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)]
    z += [(a, v) for a in (0.0, -0.0) for v in (-7.5, -2.0, -0.5, 0.5, 1.0, 3.0, 7.5)]
    z += [(v, a) for a in (0.0, -0.0) for v in (-7.5, -2.0, -0.5, 0.5, 1.0, 3.0, 7.5)]
    return np.array(z, dtype=np.float64)


def trace_zero_set(fv, half=9.0, step=0.05, tol=1e-12):
    """Zero-set points of a vectorised f((n, 2) array) -> (n,): sign changes between neighbours of a `step` grid over
    +-half, each crossing bisected until |f| < tol (or the bracket is one ulp wide).  Returns an (m, 2) array."""
    n = int(round(2 * half / step)) + 1
    g = np.linspace(-half, half, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    V = fv(np.column_stack([X.ravel(), Y.ravel()])).reshape(n, n)
    S = V < 0.0
    A, B = [], []
    i, j = np.nonzero(S[:-1, :] != S[1:, :])
    A.append(np.column_stack([X[i, j], Y[i, j]])); B.append(np.column_stack([X[i + 1, j], Y[i + 1, j]]))
    i, j = np.nonzero(S[:, :-1] != S[:, 1:])
    A.append(np.column_stack([X[i, j], Y[i, j]])); B.append(np.column_stack([X[i, j + 1], Y[i, j + 1]]))
    A, B = np.concatenate(A), np.concatenate(B)
    sa = fv(A) < 0.0
    for _ in range(70):
        M = 0.5 * (A + B)
        vm = fv(M)
        if np.all(np.abs(vm) < tol):
            break
        left = (vm < 0.0) == sa
        A = np.where(left[:, None], M, A)
        B = np.where(left[:, None], B, M)
    M = 0.5 * (A + B)
    return M[np.abs(fv(M)) < tol]


def float_fv(name, pp=(0.0, 0.0, 0.0)):
    """FLOAT mode as a vectorised function of an (n, 2) array of world points (robot at rest at the origin)."""
    sh = Shape(name, pp, FLOAT)
    return lambda xy: np.array([sh.at_rest(float(x), float(y)) for x, y in np.asarray(xy).reshape(-1, 2)])


def edge_set(name, pp, zero_pts, seed):
    """The edge inputs of one analytic shape at pose pp, as world points of a robot at rest at the origin:
    (edge (m, 2), generic (1000, 2)).  edge = features(name) with their ulp neighbours (in the world frame of pp, and as
    they stand), signed zeros and both axes, up to 200 of the given body-frame zero-set points with their +-1 ulp
    neighbours, points at radius 1e3, 1e6 and 1e9 m in 16 directions, coordinates of 1e-300 and 5e-324; generic = seeded
    normal points (sigma 3 m), the kind test_gpu_sdf_at.py draws."""
    rng = np.random.default_rng(seed)
    zero_pts = np.asarray(zero_pts, dtype=np.float64).reshape(-1, 2)
    if len(zero_pts) > 200:
        zero_pts = zero_pts[rng.choice(len(zero_pts), 200, replace=False)]
    ang = 2.0 * PI * (np.arange(16) + 0.25) / 16.0
    far = np.concatenate([r * np.column_stack([np.cos(ang), np.sin(ang)]) for r in (1e3, 1e6, 1e9)])
    far = np.concatenate([far, [[1e9, 0.0], [0.0, -1e9], [-1e6, 0.0], [0.0, 1e3]]])
    tv = [1e-300, -1e-300, 5e-324, -5e-324]
    tiny = [(a, b) for a in tv for b in tv] + [(a, b) for a in tv for b in (0.0, -0.0, 1.0, -2.5)] + \
           [(b, a) for a in tv for b in (0.0, -0.0, 1.0, -2.5)]
    edge = np.concatenate([ulp_neighbours(to_world(pp, features(name))), ulp_neighbours(features(name)),
                           signed_zeros_and_axes(), to_world(pp, signed_zeros_and_axes()),
                           ulp_neighbours(to_world(pp, zero_pts)), far, np.array(tiny, dtype=np.float64)])
    return edge, rng.normal(0.0, 3.0, (1000, 2))
