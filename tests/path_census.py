"""The whole callback of tests/golden/make_golden.py with a branch record per point (tests/golden/golden_census.json).

make_golden.Swept / scale_restatement.ScaledSwept run UNCHANGED but for one call (the rigid pose rotation's sincos, see
CensusSwept): the classes below subclass them and restate no line of the solve.  What a point did is read in two ways, neither of which can move a result:
  * the locals of make_golden's own frames: `gradient_descent` of the point's own solve at the moment it returns (a
    sys.settrace return event of that code object: stop, it), and `true_sdf` each time it asks for a ring sample (the
    calling frame of `solve`: it, theta_res, the rescan's ts and vel -- at the last sample of the last round they are final);
  * wrappers that call the inherited sdf_at / sdf_dot / solve / locate and note the argument or the value they pass through:
    the descent's trial times and time derivatives, the number of solves, locate's fall-through.
The shape is the second reading of tests/shape_restatement.py (FLOAT arithmetic) for the sixteen analytic shapes, under
make_golden's finite-difference gradient macro (SHP:35-53); where make_golden has the shape too, every evaluation asserts
that the two readings give the same bits.  Polygon is make_golden's.

A record is a string of tokens (`encode` / `decode`):
  E | I            main solve f > 0 (returns at SWM:925) | f <= 0 (the GSIP loop)
  ss se sm         interior, |v(t*)| < 0.01: t* < 0.1 (forward rescan) | t* > dur - 0.1 (backward rescan) | neither (no walk)
  ro               the rescan left the path (ts > dur or ts < 0) without finding speed
  w                theta0 < 0 was wrapped by 2 PI
  r<k> x9|xg       k GSIP rounds; left after the ninth | on |max_g| < 0.1
  f                theta_res reached its floor 0.3
  n<k>             k ring samples solved
  ip  z0           the interior result -r_star is positive; z == 0 (gradient left unnormalised)
  -- the point's own solve (the first of the call):
  s1 sl            the seed lies in the first | last layer-1 scan step (ts < 0.15 | ts > dur - 0.15)
  cn cx            a trial that moved towards the window edge was evaluated ON tmin | tmax (the clamp of SWM:1302)
  g<k>             k trials with time derivative exactly 0 (a plateau: the step is 0)
  eh et eo         the descent ended by 29 halvings | 1000 trials | the tolerance
  t0 td wn wx      t* == 0 | t* == dur | t* == tmin > 0 | t* == tmax < dur
  -- from the penalty (BEO:316-340 at safety_hor - sdf, mu = 0.01):
  l0 lk ll         inactive (x < 0) | the cubic knee (0 <= x <= mu) | linear (x > mu)
  b                the local time of t* is within one ulp of 0 or of its piece's duration
  lf<k>            k calls of locate fell through at idx == N
"""
import concurrent.futures as cf
import json
import math
import multiprocessing as mp
import os
import struct
import sys

import scale_restatement as scr
import shape_restatement as sr

mg = scr.mg
EXAMPLE = scr.EXAMPLE
MG_SHAPES = ("star", "sdHorseshoe", "sdHeart", "sdCutDisk")      # the analytic shapes make_golden has as well
MU = 0.01                                                        # grad_cost_p_sw's smoothing width (BEO:1040)


def _bits(v):
    return struct.pack("<d", v)


class CensusShape(mg.Shape):
    """make_golden.Shape (local frame, FD gradient macro, Polygon) over shape_restatement's reading of the formula."""

    def __init__(self, name, poly_params=(0.0, 0.0, 0.0), verts=None):
        super().__init__(name, poly_params, verts)
        self.second = None if name == "Polygon" else sr.Shape(name, tuple(poly_params))
        self.both = name in MG_SHAPES

    def sdf(self, x, y):
        if self.second is None:
            return super().sdf(x, y)
        v = self.second.sdf(x, y)
        if self.both:
            assert _bits(v) == _bits(super().sdf(x, y)), (self.name, x, y)
        return v


class CensusTraj(mg.Traj):
    fell = 0

    def locate(self, t):
        i, s = super().locate(t)
        # idx == N: the remainder exceeded the last duration, and (rem - T) + T gives it back exactly (Sterbenz)
        if i == self.N - 1 and s > self.T[i]:
            self.fell += 1
        return i, s


# ------------------------------------------------------------------------------------------- reading returned frames
_GD = (mg.Swept.gradient_descent.__code__, scr.ScaledSwept.gradient_descent.__code__)
_TRUE = mg.Swept.true_sdf.__code__


class _GdReturn:
    """with _GdReturn() as fr: <one solve>; fr.locals: the locals of make_golden's gradient_descent frame as it returned."""

    def __enter__(self):
        self.locals, self.prev = None, sys.gettrace()
        sys.settrace(self._call)
        return self

    def __exit__(self, *a):
        sys.settrace(self.prev)

    def _call(self, frame, event, arg):
        if frame.f_code in _GD:
            frame.f_trace_lines = False
            return self._ret
        return None

    def _ret(self, frame, event, arg):
        if event == "return":
            self.locals = dict(frame.f_locals)
        return self._ret


class _Census:
    """Mixin over make_golden.Swept or scale_restatement.ScaledSwept: notes what passes through, computes nothing."""
    _main = _in_gd = False
    _in_dot = 0

    def _note_at(self, t):
        if self._main and self._in_gd and not self._in_dot:
            self._ev.append(("a", t))

    def _note_dot(self, g):
        if self._main and self._in_gd:
            self._ev.append(("d", g))

    def gradient_descent(self, tmin, tmax, x0, px, py):
        self._in_gd = True
        if self._main:
            self._win = (tmin, tmax, x0)
        try:
            return super().gradient_descent(tmin, tmax, x0, px, py)
        finally:
            self._in_gd = False

    def solve(self, px, py):
        self._calls += 1
        if self._calls == 1:            # the point itself: the descent's frame is read when it returns
            self._main = True
            try:
                with _GdReturn() as fr:
                    r = super().solve(px, py)
            finally:
                self._main = False
            self._main_result, self._gd = r, fr.locals
            return r
        caller = sys._getframe(1)       # a ring sample: make_golden's true_sdf frame, in the round that asks for it
        assert caller.f_code is _TRUE
        self._loop = dict(caller.f_locals)
        return super().solve(px, py)

    def true_sdf_census(self, px, py, safety_hor):
        """(true_sdf's result, record dict)"""
        self._calls, self._ev, self._loop, self.traj.fell = 0, [], None, 0
        res = self.true_sdf(px, py)
        return res, self._record(res, safety_hor)

    def _record(self, res, safety_hor):
        L, G = self._loop, self._gd       # L: true_sdf's locals at its LAST ring sample (it and theta_res are final there)
        dur, rec = self.dur, {}
        f0, t0, _ = self._main_result
        rec["interior"] = L is not None
        assert rec["interior"] == (not f0 > 0)
        if rec["interior"]:
            v = self.traj.vel(t0)
            if math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) < 0.01:
                rec["slow"] = "start" if t0 < 0.1 else ("end" if t0 > dur - 0.1 else "mid")
                rec["ran_off"] = "ts" in L and (L["ts"] > dur or L["ts"] < 0)
            rec["theta0_wrap"] = math.atan2(L["vel"][0], -L["vel"][1]) < 0
            rec["rounds"] = L["it"]
            rec["exit"] = "ninth" if L["it"] > 8 else "small"
            rec["floor"] = L["theta_res"] == 0.3
            rec["ring"] = self._calls - 1
            rec["positive"] = res[0] > 0
            rec["z0"] = res[2][0] * res[2][0] + res[2][1] * res[2][1] == 0.0     # z > 0.0 failed: (gx, gy) came back as it was
        tmin, tmax, ts = self._win
        rec["seed_first"], rec["seed_last"] = ts < 0.15, ts > dur - 0.15
        g, first, g0, cn, cx = None, True, 0, False, False
        for kind, val in self._ev:
            if kind == "d":
                g = val
            elif first:
                first = False          # the descent's f(x0) (it == 0)
            else:
                g0 += g == 0
                cn |= g > 0 and val == tmin
                cx |= g < 0 and val == tmax
        rec["clamp_tmin"], rec["clamp_tmax"], rec["g0"] = cn, cx, g0
        rec["gd_exit"] = "halvings" if G["stop"] else ("trials" if G["it"] >= 1000 else "tol")
        rec["t0"], rec["tdur"] = t0 == 0.0, t0 == dur
        rec["t_tmin"], rec["t_tmax"] = (t0 == tmin and tmin > 0), (t0 == tmax and tmax < dur)
        x = safety_hor - res[0]
        rec["l1"] = "inactive" if x < 0.0 else ("linear" if x > MU else "knee")
        i, s = self.traj.locate(res[1])
        u = math.ulp(self.traj.T[i])
        rec["boundary"] = abs(s) <= u or abs(s - self.traj.T[i]) <= u
        rec["fell"] = self.traj.fell
        return rec


class CensusSwept(_Census, mg.Swept):
    """make_golden.Swept, counted.  ONE reading differs, on purpose: the pose rotation takes sin and cos of the yaw from one
    libm sincos() call, as scale_restatement.ScaledSwept._u does and as the reference's g++ -O3 build computes Eigen's
    AngleAxis; make_golden calls math.sin and math.cos, whose last bit differs for about one argument
    in a thousand.  The census settled it: on 2 of its first 1 416 points (C-bigX, C-sdPie, both on a flat stretch of f(t))
    that bit moved t* by 5e-9 against the C oracle, which calls sincos(); with it the two agree to 1e-12 everywhere."""

    def _rel(self, px, py, t):      # posEva2Rel SWM:521-526, make_golden.Swept.sdf_at's lines with the merged call
        xt = self.traj.pos(t)
        s, c = scr.sincos(xt[2])
        dx, dy = px - xt[0], py - xt[1]
        return c * dx + s * dy, (-s) * dx + c * dy

    def sdf_at(self, px, py, t):    # SWM:741-750
        f = self.shape.sdf(*self._rel(px, py, t))
        self._note_at(t)
        return f

    def grad_at(self, px, py, t):   # SWM:779-788
        return self.shape.grad(*self._rel(px, py, t))

    def sdf_dot(self, px, py, t):
        self._in_dot += 1
        try:
            g = super().sdf_dot(px, py, t)
        finally:
            self._in_dot -= 1
        self._note_dot(g)
        return g


class CensusScaledSwept(_Census, scr.ScaledSwept):
    def sdf_at_sc(self, px, py, t):
        f = super().sdf_at_sc(px, py, t)
        self._note_at(t)
        return f

    def sdf_dot_sc(self, px, py, t):
        self._in_dot += 1
        try:
            g = super().sdf_dot_sc(px, py, t)
        finally:
            self._in_dot -= 1
        self._note_dot(g)
        return g


def make_swept(shape, poly_params, verts, rows, durs, sc=None):
    sh, tr = CensusShape(shape, poly_params, verts), CensusTraj(rows, durs)
    return CensusSwept(sh, tr) if sc is None else CensusScaledSwept(sh, tr, sc)


# ------------------------------------------------------------------------------------------------------ the record
_FLAGS = [("ran_off", "ro"), ("theta0_wrap", "w"), ("floor", "f"), ("positive", "ip"), ("z0", "z0"), ("seed_first", "s1"),
          ("seed_last", "sl"), ("clamp_tmin", "cn"), ("clamp_tmax", "cx"), ("t0", "t0"), ("tdur", "td"), ("t_tmin", "wn"),
          ("t_tmax", "wx"), ("boundary", "b")]
_ENUMS = [("slow", {"start": "ss", "end": "se", "mid": "sm"}), ("exit", {"ninth": "x9", "small": "xg"}),
          ("gd_exit", {"halvings": "eh", "trials": "et", "tol": "eo"}), ("l1", {"inactive": "l0", "knee": "lk", "linear": "ll"})]
_COUNTS = [("rounds", "r"), ("ring", "n"), ("g0", "g"), ("fell", "lf")]


def encode(rec):
    out = ["I" if rec["interior"] else "E"]
    out += [tok for key, tok in _FLAGS if rec.get(key)]
    out += [m[rec[key]] for key, m in _ENUMS if key in rec]
    out += [tok + str(rec[key]) for key, tok in _COUNTS if rec.get(key)]
    return " ".join(out)


def decode(text):
    toks = text.split()
    rec = {"interior": toks[0] == "I"}
    for key, tok in _FLAGS:
        rec[key] = tok in toks
    for key, m in _ENUMS:
        for val, tok in m.items():
            if tok in toks:
                rec[key] = val
    for key, tok in _COUNTS:
        rec[key] = 0
        for t in toks:
            if t.startswith(tok) and t[len(tok):].isdigit():
                rec[key] = int(t[len(tok):])
    return rec


def features(rec):
    """The branches a record shows, as a set of names (what the census counts and the fixture must keep)."""
    out = {"interior" if rec["interior"] else "exterior", "l1_" + rec["l1"], "gd_exit_" + rec["gd_exit"]}
    out |= {key for key, _ in _FLAGS if rec.get(key)}
    if rec.get("slow"):
        out.add("slow_" + rec["slow"])
    if rec.get("exit"):
        out.add("gsip_exit_" + rec["exit"])
    if rec.get("g0"):
        out.add("plateau")
    if rec.get("fell"):
        out.add("locate_fall_through")
    return out


# ------------------------------------------------------------------------------------------------ a case, end to end
def forward_T(tau):     # BEO:213-226, as make_golden.cost_function spells it
    return [((0.5 * t + 1.0) * t + 1.0) if t > 0.0 else 1.0 / ((0.5 * t - 1.0) * t + 1.0) for t in tau]


def backward_T(T):      # BEO:228-241, as make_golden.main spells it
    return [(math.sqrt(2.0 * t - 1.0) - 1.0) if t > 1.0 else (1.0 - math.sqrt(2.0 / t - 1.0)) for t in T]


def coefficients(head, tail, x):
    N = (len(x) + 3) // 4
    T = forward_T(x[:N])
    rows, _, _ = mg.minco(head, tail, [x[N + 3 * i:N + 3 * i + 3] for i in range(N - 1)], T)
    return rows, T


def _chunk(args):
    """worker (spawned process): census of some points of one case"""
    shape, pp, verts, rows, durs, sc, sh, pts = args
    sw = make_swept(shape, pp, verts, rows, durs, sc)
    out = []
    for p in pts:
        res, rec = sw.true_sdf_census(p[0], p[1], sh)
        out.append(([res[0], res[1], res[2][0], res[2][1]], encode(rec), sw.n_solves))
        sw.n_solves = 0
    return out


def census_points(pool, inp, rows, durs, points):
    """[(per_point row, record string, solves)] of `points` under the inputs `inp`, on the executor `pool`."""
    verts = None if inp.get("polygon") is None else [tuple(v) for v in inp["polygon"]]
    n = max(1, min(len(points), 48))      # chunks: a few per worker
    parts = [points[k::n] for k in range(n)]
    res = list(pool.map(_chunk, [(inp["shape"], tuple(inp["poly_params"]), verts, rows, durs, inp.get("scale"),
                                  inp["safety_hor"], c) for c in parts]))
    out = [None] * len(points)
    for k in range(n):
        for j, r in enumerate(res[k]):
            out[k + j * n] = r
    return out


class _Replay:
    """Stands where cost_function builds its Swept: hands the points' census results to the penalty, in its order."""

    def __init__(self, traj, sc, rows):
        self.traj, self.sc, self.rows, self.k, self.n_solves = traj, sc, rows, 0, 0

    def true_sdf(self, px, py):
        r, _, ns = self.rows[self.k]
        self.k += 1
        self.n_solves += ns
        return r[0], r[1], (r[2], r[3])


def evaluate(pool, inp, head, tail, x):
    """make_golden.cost_function of one case (penalty_sc's position gradient under a schedule) with the per-point work done
    on `pool` -> dict(per_point, rec, n_solves, cost, costs3, grad, T, coeffs)."""
    rows, durs = coefficients(head, tail, x)
    pts = [[p[0], p[1], 0.0] for p in inp["points"]]
    got = census_points(pool, inp, rows, durs, pts)
    sc = inp.get("scale")
    saved = mg.Swept, mg.penalty, mg.Traj
    mg.Traj = CensusTraj
    mg.Swept = lambda shape_, traj: _Replay(traj, sc, got)
    if sc is not None:
        mg.penalty = lambda sw, r_, d_, p_, sh, wp: scr.penalty_sc(sw, r_, d_, p_, sh, wp)
    try:
        verts = None if inp.get("polygon") is None else [tuple(v) for v in inp["polygon"]]
        f, g, c3, b, Tv, per, ns = mg.cost_function(inp["shape"], tuple(inp["poly_params"]), verts, head, tail, x, pts,
                                                    inp["safety_hor"], inp["weight_p"], inp["rho"])
    finally:
        mg.Swept, mg.penalty, mg.Traj = saved
    assert Tv == durs and [list(r) for r in b] == [list(r) for r in rows]
    return dict(per_point=per, rec=[r[1] for r in got], n_solves=ns, cost=f, costs3=c3, grad=g, T=Tv, coeffs=b)


def executor(workers=None):
    nw = workers or max(1, min(16, (os.cpu_count() or 2)))
    return cf.ProcessPoolExecutor(max_workers=nw, mp_context=mp.get_context("spawn"))


# ------------------------------------------------------------------------------------------- what the fixture must hold
PER_CASE = ("exterior", "interior", "l1_knee")
PER_SHAPE = ("slow_start", "slow_end", "slow_mid", "t0", "tdur", "clamp_tmax", "plateau", "theta0_wrap", "floor",
             "gsip_exit_small", "l1_inactive", "l1_linear")
IN_THREE_SHAPES = ("gsip_exit_ninth", "clamp_tmin", "ran_off")
NEVER_REQUIRED = ("gd_exit_trials", "gd_exit_tol", "t_tmin", "t_tmax", "z0", "positive", "locate_fall_through")
ALL_BRANCHES = PER_CASE + PER_SHAPE + IN_THREE_SHAPES + ("gd_exit_halvings", "seed_first", "seed_last", "boundary") + NEVER_REQUIRED


def table(cases):
    """{branch: {shape: number of census points that show it}} over the cases of a fixture."""
    out = {b: {} for b in ALL_BRANCHES}
    for c in cases:
        for text in c["rec"]:
            for b in features(decode(text)):
                out[b][c["shape"]] = out[b].get(c["shape"], 0) + 1
    return out


def check_requirements(doc):
    """The requirements of the census on a fixture (asserted by the generator and by test_path_census.py)."""
    cases, missing = doc["cases"], []
    shapes = sorted({c["shape"] for c in cases})
    assert len(shapes) == 17
    for c in cases:
        have = set().union(*[features(decode(t)) for t in c["rec"]])
        missing += [(c["id"], b) for b in PER_CASE if b not in have]
        x = doc["trajectories"][c["traj"]]["x"]
        N = len(doc["trajectories"][c["traj"]]["T"])
        assert c["tau_le0"] == [i for i in range(N) if x[i] <= 0.0]
        if c["traj"] == "A":      # forwardT / backwardGradT for tau <= 0 (BEO:213-289)
            assert len(c["tau_le0"]) == 2 and all(c["grad"][i] != 0.0 for i in c["tau_le0"]), c["id"]
    tab = table(cases)
    missing += [(s, b) for b in PER_SHAPE for s in shapes if tab[b].get(s, 0) < 1]
    missing += [(sorted(tab[b]), b) for b in IN_THREE_SHAPES if len(tab[b]) < 3]
    assert not missing, missing
    return tab


# ------------------------------------------------------------------------------------------- the fixture, for the tests
def load_fixture():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_census.json")))


def oracle_of(doc, case):
    """(the C oracle of a case with its schedule, no trajectory yet; the case's trajectory record)"""
    import numpy as np
    from oracle import orc
    tj = doc["trajectories"][case["traj"]]
    o = orc.Oracle(case["shape"], safety_hor=case["safety_hor"], weight_p=case["weight_p"], rho=case["rho"],
                   poly_params=case["poly_params"], polygon=case["polygon"], head_state=np.array(tj["head"]).T,
                   tail_state=np.array(tj["tail"]).T)
    if case["scale"]:
        o.set_scale(**case["scale"])
    return o, tj


def cloud(case, repeat=1):
    import numpy as np
    return np.tile(np.array([[p[0], p[1], 0.0] for p in case["points"]]), (repeat, 1))
