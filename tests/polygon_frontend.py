"""Expected values of the Polygon front end (SVSDF_FLAG_POLYGON_YAW_KERNELS), composed from code that is already pinned.
A helper, not a test (tests/test_polygon_frontend.py on the CPU, tests/test_polygon_frontend_gpu.py on the device).

The yaw kernels: cell (x, y) of kernel k is occupied iff Polygon::getonlySDF((x c + y s, x (-s) + y c)) <= margin with
(c, s) = (cos, sin)(yaw_k) -- the body of the reference's two-argument overload (Shape.hpp:1477-1500) with the upper-left
block of AngleAxisd(yaw_k, Z).  The yaw table is the oracle's (shape-independent), cos / sin are libm's through `math`
like the oracle's, the SDF is the oracle's one-argument Polygon::getonlySDF.  Table, successors and searches then come
from the restatements of tests/test_frontend_succ_gpu.py and tests/astar_restatement.py fed with those bytes.

The robots are de-aligned on purpose: the maps put obstacle points and poses on a half-integer lattice, an outline with
integer coordinates puts queries exactly on edges or exactly at the margin, and there the last bit of sin / cos / atan2
-- which differs between libm and the device library -- decides.  The assert_*_admissible functions state what every test re-asserts from
the oracle alone before it looks at a device result."""
import functools
import math

import numpy as np

import astar_restatement as ar
from oracle import orc

MARGIN = 0.5
BAR = ((-5.83, -0.13), (5.83, -0.13), (5.83, 0.13), (-5.83, 0.13))      # 9 distinct kernels of 18: blind to k <-> k + 9
ELL = ((-2.87, -1.21), (3.13, -1.21), (3.13, -0.19), (-1.93, -0.19), (-1.93, 3.77), (-2.87, 3.77))    # 18 distinct kernels
MESH = "sdHeart"        # the reference mesh whose z = 0 outline is the third robot
MIN_GAP = 1e-9          # condition (a)


def _extrude(loops, z0=-0.5, z1=0.5):
    """A triangle mesh whose z = 0 section is the given loops (the walls only, as tests/test_gpu_mesh_shapes.py does)."""
    V, F = [], []
    for lp in loops:
        b, m = len(V), len(lp)
        V += [(x, y, z0) for x, y in lp] + [(x, y, z1) for x, y in lp]
        for i in range(m):
            j = (i + 1) % m
            F += [(b + i, b + j, b + m + j), (b + i, b + m + j, b + m + i)]
    return np.array(V, dtype=np.float64), np.array(F, dtype=np.int32)


class Robot:
    """An outline (n, 2) and, for a multi-loop section, the vertex counts of its loops."""

    def __init__(self, name, xy, loops=None):
        self.name = name
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self.loops = None if loops is None or len(loops) < 2 else [int(v) for v in loops]
        self._zero = None

    def oracle(self):
        return orc.Oracle("Polygon", polygon=self.xy, polygon_loops=self.loops)

    def sdf(self, x, y):
        """Polygon::getonlySDF((x, y)), the one-argument form, through the oracle."""
        if self.loops is None:
            return orc.shape_sdf("Polygon", x, y, polygon=self.xy)
        if self._zero is None:      # what orc.shape_sdf does, with the loops: a zero-motion trajectory
            self._zero = self.oracle()
            self._zero.set_traj(np.zeros((6, 3)), np.array([1.0]))
        return self._zero.sdf_at_time(x, y, 0.0)

    def context(self, svsdf_amd, flags=None, **kw):
        flags = svsdf_amd.FLAG_POLYGON_YAW_KERNELS if flags is None else flags
        return svsdf_amd.SvsdfContext(shape="Polygon", polygon=self.xy, polygon_loops=self.loops, flags=flags, **kw)


@functools.lru_cache(maxsize=None)
def robot(name):
    """bar, L: literal outlines.  mesh: the z = 0 outline of a reference mesh through svsdf_mesh_outline.  ring: the two
    loops of an annular section through svsdf_mesh_section (both host code of the library: no device)."""
    if name == "bar":
        return Robot(name, BAR)
    if name == "L":
        return Robot(name, ELL)
    import svsdf_amd
    from svsdf_amd import workload
    if name == "mesh":
        return Robot(name, workload.mesh_outline(MESH))
    assert name == "ring"
    a = np.linspace(0, 2 * np.pi, 24, endpoint=False) + 0.0137
    outer = np.column_stack([4.37 * np.cos(a), 2.91 * np.sin(a)])
    inner = np.column_stack([0.41 + 2.63 * np.cos(a[::2]), -0.23 + 1.47 * np.sin(a[::2])])[::-1]      # off-centre: 18 distinct kernels
    xy, sizes = svsdf_amd.mesh_section(*_extrude([outer, inner]))
    assert len(sizes) == 2
    return Robot(name, xy, sizes)


@functools.lru_cache(maxsize=None)
def yaw_table(count):
    """(yaws, loop count) of BasicShape::initShape's accumulated loop -PI ... PI: shape-independent, the oracle's."""
    _, _, yaws, n = orc.Oracle("star").shape_kernels(3, count, 1.0, MARGIN)
    return yaws, n


@functools.lru_cache(maxsize=None)
def expected_kernels(name, ks, count, res, margin):
    """(map [count, ks, ks] bool, bytes [count, ks, (ks + 7) // 8], yaws, loop count, min |sdf - margin| over all cells)."""
    rb = robot(name)
    yaws, n = yaw_table(count)
    side = int(0.5 * (ks - 1))
    occ = np.zeros((count, ks, ks), dtype=bool)
    gap = math.inf
    for k in range(count):
        c, s = math.cos(yaws[k]), math.sin(yaws[k])
        for a in range(ks):
            x = res * a - side * res
            for b in range(ks):
                y = res * b - side * res
                d = rb.sdf(x * c + y * s, x * (-s) + y * c)
                occ[k, a, b] = d <= margin
                gap = min(gap, abs(d - margin))
    by = np.packbits(occ, axis=2, bitorder="big")
    for v in (occ, by):
        v.setflags(write=False)
    return occ, by, yaws, n, gap


class PolyCase(ar.Case):
    """astar_restatement.Case for a Polygon robot: the same members, the bytes from expected_kernels instead of
    oracle_bytes(shape, ...), the successor oracle Oracle("Polygon", polygon=outline) -- in libm trig (mode 0, the oracle of
    record) and, as `alt`, with the device library's algorithms (mode 1): condition (b) compares what the two give."""

    def __init__(self, name, ks, count, res, cloud, sta_threshold, occ, bmin, bmax, margin=MARGIN):
        from test_frontend_succ_gpu import yaw_free_ref
        self.shape, self.ks, self.count, self.res, self.margin = name, ks, count, res, margin
        self.robot = robot(name)
        self.cloud, self.sta_threshold = cloud, sta_threshold
        self.occ, self.bmin, self.bmax = occ, np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
        self.X, self.Y = occ.shape[:2]
        _, kb, _, _, self.gap = expected_kernels(name, ks, count, res, margin)
        self.free = yaw_free_ref(occ[:, :, 0], kb, ks)
        self.free.setflags(write=False)
        self.oracles = [self.robot.oracle(), self.robot.oracle()]
        self.oracles[1].set_trig_mode(1)
        self.successors = ar.successors_from_ref(self.oracles[0], occ, self.bmin, self.bmax, res, self.free, ks, count)
        self._memo = {}
        self.alt = _Alt(self)

    def table_kind(self):
        full = np.uint64((1 << self.count) - 1)
        return "ones" if (self.free == full).all() else "mixed" if self.free.any() else "zeros"


class _Alt:
    """The same case searched with the trig-mode-1 oracle (Case.search with the other successor callable)."""

    def __init__(self, c):
        self.__dict__.update({k: getattr(c, k) for k in ("bmin", "bmax", "res", "occ", "X", "Y")})
        self.successors = ar.successors_from_ref(c.oracles[1], c.occ, c.bmin, c.bmax, c.res, c.free, c.ks, c.count)
        self._memo = {}

    search = ar.Case.search


_CASES = {}


def demo_case(name, map_name):
    """Robot `name` on demo map `map_name` of golden/reference_assets.json at resolution 1, kernels 17 / 18, with the
    map's own scenario start and end."""
    key = ("demo", name, map_name)
    if key not in _CASES:
        import test_frontend_succ_gpu as fs
        cloud = np.array(fs.ASSETS["maps"][map_name], dtype=np.float32)
        occ, bmin, bmax = fs.grid_from_cloud(cloud, 1.0)
        c = PolyCase(name, 17, 18, 1.0, cloud, 1, occ, bmin, bmax)
        sc = fs.ASSETS["scenarios"][map_name]
        c.start, c.end = [float(v) for v in sc["start"]], [float(v) for v in sc["end"]]
        _CASES[key] = c
    return _CASES[key]


def grid_case(name, ks, count, res, g, margin=MARGIN):
    """Robot `name` on a synthetic layer-0 occupancy g [X, Y] (test_frontend_succ_gpu.cloud_of)."""
    key = ("grid", name, ks, count, res, margin, g.shape, g.tobytes())
    if key not in _CASES:
        import test_frontend_succ_gpu as fs
        X, Y = g.shape
        _CASES[key] = PolyCase(name, ks, count, res, fs.cloud_of(g, res), 2, g[:, :, None].copy(), [0.0, 0.0, 0.0],
                               [X * res, Y * res, res], margin)
    return _CASES[key]


@functools.lru_cache(maxsize=None)
def demo_successors(name, map_name):
    """The parents / yaws recipe of test_frontend_succ_gpu.reference_case on a demo map, the expected successors in trig
    mode 0 and, for condition (b), in mode 1."""
    import test_frontend_succ_gpu as fs
    from test_frontend_succ import handout_yaws
    c = demo_case(name, map_name)
    cells = [(i, j) for i in range(0, c.X, 2) for j in range(0, c.Y, 3) if not c.occ[i, j, 0]]
    hy = handout_yaws(c.count)
    parents = [cell for cell in cells for _ in (2, 9, 14)]
    yaws = [hy[k] for _ in cells for k in (2, 9, 14)]
    both = [fs.successors_ref(o, c.occ, c.bmin, c.bmax, c.res, c.free, c.ks, c.count, parents, yaws) for o in c.oracles]
    for r in both:
        for a in r:
            a.setflags(write=False)
    return dict(parents=np.array(parents, dtype=np.int32), yaws=np.array(yaws), ok=both[0][0], cyaw=both[0][1],
                stage=both[0][2], alt=both[1])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def assert_successors_admissible(name, map_name):
    """Conditions (a) - (c) of a demo-map successor case, from the oracle alone."""
    c = demo_case(name, map_name)
    s = demo_successors(name, map_name)
    assert c.gap >= MIN_GAP, (name, c.gap)                                                      # (a)
    ok1, cy1, st1 = s["alt"]
    assert np.array_equal(s["ok"], ok1) and np.array_equal(s["stage"], st1) and same_bits(s["cyaw"], cy1)     # (b)
    assert c.table_kind() == "mixed"                                                            # (c)
    assert (np.bincount(s["stage"].ravel(), minlength=5) > 0).all(), np.bincount(s["stage"].ravel(), minlength=5)
    return c, s


def assert_search_admissible(c, start, end, stages_missing=(), **kw):
    """Conditions (a) and (b) of one search, and of (c) the five stages -- `stages_missing` names the stages a case
    cannot show, for a reason its caller gives.  Returns the expected search."""
    ref = c.search(start, end, **kw)
    assert c.gap >= MIN_GAP, (c.shape, c.gap)
    assert ar.same_search(c.alt.search(start, end, **kw), ref) == []
    present = [int(v) > 0 for v in ref["stage_counts"]]
    assert present == [k not in stages_missing for k in range(5)], ref["stage_counts"]
    return ref


# ---------------------------------------------------------------- the committed inputs of both test files
# (robot, kernel_size, kernel_count, resolution, margin) of the svsdf_shape_kernels cases
KERNEL_CASES = [("bar", 17, 18, 1.0, 0.5), ("L", 17, 18, 1.0, 0.5), ("bar", 21, 36, 0.7, 0.35), ("L", 21, 36, 0.7, 0.35),
                ("mesh", 17, 18, 1.0, 0.5), ("ring", 17, 18, 1.0, 0.5), ("bar", 63, 64, 1.0, 0.5)]
GRIDS = [(5, 11), (13, 70)]
GRID_KERNELS = [(3, 2), (9, 8)]
LAYOUTS = ["none", "all", "border", "one", "random"]
MAPS = ["sdHeart", "sdHorseshoe", "star"]
SUCCESSOR_CASES = [(name, m) for name in ("bar", "L") for m in MAPS]


def grid_table_case(name, X, Y, ks, count, lay):
    import test_frontend_succ_gpu as fs
    return grid_case(name, ks, count, 1.0, fs.layout(lay, X, Y, seed=X * 1000 + Y + ks))


# A table of all ones or all zeros compares one constant: outside "none" (ones) and "all" (zeros) every synthetic case has
# a mixed table, except where the geometry leaves no room for one (worked out from the oracle's side alone): the L's 9 x 9
# kernels cover 7 x 6 cells at least, and no cell of a 5 x 11 grid keeps that clear of an occupied border.
DEGENERATE = {("L", 5, 11, 9, "border"): "zeros"}


def expected_table_kind(name, X, Y, ks, lay):
    return {"none": "ones", "all": "zeros"}.get(lay) or DEGENERATE.get((name, X, Y, ks, lay), "mixed")


# The searches: key -> what the oracle-side search must give (the issue's measured reference) and the stages it cannot
# show, with the reason.  Every other case shows all five stages.
SEARCH_CASES = {
    "bar star forward": dict(robot="bar", map="star", reverse=False, status="FOUND", path_len=63),
    "bar star reverse": dict(robot="bar", map="star", reverse=True, status="FOUND", path_len=61),
    "L star forward": dict(robot="L", map="star", reverse=False, status="EXHAUSTED", path_len=0),
    "L star reverse": dict(robot="L", map="star", reverse=True, status="FOUND", path_len=66),
    "L sdHeart forward": dict(robot="L", map="sdHeart", reverse=False, status="EXHAUSTED", path_len=0),
    # the expansion limit keeps the search at the scenario's start, which lies in open space well inside the map: one
    # expansion tests the start cell's nine neighbours and accepts them all; fifty never reach the map's border (no stage
    # 1) nor a cell without a free yaw kernel (no stage 3)
    "bar star limit 1": dict(robot="bar", map="star", reverse=False, status="LIMIT", path_len=0, max_expansions=1,
                             stages_missing=(1, 2, 3, 4)),
    "bar star limit 50": dict(robot="bar", map="star", reverse=False, status="LIMIT", path_len=0, max_expansions=50,
                              stages_missing=(1, 3)),
    # a grid without an occupied cell: nothing to be occupied by, to collide with or to block a yaw
    "bar free 5 x 11": dict(robot="bar", grid=(5, 11, 3, 2), status="FOUND", path_len=11, stages_missing=(2, 3, 4)),
}


def search_case(key):
    """(case, start, end, search keywords, expected search) of SEARCH_CASES[key], conditions (a) - (c) asserted."""
    w = SEARCH_CASES[key]
    kw = {k: w[k] for k in ("max_expansions",) if k in w}
    if "grid" in w:
        X, Y, ks, count = w["grid"]
        c = grid_case(w["robot"], ks, count, 1.0, np.zeros((X, Y), dtype=bool))
        start, end = c.centre((0, 0)), c.centre((X - 1, Y - 1))
    else:
        c = demo_case(w["robot"], w["map"])
        start, end = (c.end, c.start) if w["reverse"] else (c.start, c.end)
        assert c.table_kind() == "mixed"
    ref = assert_search_admissible(c, start, end, w.get("stages_missing", ()), **kw)
    return c, start, end, kw, ref
