"""AstarPathSearcher::AstarPathSearch + getPath (front_end_Astar.hpp:243-390) in plain Python, over a callable
`successors(cell, yaw) -> (ok[9], child_yaw[9], stage[9])` that stands for AstarGetSucc (:192-241).  A helper, not a test.

What is restated, because svsdf_astar_search has to reproduce it bit for bit:
  * the separate start node (startPtr, :266-283): g = 0, yaw = start_yaw, no father; the MAP's start cell only gets
    id = 1, g = 0, f = h (:285-287) and never enters the open set;
  * the open set is a std::multimap<double, GridNode*>: begin() is the smallest key and, among equal keys, the entry
    inserted first -- the minimum over (key, insertion sequence number);
  * the three id branches (:319-357): id 0 -> discovered and pushed; id 1 -> g / f / father lowered, the multimap key
    stays (stale key); id -1 -> lowered, reopened and pushed;
  * a node's yaw is the one handed out at its first discovery (:231-234), whatever father it ends up with;
  * the goal test is the index comparison at pop time, before expansion.
The stop after `max_expansions` expansions is the library's (the reference has none): after an expansion the search ends
EXHAUSTED when the open set is empty, else LIMIT when the count is reached.

open_set="argmin": an unordered list, pop = min over (key, seq).  open_set="sorted": the literal second form -- a list kept
sorted by key, insertion at the upper bound of the equal range (std::multimap::insert), pop from the front."""
import bisect
import math

import numpy as np

START = -2       # father_cell of the start node's children; -1: none
STATUS = ["FOUND", "EXHAUSTED", "LIMIT", "OUT_OF_MAP"]


def heu(i, j, gi, gj):
    """getHeu (:165-182) with dz = 0."""
    p = 1.0 / 1000
    dx, dy, dz = abs(i - gi), abs(j - gj), 0
    dmin = min(dx, min(dy, dz))
    dmax = max(dx, max(dy, dz))
    dmid = dx + dy + dz - dmin - dmax
    h = math.sqrt(3) * dmin + math.sqrt(2) * (dmid - dmin) + (dmax - dmid)
    return h * (1 + p)


class _ArgminOpen:
    def __init__(self):
        self.e = []          # (key, seq, node)
        self.seq = 0

    def push(self, key, node):
        self.e.append((key, self.seq, node))
        self.seq += 1

    def pop(self):
        k = min(range(len(self.e)), key=lambda q: self.e[q][:2])
        key, _, node = self.e[k]
        tie = sum(1 for x in self.e if x[0] == key) >= 2
        self.e[k] = self.e[-1]      # swap with the last entry
        self.e.pop()
        return node, tie

    def __len__(self):
        return len(self.e)


class _SortedOpen:
    def __init__(self):
        self.keys, self.nodes = [], []

    def push(self, key, node):
        at = bisect.bisect_right(self.keys, key)      # the upper bound of the equal range
        self.keys.insert(at, key)
        self.nodes.insert(at, node)

    def pop(self):
        tie = len(self.keys) >= 2 and self.keys[0] == self.keys[1]
        self.keys.pop(0)
        return self.nodes.pop(0), tie

    def __len__(self):
        return len(self.keys)


def search(successors, X, Y, start, goal, res, bmin, start_yaw=0.0, max_expansions=0, open_set="argmin"):
    """start / goal: cells (i, j).  Returns a dict shaped like SvsdfContext.astar_search + astar_nodes: status, cells,
    path, path_len, id, g, f, yaw, father_cell, expansions, pushes, relaxed_open, reopened, stage_counts, g_goal; plus
    ties (pops at which the two smallest keys were equal), pops and max_open."""
    si, sj = start
    gi, gj = goal
    nid = np.zeros((X, Y), dtype=np.int8)
    g = np.zeros((X, Y))
    f = np.zeros((X, Y))
    yaw = np.zeros((X, Y))
    father = np.full((X, Y), -1, dtype=np.int32)
    opn = _ArgminOpen() if open_set == "argmin" else _SortedOpen()
    h0 = heu(si, sj, gi, gj)
    opn.push(h0, START)
    nid[si, sj], g[si, sj], f[si, sj] = 1, 0.0, h0
    out = dict(expansions=0, pushes=1, relaxed_open=0, reopened=0, ties=0, pops=0, max_open=1, g_goal=0.0)
    stage_counts = np.zeros(5, dtype=np.uint64)
    status, terminate = None, None
    while status is None:
        cur, tie = opn.pop()
        out["pops"] += 1
        out["ties"] += int(tie)
        if cur == START:
            ci, cj, fy, gcur = si, sj, start_yaw, 0.0
        else:
            ci, cj = divmod(cur, Y)
            fy, gcur = float(yaw[ci, cj]), float(g[ci, cj])
            nid[ci, cj] = -1
        if (ci, cj) == (gi, gj):
            status, terminate = "FOUND", cur
            out["g_goal"] = gcur
            break
        ok, cyaw, stage = successors((ci, cj), fy)
        for s in range(9):
            stage_counts[int(stage[s])] += 1
        for s in range(9):
            if not ok[s]:
                continue
            i, j = s // 3 - 1, s % 3 - 1
            vi, vj = ci + i, cj + j
            ec = math.sqrt(i * i + j * j)
            tg = ec + gcur
            if nid[vi, vj] == 0:
                yaw[vi, vj] = cyaw[s]
            elif not tg < g[vi, vj]:
                continue
            was = nid[vi, vj]
            father[vi, vj] = cur
            g[vi, vj] = tg
            f[vi, vj] = tg + heu(vi, vj, gi, gj)
            if was == 1:
                out["relaxed_open"] += 1          # the key in the open set stays
                continue
            nid[vi, vj] = 1
            opn.push(float(f[vi, vj]), vi * Y + vj)
            out["pushes"] += 1
            out["reopened"] += int(was == -1)
        out["max_open"] = max(out["max_open"], len(opn))
        out["expansions"] += 1
        if len(opn) == 0:
            status = "EXHAUSTED"
        elif max_expansions and out["expansions"] >= max_expansions:
            status = "LIMIT"
    cells = []
    if status == "FOUND":               # getPath: walk the fathers, reverse
        c = terminate
        while c != START:
            cells.append(divmod(c, Y))
            c = int(father[cells[-1]])
            assert c != -1
        cells.append((si, sj))
        cells.reverse()
    path = np.zeros((len(cells), 3))
    for k, (i, j) in enumerate(cells):
        path[k] = [(i + 0.5) * res + bmin[0], (j + 0.5) * res + bmin[1], start_yaw if k == 0 else yaw[i, j]]
    out.update(status=status, cells=np.array(cells, dtype=np.int32).reshape(-1, 2), path=path, path_len=len(cells), id=nid, g=g,
               f=f, yaw=yaw, father_cell=father, stage_counts=stage_counts)
    return out


def successors_from_ref(o, occ, bmin, bmax, res, free, ks, count):
    """The callable `search` wants, composed from tests/test_frontend_succ_gpu.successors_ref (the map restatement and the
    oracle's checkSubSWCollision).  A node expanded again (reopened) asks the same question: answers are kept."""
    from test_frontend_succ_gpu import successors_ref
    memo = {}

    def successors(cell, fy):
        key = (cell[0], cell[1], float(fy).hex())
        if key not in memo:
            ok, cy, st = successors_ref(o, occ, bmin, bmax, res, free, ks, count, [cell], [fy])
            memo[key] = (ok[0], cy[0], st[0])
        return memo[key]
    return successors


NODE_KEYS = ("id", "g", "f", "yaw", "father_cell")
COUNTERS = ("expansions", "pushes", "relaxed_open", "reopened")


def same_search(a, b, keys=("status", "path_len", "g_goal") + COUNTERS):
    """Every field two results share must be equal: the floats bit for bit.  Returns the list of differing fields."""
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    bad = [k for k in keys if k in a and k in b and a[k] != b[k]]
    bad += [k for k in ("cells", "id", "father_cell", "stage_counts") if not np.array_equal(a[k], b[k])]
    bad += [k for k in ("path", "g", "f", "yaw") if a[k].shape != b[k].shape or not np.array_equal(bits(a[k]), bits(b[k]))]
    return bad


# ---------------------------------------------------------------- the cases of tests/test_astar_*.py
MARGIN = 0.5


def grid_index(p, bmin, bmax, res, dims):
    """isInMap (Gridmap3D.cpp:43-71) + getGridIndex (:137-177): None outside the map, else the cell (i, j, k)."""
    if any(p[d] < bmin[d] or p[d] > bmax[d] for d in range(3)):
        return None
    return tuple(min(max(int(math.floor((p[d] - bmin[d]) / res)), 0), dims[d] - 1) for d in range(3))


class Case:
    """A map, a robot, the kernel geometry and everything the restatement needs; built once and shared."""

    def __init__(self, shape, ks, count, res, cloud, sta_threshold, occ, bmin, bmax):
        from oracle import orc
        from test_frontend_succ_gpu import oracle_bytes, yaw_free_ref
        self.shape, self.ks, self.count, self.res = shape, ks, count, res
        self.cloud, self.sta_threshold = cloud, sta_threshold
        self.occ, self.bmin, self.bmax = occ, np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
        self.X, self.Y = occ.shape[:2]
        self.free = yaw_free_ref(occ[:, :, 0], oracle_bytes(shape, ks, count, res, MARGIN), ks)
        self.successors = successors_from_ref(orc.Oracle(shape), occ, self.bmin, self.bmax, res, self.free, ks, count)
        self._memo = {}

    def centre(self, cell):
        return [(cell[0] + 0.5) * self.res + self.bmin[0], (cell[1] + 0.5) * self.res + self.bmin[1],
                0.5 * self.res + self.bmin[2]]

    def search(self, start_xyz, end_xyz, start_yaw=0.0, max_expansions=0, open_set="argmin"):
        """AstarPathSearch(start, end) in world coordinates; results are kept (and must not be written to)."""
        key = (tuple(start_xyz), tuple(end_xyz), start_yaw, max_expansions, open_set)
        if key not in self._memo:
            s = grid_index(start_xyz, self.bmin, self.bmax, self.res, self.occ.shape)
            e = grid_index(end_xyz, self.bmin, self.bmax, self.res, self.occ.shape)
            if s is None or e is None:
                self._memo[key] = dict(status="OUT_OF_MAP", path_len=0)
            else:
                assert s[2] == 0 and e[2] == 0
                self._memo[key] = search(self.successors, self.X, self.Y, s[:2], e[:2], self.res, self.bmin, start_yaw,
                                         max_expansions, open_set)
        return self._memo[key]

    def device_map(self, svsdf_amd):
        return svsdf_amd.OccupancyMap(self.cloud, resolution=self.res, sta_threshold=self.sta_threshold)


_CASES = {}


def demo_case(name):
    """Demo scenario `name` of golden/reference_assets.json: its map at resolution 1, kernels 17 / 18, its own shape."""
    if ("demo", name) not in _CASES:
        import test_frontend_succ_gpu as fs
        cloud = np.array(fs.ASSETS["maps"][name], dtype=np.float32)
        occ, bmin, bmax = fs.grid_from_cloud(cloud, 1.0)
        c = Case(name, 17, 18, 1.0, cloud, 1, occ, bmin, bmax)
        sc = fs.ASSETS["scenarios"][name]
        c.start, c.end = [float(v) for v in sc["start"]], [float(v) for v in sc["end"]]
        _CASES[("demo", name)] = c
    return _CASES[("demo", name)]


def grid_case(shape, ks, count, res, g):
    """A synthetic layer-0 occupancy g [X, Y] (tests/test_frontend_succ_gpu.cloud_of: bounds 0 .. X res, 0 .. Y res, one layer)."""
    key = ("grid", shape, ks, count, res, g.shape, g.tobytes())
    if key not in _CASES:
        import test_frontend_succ_gpu as fs
        X, Y = g.shape
        _CASES[key] = Case(shape, ks, count, res, fs.cloud_of(g, res), 2, g[:, :, None].copy(), [0.0, 0.0, 0.0],
                           [X * res, Y * res, res])
    return _CASES[key]


def sparse_grid(density, seed):
    """Case 3's 13 x 70 layout: default_rng(seed).random((13, 70)) < density with the two end cells cleared."""
    g = np.random.default_rng(seed).random((13, 70)) < density
    g[1, 1] = g[11, 68] = False
    return g
