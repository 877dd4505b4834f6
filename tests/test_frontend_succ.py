"""svsdf_kernel_bfs against a plain-Python restatement of SweptVolumeManager::checkKernelValue and
visit_kernels_by_distance (sw_manager.hpp:1103-1169) on one cell's word of the yaw-free table.

Host only: no device, no context.  Found / not found, the kernel index and the bits of the child yaw must be equal."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

PI_SW = 3.1415926536            # `#define pi` of sw_manager.hpp:20 (not Shape.hpp:31's PI)
COUNTS = [2, 3, 8, 11, 12, 18, 36, 64]
# i whose hand-out yaw 2*pi*i/count - pi truncates back to i - 1 (the issue's CPU check); the other counts of COUNTS: none
TRUNCATED = {8: [], 18: [2, 11], 36: [1, 4, 11, 22, 29], 64: list(range(43, 64, 4))}


def father_index(count, father_yaw):
    """int(kernel_count * ((father_yaw + pi) / (2 * pi))) (sw_manager.hpp:1160); None where it leaves [0, count)."""
    v = count * ((father_yaw + PI_SW) / (2 * PI_SW))
    if math.isnan(v) or math.isinf(v):
        return None
    i = int(v)                   # truncates towards zero like the C cast
    return i if 0 <= i < count else None


def bfs_ref(mask, count, father_yaw, maxdeepth=10):
    """-> "error" | None | (child_yaw, index).  kernelConv<true>(x, ind) is bit x of `mask`."""
    start = father_index(count, father_yaw)
    if start is None:
        return "error"
    visited = [False] * count
    q = collections.deque([start])
    visited[start] = True
    deep = 0
    while q:
        deep += 1
        x = q.popleft()
        if (mask >> x) & 1:
            return (2 * PI_SW * x / count - PI_SW, x)
        for d in (-1, 1):
            nx = x + d
            if nx < 0:
                nx = count - 1
            if nx >= count:
                nx = 0
            if visited[nx]:
                continue
            visited[nx] = True
            q.append(nx)
        if deep > maxdeepth:
            break
    return None


def handout_yaws(count):
    return [2 * PI_SW * i / count - PI_SW for i in range(count)]


def _c_bfs(L, mask, count, fy, cy0=123.5, ki0=-7):
    cy, ki = C.c_double(cy0), C.c_int(ki0)
    rc = L.svsdf_kernel_bfs(mask, count, fy, C.byref(cy), C.byref(ki))
    return rc, cy.value, ki.value


@pytest.fixture(scope="module")
def L(built):
    import svsdf_amd
    return svsdf_amd.lib()


def _father_yaws(count):
    ys = []
    for y in handout_yaws(count):
        ys += [y, float(np.nextafter(y, -np.inf)), float(np.nextafter(y, np.inf))]
    ys += [-PI_SW, float(np.nextafter(PI_SW, 0.0))]
    return ys


def _masks(count):
    rng = np.random.default_rng(1000 + count)
    full = (1 << count) - 1
    ms = [0, full] + [1 << k for k in range(count)]
    ms += [int(v) & full for v in rng.integers(0, 2 ** 63, 200, dtype=np.uint64) * 2 + rng.integers(0, 2, 200, dtype=np.uint64)]
    return ms


@pytest.mark.parametrize("count", COUNTS)
def test_kernel_bfs_matches_restatement(L, count):
    masks = _masks(count)
    seen = collections.Counter()
    for fy in _father_yaws(count):
        for m in masks:
            want = bfs_ref(m, count, fy)
            rc, cy, ki = _c_bfs(L, m, count, fy)
            if want == "error":
                assert rc < 0 and cy == 123.5 and ki == -7, (count, fy, m)
            elif want is None:
                assert rc == 0 and cy == 123.5 and ki == -7, (count, fy, m)
            else:
                assert rc == 1 and ki == want[1] and cy.hex() == want[0].hex(), (count, fy, m, cy, ki, want)
            seen["error" if want == "error" else "none" if want is None else "found"] += 1
    assert seen["found"] and seen["none"]      # (every yaw of this list with an empty mask is a "none")


def test_kernel_bfs_python_wrapper(L):
    import svsdf_amd
    y = handout_yaws(18)
    assert svsdf_amd.kernel_bfs(1 << 9, 18, y[9]) == (y[9], 9)
    assert svsdf_amd.kernel_bfs(0, 18, y[9]) is None
    with pytest.raises(ValueError):
        svsdf_amd.kernel_bfs(1, 18, PI_SW)


@pytest.mark.parametrize("count", COUNTS)
def test_truncation_of_handed_out_yaws(L, count):
    """Fed the child yaws it hands out itself, the function starts its search at i - 1 for the listed i."""
    ys = handout_yaws(count)
    off = [i for i in range(count) if father_index(count, ys[i]) != i]
    if count in TRUNCATED:
        assert off == TRUNCATED[count]
    assert all(father_index(count, ys[i]) == i - 1 for i in off)
    full = (1 << count) - 1
    for i in range(count):      # a full mask returns the start index itself
        rc, cy, ki = _c_bfs(L, full, count, ys[i])
        assert rc == 1 and ki == (i - 1 if i in off else i)
        assert cy.hex() == ys[ki].hex()


def test_search_depth_at_18_kernels(L):
    """At most 11 kernels, s, s-1, s+1, ..., s-5, s+5: a lone free kernel at s +- 5 is found, at s +- 6 not."""
    count = 18
    ys = handout_yaws(count)
    for s in (0, 9, 17):
        assert father_index(count, ys[s]) == s
        for d in (-5, 5):
            k = (s + d) % count
            rc, cy, ki = _c_bfs(L, 1 << k, count, ys[s])
            assert rc == 1 and ki == k and cy.hex() == ys[k].hex()
        for d in (-6, 6):
            rc, cy, ki = _c_bfs(L, 1 << ((s + d) % count), count, ys[s])
            assert (rc, cy, ki) == (0, 123.5, -7)
    # the order: with s-1 and s+1 both free the search returns s-1; with s+1 and s-2, s+1
    rc, _, ki = _c_bfs(L, (1 << 8) | (1 << 10), count, ys[9])
    assert rc == 1 and ki == 8
    rc, _, ki = _c_bfs(L, (1 << 10) | (1 << 7), count, ys[9])
    assert rc == 1 and ki == 10


def test_small_counts_visit_every_kernel(L):
    """count <= 11: wrap-around and the visited set decide the order; count = 2 tests s, then s - 1."""
    ys = handout_yaws(2)
    assert _c_bfs(L, 0b10, 2, ys[0])[::2] == (1, 1)
    assert _c_bfs(L, 0b01, 2, ys[1])[::2] == (1, 0)
    for count in (3, 8, 11):
        ys = handout_yaws(count)
        for s in range(count):
            for k in range(count):
                rc, _, ki = _c_bfs(L, 1 << k, count, ys[s])
                assert rc == 1 and ki == k
    # 12 kernels: the one opposite the start (s + 6) is out of reach
    ys = handout_yaws(12)
    assert _c_bfs(L, 1 << 6, 12, ys[0])[0] == 0


@pytest.mark.parametrize("count", COUNTS)
def test_rejected_yaws_leave_outputs_untouched(L, count):
    full = (1 << count) - 1
    step = 2 * PI_SW / count
    bad = [PI_SW, float(np.nextafter(PI_SW, np.inf)), 4.0, 1e300, float("inf"), float("-inf"), float("nan"),
           -PI_SW - step, -PI_SW - 1.5 * step, -1e300]
    for fy in bad:
        if bfs_ref(full, count, fy) != "error":       # (-pi - 2 pi / count may round to an index of exactly -1 + ulp)
            continue
        assert _c_bfs(L, full, count, fy) == (-1, 123.5, -7), fy
    assert bfs_ref(full, count, PI_SW) == "error" and bfs_ref(full, count, float("nan")) == "error"
    assert bfs_ref(full, count, -PI_SW - 1.5 * step) == "error"
    # between -pi - 2 pi / count and -pi the cast truncates to index 0: accepted
    fy = -PI_SW - 0.5 * step
    assert father_index(count, fy) == 0
    rc, cy, ki = _c_bfs(L, full, count, fy)
    assert rc == 1 and ki == 0 and cy.hex() == handout_yaws(count)[0].hex()
    # bad counts / null outputs
    assert _c_bfs(L, 1, 0, 0.0)[0] < 0 and _c_bfs(L, 1, 65, 0.0)[0] < 0
    assert L.svsdf_kernel_bfs(1, count, 0.0, None, None) < 0
