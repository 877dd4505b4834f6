"""The kernels' square root without range scaling (svsdf_shapes.hpp: sqrt_nz, sqrt_z) against sqrt, bit for bit.

About 2 M operands: +0, the smallest and the largest denormal, 2^-1022, the guard's threshold 2^-767 with its +-1 and +-2 ulp
neighbours, every power of two a double can hold with its two neighbours, perfect squares with their neighbours (the
operands whose root is exact: a wrong last residual step shows there first), +inf, NaN and a log-uniform draw over the
whole exponent range.  The expected count of differing operands is 0 for both helpers; no operand is left out.

The helpers decide per wave: one operand outside [2^-767, inf) sends all 64 lanes through sqrt itself, which would hide the
fast path of its neighbours.  So each helper sees the operands twice: once laid out with the operands its fast path takes
(by the rule stated in svsdf_shapes.hpp) in waves of their own, and once shuffled, every wave mixed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LO = 2.0 ** -767


def _operands():
    rng = np.random.default_rng(8)
    u = lambda b: np.asarray(b, dtype=np.uint64).view(np.float64)
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.uint64)
    parts = [np.array([0.0, 5e-324, np.inf, np.nan, 2.0 ** -1022]), u([0x000FFFFFFFFFFFFF])]
    t = int(bits(LO))
    parts.append(u([t - 2, t - 1, t, t + 1, t + 2]))
    p2 = bits(2.0 ** np.arange(-1074, 1024).astype(np.float64))
    assert p2[0] == 1 and len(np.unique(p2)) == 2098
    parts.append(u(np.concatenate([p2 - 1, p2, p2 + 1])))              # (2^-1074 - 1 ulp is +0, 2^1023's neighbours are finite)
    k = np.arange(1, 150001, dtype=np.float64)
    sq = [k * k]                                                         # exact squares of integers
    m = rng.integers(1 << 25, 1 << 26, 150000).astype(np.float64)        # 26-bit significands: the square is exact
    e = rng.integers(-500, 480, 150000)                                  # 2^-950 .. 2^1012: both sides of the threshold
    sq.append(np.ldexp(m * m, 2 * e))
    for s in sq:
        b = bits(s)
        parts.append(u(np.concatenate([b - 1, b, b + 1])))
    parts.append(u(rng.integers(1, 0x7FF0000000000000, 1200000, dtype=np.uint64)))   # log-uniform: every exponent, denormals too
    x = np.concatenate(parts)
    assert 2_000_000 <= x.size <= 2_300_000
    return x


def _fast(x, flavour):
    """Operands the helper's fast path takes: 2^-767 <= x < inf, and for flavour 1 also +0."""
    f = (x >= LO) & (x < np.inf)
    if flavour == 1:
        f |= x.view(np.uint64) == 0
    return f


@pytest.fixture(scope="module")
def ctx(built):
    import svsdf_amd
    c = svsdf_amd.SvsdfContext(shape="star", device=0)
    yield c
    c.close()


@pytest.mark.parametrize("flavour", [0, 1])
def test_unscaled_sqrt_is_sqrt_bit_for_bit(ctx, flavour):
    x = _operands()
    f = _fast(x, flavour)
    assert f.sum() > 1_500_000 and (~f).sum() > 150_000           # both paths see plenty
    pad = np.ones((-int(f.sum())) % 256)                          # the other operands start at a block (and wave) boundary
    laid = np.concatenate([x[f], pad, x[~f]])
    assert laid.size == x.size + pad.size
    n_laid = ctx.sqrt_mismatches(laid, flavour)
    n_mixed = ctx.sqrt_mismatches(x[np.random.default_rng(9).permutation(x.size)], flavour)
    print(f"flavour {flavour}: {x.size} operands, {int(f.sum())} on the fast path; mismatches laid out {n_laid}, mixed {n_mixed}")
    assert n_laid == 0 and n_mixed == 0


def test_entry_rejects_an_unknown_flavour(ctx):
    """Errors are -1, never a count."""
    assert ctx.sqrt_mismatches(np.array([4.0]), 2) == -1
    assert ctx.sqrt_mismatches(np.array([4.0, 0.0, np.inf]), 0) == 0
