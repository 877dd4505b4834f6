"""The reference's piece-local time, restated in plain Python, pins the oracle's two forms of it (no GPU).

Trajectory::locatePieceIdx (TRJ:498-516) subtracts the durations one after the other from t until the remainder is no
longer above the next duration (past the end: the last piece, TRJ:510-514); Trajectory::getPos (TRJ:520-524) then
evaluates that piece's quintic with tn built by repeated multiplication (Piece::getPos, TRJ:104-114).  Python floats are
IEEE doubles and every operation below is one rounding in the reference's order, so the restatement is exact: the oracle
(built with -ffp-contract=off) must reproduce it bit for bit --
  * orc set_modes(., 0): the reference's chain of subtractions;
  * orc set_modes(., 1): the cumulative form t - S_i (S_i = T_0 + ... + T_{i-1} summed left to right), one rounding.
The GPU tests (test_piece_time_gpu.py) compare the kernels against the oracle; this file makes sure the oracle itself is
the reference's arithmetic, and that the library's rule for when the cumulative form may stand in for the chain
(svsdf_pipeline.hip: every duration a multiple of 2^-20 below 2^20) is both sound and not vacuous.
The helpers are imported by test_piece_time_gpu.py.
"""
import struct

import numpy as np
import pytest

from oracle import orc

PIECE_COUNTS = [1, 2, 5, 8, 9, 16, 17, 33, 64, 65, 127, 128]


# ---- the restatement -------------------------------------------------------------------------------------------------
def locate_chain(T, t):
    """Trajectory::locatePieceIdx (TRJ:498-516): (piece, local time)."""
    N = len(T)
    idx = 0
    while idx < N and t > T[idx]:
        t -= T[idx]
        idx += 1
    if idx == N:
        idx -= 1
        t += T[idx]
    return idx, t


def locate_cumulative(T, t):
    """The cumulative form: piece = first i with t <= S_{i+1} (clamped to N - 1), local time t - S_i in one rounding."""
    N = len(T)
    S = 0.0
    idx = 0
    while idx < N - 1 and t > S + T[idx]:
        S += T[idx]
        idx += 1
    return idx, t - S


def piece_pos(coeffs, i, s):
    """Piece::getPos (TRJ:104-114); coeffs row 6 i + k = coefficient of s^k of piece i."""
    out = []
    for d in range(3):
        p, tn = 0.0, 1.0
        for k in range(6):
            p += tn * float(coeffs[6 * i + k, d])
            tn *= s
        out.append(p)
    return out


def pos(coeffs, T, t, cumulative=False):
    i, s = (locate_cumulative if cumulative else locate_chain)(T, t)
    return piece_pos(coeffs, i, s)


def partial_sums(T):
    """S_0 = 0, S_{i+1} = S_i + T_i, summed left to right (Trajectory::getTotalDuration's order, TRJ:410-419)."""
    S = [0.0]
    for v in T:
        S.append(S[-1] + float(v))
    return S


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def chain_boundaries(T):
    """For i = 0 .. N-2: the largest t (a positive double) that the chain still places in piece <= i.  The chain's piece
    index is monotone in t (rounded subtraction and comparison both are), so a bisection over the bit patterns of the
    positive doubles finds the exact switch next to S_{i+1}."""
    T = [float(v) for v in T]
    S = partial_sums(T)
    out = []
    for i in range(len(T) - 1):
        lo = hi = _bits(S[i + 1])
        step = 64
        while locate_chain(T, _from_bits(lo))[0] > i:
            lo -= step
            step *= 2
        step = 64
        while locate_chain(T, _from_bits(hi))[0] <= i:
            hi += step
            step *= 2
        while hi - lo > 1:                      # invariant: lo in piece <= i, hi in piece > i
            mid = (lo + hi) // 2
            if locate_chain(T, _from_bits(mid))[0] <= i:
                lo = mid
            else:
                hi = mid
        out.append(_from_bits(lo))
    return out


def probe_times(T, rng, n_uniform=200):
    """The times the tests probe: uniform over [0, total]; every sequential partial sum S_i and its neighbours at +-1, +-2
    and +-64 ulp; the chain's exact boundaries and the double after each; 0, total, and past the end up to total + 3.4."""
    T = [float(v) for v in T]
    S = partial_sums(T)
    total = S[-1]
    ts = list(rng.uniform(0.0, total, n_uniform))
    for s in S[1:]:
        ts.append(s)
        for k in (1, 2, 64):
            up, dn = s, s
            for _ in range(k):
                up = np.nextafter(up, np.inf)
                dn = np.nextafter(dn, -np.inf)
            ts += [float(up), float(dn)]
    for b in chain_boundaries(T):
        ts += [b, float(np.nextafter(b, np.inf))]
    ts += [0.0, total, total + 1e-9, total + 0.5, total + 3.4]
    return np.array([t for t in ts if t >= 0.0])


def generic_durations(N, rng):
    """Generic doubles with a wide spread (0.05 ... 4 s); one trajectory in three also puts a 1e-3 s piece next to a
    3 s one."""
    T = rng.uniform(0.05, 4.0, N)
    if N >= 3 and N % 3 == 0:
        k = int(rng.integers(0, N - 1))
        T[k], T[k + 1] = 1e-3 * (1.0 + 1e-3 * rng.standard_normal()), 3.0 * (1.0 + 1e-3 * rng.standard_normal())
    return T


def _oracle(N, T, rng, cum):
    coeffs = rng.uniform(-3.0, 3.0, (6 * N, 3))
    o = orc.Oracle("star")
    o.set_traj(coeffs, T)
    o.set_modes(1, cum)
    return o, coeffs


# ---- the oracle against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", PIECE_COUNTS)
def test_oracle_pos_is_the_reference_chain_and_the_cumulative_form(N):
    rng = np.random.default_rng(500 + N)
    T = generic_durations(N, rng)
    ts = probe_times(T, rng)
    for cum in (0, 1):
        o, coeffs = _oracle(N, T, rng, cum)
        got = np.array([o.pos(t) for t in ts])
        want = np.array([pos(coeffs, T, float(t), cumulative=bool(cum)) for t in ts])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (N, cum, len(bad), ts[bad[:3]])


def test_chain_boundaries_are_exact():
    """The bisection's boundary b_i is in piece i and the next double is in piece i + 1; the boundary sits within a few
    ulp of S_{i+1} and on either side of it, depending on rounding (so the S_i neighbours alone would miss some)."""
    rng = np.random.default_rng(3)
    T = generic_durations(128, rng)
    S = partial_sums(T)
    sides = set()
    for i, b in enumerate(chain_boundaries(T)):
        assert locate_chain(T, b)[0] == i and locate_chain(T, float(np.nextafter(b, np.inf)))[0] == i + 1, i
        assert abs(b - S[i + 1]) <= 256 * np.spacing(S[i + 1]), (i, b, S[i + 1])
        sides.add(np.sign(b - S[i + 1]))
    assert {-1.0, 1.0} <= sides, sides


# ---- the mode rule: when the cumulative form is the chain ---------------------------------------------------------------
def _coarse(T):
    return all(v < 2.0 ** 20 and np.ldexp(v, 20) == np.floor(np.ldexp(v, 20)) for v in T)


@pytest.mark.parametrize("T", [np.full(16, 2.5), np.full(128, 2.5), np.array([2.5 + 2.0 ** -20] * 40),
                               np.array([0.75, 2.5, 2.5 + 2.0 ** -20, 1.0, 0.5 + 3 * 2.0 ** -20] * 13),
                               np.array([2.0 ** 19 + 2.0 ** -20, 3 * 2.0 ** -20, 1000.25])],
                         ids=["16x2.5", "128x2.5", "40x(2.5+2^-20)", "mixed65", "wide3"])
def test_coarse_durations_make_both_forms_identical(T):
    """Every duration a multiple of 2^-20 below 2^20 (the library's "coarse" rule, mode 0): all partial sums and all
    differences with t are exact, so the chain and the cumulative form agree to the last bit -- piece and local time --
    at every probed time, and the oracle's two modes give the same pose bits."""
    assert _coarse(T)
    rng = np.random.default_rng(len(T))
    ts = probe_times(T, rng, n_uniform=2000)
    ts = np.concatenate([ts, rng.uniform(0.0, 2.0 ** 30, 500)])      # up to the rule's bound on the total duration
    for t in ts:
        assert locate_chain(T, float(t)) == locate_cumulative(T, float(t)), (t,)
    N = len(T)
    oc, coeffs = _oracle(N, T, rng, 0)
    ou = orc.Oracle("star")
    ou.set_traj(coeffs, T)
    ou.set_modes(1, 1)
    a = np.array([oc.pos(t) for t in ts])
    b = np.array([ou.pos(t) for t in ts])
    assert np.array_equal(a, b)


def _first_difference(T, ts):
    for t in ts:
        if locate_chain(T, float(t)) != locate_cumulative(T, float(t)):
            return float(t)
    return None


def test_the_coarse_rule_is_not_vacuous():
    """Off the rule the two forms part: generic durations at ordinary times, and 2^-21-granular durations as soon as
    ulp(t) outgrows their granularity (the rule's 2^-20 and its total below 2^30 leave that far out of reach).  Each difference found in the
    restatement is also one in the oracle's pose.  (The 2^-21 case needs t >= 2^33: ties of the chain's roundings cancel below that
for these durations.)"""
    rng = np.random.default_rng(21)
    cases = []
    T = generic_durations(16, rng)                          # generic doubles: within the trajectory
    cases.append((T, probe_times(T, rng)))
    T = np.array([2.5 + 2.0 ** -21, 0.75 + 2.0 ** -21, 1.0 + 3 * 2.0 ** -21] * 3)
    assert not _coarse(T)
    cases.append((T, 2.0 ** 33 + 2.0 ** -19 * rng.integers(0, 2 ** 20, 2000)))
    for T, ts in cases:
        t = _first_difference(T, ts)
        assert t is not None, T
        N = len(T)
        oc, coeffs = _oracle(N, T, rng, 0)
        ou = orc.Oracle("star")
        ou.set_traj(coeffs, T)
        ou.set_modes(1, 1)
        assert list(oc.pos(t)) == pos(coeffs, T, t) and list(ou.pos(t)) == pos(coeffs, T, t, cumulative=True)
        ic, sc = locate_chain(T, t)
        iu, su = locate_cumulative(T, t)
        assert (ic, sc) != (iu, su)
        if ic == iu:                                        # same piece, another local time: another pose
            assert not np.array_equal(oc.pos(t), ou.pos(t)), t
    # and 2^-21 granularity is still exact below 2^32 -- where the library's times live (total < 2^30)
    T = cases[1][0]
    assert _first_difference(T, probe_times(T, rng, n_uniform=2000)) is None
