"""svsdf_scale_bounds on the host: rigorous bounds {Smin, Smax, Imax, Q} of a scale schedule
s_a(t) = c_a + sin(w_a t + phi_a) A_a over a time interval -- the smallest and largest scale factor, the largest 1 / s_a and
the largest |s_a'| / s_a^2 -- which the certified clearance under a schedule rests on ("Under a scale
schedule").  Domination against dense sampling, tightness on short intervals, the special values, every refusal, and the
opt-in flag on a host-only context; and the host header compiled alone with the address and undefined-behaviour sanitizers
into a stand-alone program (tests/cpp/scale_host.cpp), run once.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

SAMPLES = 2001


def _sampled(s, ta, tb):
    """min s, max s, max 1 / s, max |s'| / s^2 over SAMPLES equispaced times of [ta, tb] plus both ends, over both axes."""
    t = np.concatenate([np.linspace(ta, tb, SAMPLES), [ta, tb]])[:, None]
    c, A, w, ph = (np.asarray(s[k], dtype=np.float64)[None, :] for k in ("c", "amp", "omega", "phase"))
    arg = w * t + ph
    sv = c + np.sin(arg) * A
    ds = np.abs(A * w * np.cos(arg))
    return float(sv.min()), float(sv.max()), float((1.0 / sv).max()), float((ds / sv ** 2).max())


def _schedule(rng, amp_share=1.0):
    c = rng.uniform(0.3, 2.0, 2)
    amp = c * rng.uniform(0.0, amp_share, 2) * (1.0 - 1e-9) * rng.choice([-1.0, 1.0], 2)
    w = rng.uniform(-6.0, 6.0, 2)
    kind = rng.integers(0, 8, 2)
    w[kind == 0] = 0.0                 # exactly 0: a constant factor sin(phi) A
    amp[kind == 1] = 0.0               # A = 0: a constant scale
    return dict(c=tuple(c), amp=tuple(amp), omega=tuple(w), phase=tuple(rng.uniform(-10.0, 10.0, 2)))


def test_domination(built):
    """2 000 random (schedule, interval) pairs, widths from 1e-9 s to 20 s (some longer than a period): no sampled value
    escapes its bound."""
    import svsdf_amd
    rng = np.random.default_rng(11)
    longer = 0
    for i in range(2000):
        s = _schedule(rng)
        assert all(abs(a) < c for a, c in zip(s["amp"], s["c"]))
        ta = rng.uniform(0.0, 300.0)
        width = 10.0 ** rng.uniform(-9.0, np.log10(20.0))
        tb = ta + width
        Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(s, ta, tb)
        lo, hi, inv, q = _sampled(s, ta, tb)
        assert lo >= Smin and hi <= Smax and inv <= Imax and q <= Q, (i, s, ta, tb, (Smin, Smax, Imax, Q), (lo, hi, inv, q))
        assert Smin > 0.0 and Smin >= min(c - abs(a) for a, c in zip(s["amp"], s["c"])) * (1 - 1e-9)
        longer += any(abs(w) * width >= 2 * np.pi for w in s["omega"])
    assert longer >= 50, longer


def test_tightness(built):
    """Short intervals around 200 random times: every output within a factor 1 + 20 width (|w|_max + 1) of its sampled
    counterpart; Q, which can be 0, also gets the additive 20 width |A w^2|_max / Smin^2 (the range of |cos| over the
    interval times the largest 1 / s^2)."""
    import svsdf_amd
    rng = np.random.default_rng(12)
    for i in range(200):
        s = _schedule(rng, amp_share=0.9)
        t = rng.uniform(0.0, 300.0)
        for width in (1e-2, 1e-4, 1e-6):
            ta, tb = t - 0.5 * width, t + 0.5 * width
            Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(s, ta, tb)
            lo, hi, inv, q = _sampled(s, ta, tb)
            wmax = max(abs(w) for w in s["omega"])
            f = 1.0 + 20.0 * width * (wmax + 1.0)
            add = 20.0 * width * max(abs(a * w * w) for a, w in zip(s["amp"], s["omega"])) / Smin ** 2
            assert lo >= Smin >= lo / f and hi <= Smax <= hi * f and inv <= Imax <= inv * f, (i, width, s, (Smin, Smax, Imax), (lo, hi, inv))
            assert q <= Q <= q * f + add, (i, width, s, Q, q)


def test_q_is_small_at_an_extremum(built):
    """Centred on the minimum of s_x of the reference's worked example (s_x = 0.2, where 1 / s^2 is largest and cos passes
    through 0): with sup |cos| = 1 the bound would be |A w| / Smin^2 = 22.5; the range of |cos| over the interval gives a
    fraction of it."""
    import svsdf_amd
    ex = svsdf_amd.binding.EXAMPLE_SCALE
    t_star = (-0.5 * np.pi - ex["phase"][0] + 2 * np.pi) / ex["omega"][0]      # sin(w t + phi) = -1
    Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(ex, t_star - 0.01, t_star + 0.01)
    lo, hi, inv, q = _sampled(ex, t_star - 0.01, t_star + 0.01)
    aw = max(abs(a * w) for a, w in zip(ex["amp"], ex["omega"]))
    print("Smin", Smin, "Q", Q, "sampled", q, "sup-|cos| = 1 form", aw / Smin ** 2)
    assert abs(Smin - 0.2) < 1e-9 and lo >= Smin
    assert q <= Q <= 0.2 * aw / Smin ** 2, (Q, q)
    # a random extremum of each kind: |cos| = 0 inside the interval, Q within the additive term of the sampled value
    rng = np.random.default_rng(13)
    for i in range(50):
        s = _schedule(rng, amp_share=0.9)
        if s["omega"][0] == 0.0 or s["amp"][0] == 0.0:
            continue
        k = int(rng.integers(0, 40))
        t0 = ((0.5 + k) * np.pi - s["phase"][0]) / s["omega"][0]
        width = 1e-3
        Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(s, t0 - 0.5 * width, t0 + 0.5 * width)
        lo, hi, inv, q = _sampled(s, t0 - 0.5 * width, t0 + 0.5 * width)
        add = 20.0 * width * max(abs(a * w * w) for a, w in zip(s["amp"], s["omega"])) / Smin ** 2
        assert q <= Q <= q * (1.0 + 20.0 * width * (max(abs(w) for w in s["omega"]) + 1.0)) + add, (i, s, Q, q)
        assert lo >= Smin and hi <= Smax and inv <= Imax


def test_special_values(built):
    import svsdf_amd
    ident = (1.0, 1.0, 1.0, 0.0)
    assert svsdf_amd.scale_bounds(None, 0.0, 5.0) == ident
    assert svsdf_amd.scale_bounds(svsdf_amd.binding.EXAMPLE_SCALE, 0.0, 5.0, enabled=False) == ident
    assert svsdf_amd.scale_bounds(dict(c=(1.0, 1.0), amp=(0.0, 0.0), omega=(3.0, -2.0), phase=(0.5, 0.1)), 1.0, 9.0) == ident
    # a disabled schedule is not validated beyond its size, as in svsdf_set_scale
    assert svsdf_amd.scale_bounds(dict(c=(0.0, 0.0)), 0.0, 1.0, enabled=False) == ident
    # a constant anisotropic scale: the factors themselves
    Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(dict(c=(1.3, 0.6)), 0.0, 7.0)
    assert (Smin, Smax, Q) == (0.6, 1.3, 0.0) and 1.0 / 0.6 <= Imax <= (1.0 / 0.6) * (1 + 1e-11)
    # ta == tb: the point value
    ex = svsdf_amd.binding.EXAMPLE_SCALE
    Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(ex, 2.0, 2.0)
    lo, hi, inv, q = _sampled(ex, 2.0, 2.0)
    assert lo >= Smin >= lo * (1 - 1e-9) and hi <= Smax <= hi * (1 + 1e-9) and inv <= Imax <= inv * (1 + 1e-9) and q <= Q <= q * (1 + 1e-9)
    # a whole period: the full range
    Smin, Smax, Imax, Q = svsdf_amd.scale_bounds(ex, 1.0, 1.0 + 2 * np.pi / 1.5 + 1e-9)
    assert abs(Smin - 0.2) < 1e-9 and abs(Smax - 1.4) < 1e-9 and abs(Imax - 5.0) < 1e-8


def test_refusals(built):
    import svsdf_amd
    ex = svsdf_amd.binding.EXAMPLE_SCALE
    E = svsdf_amd.SvsdfError
    with pytest.raises(E, match=r"svsdf_scale_bounds failed \(1\).*struct_size"):
        svsdf_amd.scale_bounds(ex, 0.0, 1.0, struct_size=8)
    for name in ("c", "amp", "omega", "phase"):
        for bad in (float("nan"), float("inf")):
            s = dict(ex); s[name] = (ex[name][0], bad)
            with pytest.raises(E, match=r"svsdf_scale_bounds failed \(1\).*non-finite"):
                svsdf_amd.scale_bounds(s, 0.0, 1.0)
    for s in (dict(ex, amp=(0.8, 0.4)), dict(ex, amp=(0.6, -0.9)), dict(ex, c=(0.0, 0.8), amp=(0.0, 0.4)), dict(ex, c=(-1.0, 0.8))):
        with pytest.raises(E, match=r"svsdf_scale_bounds failed \(1\).*singular"):
            svsdf_amd.scale_bounds(s, 0.0, 1.0)
    for ta, tb in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(E, match=r"svsdf_scale_bounds failed \(1\).*ta <= tb"):
            svsdf_amd.scale_bounds(ex, ta, tb)
        with pytest.raises(E, match=r"svsdf_scale_bounds failed \(1\)"):
            svsdf_amd.scale_bounds(None, ta, tb)
    L = svsdf_amd.lib()
    assert L.svsdf_scale_bounds(None, 0.0, 1.0, None) == 1                      # a null out4


def test_flag_on_a_host_only_context(built):
    import svsdf_amd
    assert svsdf_amd.FLAG_SCALED_CLEARANCE == 32 and "FLAG_SCALED_CLEARANCE" in svsdf_amd.__all__
    assert "scale_bounds" in svsdf_amd.__all__
    ctx = svsdf_amd.SvsdfContext(shape="star", flags=svsdf_amd.FLAG_HOST_ONLY | svsdf_amd.FLAG_SCALED_CLEARANCE)
    T = np.array([1.1, 0.9, 1.3])
    coeffs = np.random.default_rng(3).normal(0.0, 1.0, (18, 3))
    for sched in (None, svsdf_amd.binding.EXAMPLE_SCALE):
        if sched:
            ctx.set_scale(**sched)
        with pytest.raises(svsdf_amd.SvsdfError, match=r"svsdf_min_clearance failed \(2\)"):       # SVSDF_ERR_NO_DEVICE
            ctx.min_clearance(coeffs, T)
        with pytest.raises(svsdf_amd.SvsdfError, match=r"svsdf_point_clearance failed \(2\)"):
            ctx.point_clearance(coeffs, T)
    ctx.close()
    assert C.sizeof(svsdf_amd.binding.Scale) == 72


def test_scale_host_under_sanitizers(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "scale_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(here, "cpp", "scale_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert out.strip().split("\n")[-2:] == ["pairs 400", "all checks passed"]
