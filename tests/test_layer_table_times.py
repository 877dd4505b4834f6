"""The keying claim behind the pose tables of scan layers 2 and 3 (k_layer_tables), checked without a
GPU: the sample times choiceTInit visits in layer 2 are a function of the layer-1 winner's index best_k alone, those of
layer 3 of (best_k, w2) with w2 = layer 2's winning sample or "none beat the carried minimum".

The independent restatement (tests/golden/make_golden.py, imported unchanged; its sdf_at wrapped so that every visited
time is recorded) runs choice_t_init for a few hundred query points of a random 32-piece trajectory, with coarse and with
generic piece durations, points near both trajectory ends included (windows clamped at 0 and at the duration).  The two
time sequences are rebuilt here from best_k / (best_k, w2) with the additions the table kernel makes -- t0, then += dt one
at a time; dt = 0.15, *= 0.1 per layer -- and compared float for float with what the restatement visited."""
import importlib.util
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    spec = importlib.util.spec_from_file_location("make_golden_layer_times", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def window(seed, dt, dur):
    """times of one layer's window around `seed`: t0 = max(0, seed - 10 dt), += dt while t <= min(dur, seed + 10 dt)"""
    t, terminal, out = max(0.0, seed - 10 * dt), min(dur, seed + 10 * dt), []
    while t <= terminal:
        out.append(t)
        t += dt
    return out


def table_rows(tk, dur):
    """What the table kernel holds, as times: row2[k] the layer-2 window of seed k; row3[k][w2 + 1] the layer-3 window after
    hand-over w2 (-1: the seed itself)."""
    dt2 = 0.15
    dt2 *= 0.1
    dt3 = dt2
    dt3 *= 0.1
    row2 = [window(s, dt2, dur) for s in tk]
    row3 = [[window(s, dt3, dur)] + [window(t, dt3, dur) for t in row2[k]] for k, s in enumerate(tk)]
    return row2, row3


def _trajectory(g, rng, generic):
    N = 32
    durs = [2.5] * N
    if generic:
        durs = [2.5 * (0.7 + 0.6 * rng.random()) for _ in range(N)]
    rows = [[rng.uniform(-1.0, 1.0) * (0.5 ** (r % 6)) * (4.0 if r % 6 == 0 else 1.0) for _ in range(3)] for r in range(6 * N)]
    return g.Traj(rows, durs)


@pytest.mark.parametrize("generic", [False, True], ids=["coarse", "generic"])
def test_layer_times_follow_from_the_seed_index(generic):
    g = _golden()
    rng = random.Random(20260 + int(generic))
    traj = _trajectory(g, rng, generic)
    sw = g.Swept(g.Shape("sdHorseshoe"), traj)
    dur = sw.dur
    tk, t = [], 0.0
    while t <= dur:
        tk.append(t)
        t += 0.15
    K = len(tk)
    assert K > 500
    row2, row3 = table_rows(tk, dur)
    assert max(len(r) for r in row2) <= 21 and max(len(r) for rs in row3 for r in rs) <= 21
    assert all(len(rs) <= 22 for rs in row3)

    visited = []
    plain = sw.sdf_at

    def recording(px, py, t):
        d = plain(px, py, t)
        visited.append((t, d))
        return d

    sw.sdf_at = recording
    # query points: around poses all along the path, and a share right at its two ends (clamped windows)
    queries = []
    for i in range(300):
        u = rng.random()
        tq = (0.02 * u * dur) if i % 5 == 0 else (dur - 0.02 * u * dur) if i % 5 == 1 else u * dur
        p = traj.pos(tq)
        queries.append((p[0] + rng.uniform(-1.5, 1.5), p[1] + rng.uniform(-1.5, 1.5)))
    none_won, first_seed, last_seed = 0, 0, 0
    for px, py in queries:
        del visited[:]
        seed = sw.choice_t_init(px, py, 0.15)
        assert [t for t, _ in visited[:K]] == tk                     # layer 1 is the table k_prep already holds
        min_dis, best_k = 1e9, None
        for k, (_, d) in enumerate(visited[:K]):
            if d < min_dis:
                min_dis, best_k = d, k
        assert best_k is not None
        first_seed += best_k == 0
        last_seed += best_k == K - 1
        want2 = row2[best_k]
        got2 = visited[K:K + len(want2)]
        assert [t for t, _ in got2] == want2, (best_k, want2, got2)
        w2 = -1
        for i, (_, d) in enumerate(got2):
            if d < min_dis:
                min_dis, w2 = d, i
        none_won += w2 < 0
        want3 = row3[best_k][w2 + 1]
        got3 = visited[K + len(want2):K + len(want2) + len(want3)]
        assert [t for t, _ in got3] == want3, (best_k, w2, want3, got3)
        # what is left is layer 4 around layer 3's winner, and it ends where the restatement's seed says
        seed3 = tk[best_k] if w2 < 0 else want2[w2]
        for t3, d in got3:
            if d < min_dis:
                min_dis, seed3 = d, t3
        dt4 = 0.15
        for _ in range(3):
            dt4 *= 0.1
        want4 = window(seed3, dt4, dur)
        got4 = visited[K + len(want2) + len(want3):]
        assert [t for t, _ in got4] == want4
        for t4, d in got4:
            if d < min_dis:
                min_dis, seed3 = d, t4
        assert seed3 == seed
    assert none_won > 0          # the hand-over "no sample of layer 2 wins" occurs
    assert first_seed > 0 and last_seed > 0   # windows clamped at 0 and at the duration were visited
