"""Every device and pinned allocation of the library goes through one owner type that counts (svsdf_debug_live_allocations).
A context that walked every allocating path of the host layer and was closed must leave the count, and the bytes, exactly
where they were before it was created: a buffer that nobody owns shows up here as a difference."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _live(svsdf_amd):
    gc.collect()          # contexts that earlier tests dropped without close() go now, not in the middle of a lifetime
    return svsdf_amd.live_allocations()


def _traj(svsdf_amd, workload, N, piece_time=None):
    w = workload.make("C1", P=16, N=N, minco=None)
    T = w["T"] if piece_time is None else np.full(N, float(piece_time))
    return svsdf_amd.minco_coeffs(w["head_state"], w["tail_state"], w["q"], T), T


def _table_launches(ctx):
    return [r["targ"][0] for r in ctx.last_launches() if r["kernel"] == "layer_tables"]


def _lifetime(svsdf_amd, workload, shape, n0):
    ctx = svsdf_amd.SvsdfContext(shape=shape, device=0)
    assert svsdf_amd.live_allocations()[0] > n0
    c4, T4 = _traj(svsdf_amd, workload, 4)
    ctx.set_points(workload.make("C1", P=300)["points"])
    for _ in range(2):                                        # (the second evaluation may take the fused tail)
        assert np.isfinite(ctx.eval_penalty(c4, T4)[0])
    ctx.set_points(workload.make("C1", P=3000)["points"])     # every per-point array is allocated again
    if shape == "star":       # pin the layer-2 / 3 pose tables on: the rule leaves so small a cloud without them (and the
        ctx.set_plan(layer_tables=3)                          # Polygon never builds them)
    assert np.isfinite(ctx.eval_penalty(c4, T4)[0])
    assert _table_launches(ctx) == ([3] if shape == "star" else [])
    # 100 pieces of 2.99 s (299 s, under the 300 s duration cap): 1994 scan seeds against the 67 of the first trajectory.
    # Every trajectory-sized buffer is outgrown: the staging pair needs 19 * 100 + 1994 + 2 * 250 = 4394 doubles and holds
    # (19 * 4 + 67 + 2 * 9) + 4096 = 4257, the pose and chunk tables hold 67 + 1024 seeds, the layer tables 67 + 256.
    before = svsdf_amd.live_allocations()
    c100, T100 = _traj(svsdf_amd, workload, 100, piece_time=2.99)
    assert np.isfinite(ctx.eval_penalty(c100, T100)[0])
    assert _table_launches(ctx) == ([3] if shape == "star" else [])
    after = svsdf_amd.live_allocations()
    assert after[0] == before[0] and after[1] > before[1]     # replaced, not added: the same buffers, larger
    rng = np.random.default_rng(3)
    out = ctx.debug_sdf_at(c4, T4, rng.uniform(-3.0, 3.0, (10, 2)), rng.uniform(0.0, float(T4.sum()), 10))
    assert out.shape == (10, 8) and np.isfinite(out).all()
    assert ctx.sqrt_mismatches(np.linspace(1.0, 2.0, 64), 0) == 0
    states = rng.uniform(-1.0, 1.0, (3, 3))
    free = ctx.check_sub_sw_collision(states, states + 0.25, [rng.uniform(-4.0, 4.0, (5, 2)) for _ in range(3)])
    assert free.shape == (3,)
    if shape == "star":    # the front end (the Polygon has no yaw kernels)
        # the 5 x 11 free grid of test_astar_search_gpu.test_small_grids (kernels 3 / 2, resolution 1): the two corner
        # points fix the bounds and stay below the occupancy threshold
        m = svsdf_amd.OccupancyMap(np.array([[0.0, 0.0, 0.0], [5.0, 11.0, 1.0]], dtype=np.float32), resolution=1.0,
                                   sta_threshold=2)
        assert ctx.shape_kernels(3, 2, 1.0, 0.5)[0].shape == (2, 3, 3)
        ctx.frontend_set_map(m, 3, 2, 0.5)
        ok, _, stage = ctx.astar_successors([[0, 0], [1, 1], [2, 5], [4, 10]], np.zeros(4))
        assert ok.shape == (4, 9) and (ok == (stage == 0)).all()
        r = ctx.astar_search([0.5, 0.5, 0.5], [4.5, 10.5, 0.5])
        assert (r["status"], r["path_len"]) == ("FOUND", 11)
        ctx.frontend_set_map(m, 3, 2, 0.5)                    # releases the map and the search state, builds them again
        assert ctx.astar_search([0.5, 0.5, 0.5], [4.5, 10.5, 0.5])["path_len"] == 11
    assert svsdf_amd.live_allocations()[0] > n0
    ctx.close()


@pytest.mark.parametrize("shape", ["star", "Polygon"])
def test_a_closed_context_leaves_no_allocation(built, shape):
    import svsdf_amd
    from svsdf_amd import workload
    n0, b0 = _live(svsdf_amd)
    for _ in range(2):
        _lifetime(svsdf_amd, workload, shape, n0)
        assert svsdf_amd.live_allocations() == (n0, b0)


def test_a_closed_group_leaves_no_allocation(built):
    """Two stripes on one GPU, host combine (as tests/test_multidevice.py runs a group on a single device)."""
    import svsdf_amd
    from svsdf_amd import workload
    n0, b0 = _live(svsdf_amd)
    w = workload.make("C1", P=2000, N=4, minco=svsdf_amd.minco_coeffs)
    grp = svsdf_amd.SvsdfContext(shape="star", devices=[0, 0])
    grp.set_points(w["points"])
    assert np.isfinite(grp.eval_penalty(w["coeffs"], w["T"])[0])
    assert svsdf_amd.live_allocations()[0] > n0
    grp.close()
    assert svsdf_amd.live_allocations() == (n0, b0)
