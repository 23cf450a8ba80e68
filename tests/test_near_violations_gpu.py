"""The near form of scp_collision_violations_at (scp_near.hip: only the pairs close enough to be violated, a uniform grid
per time step) against the pass with the near form switched off, from identical inputs: the same row list, count, bits
of max_violation and working-set bitmap, and a clean scratch map.  Shapes are the smallest at which each mechanism of the
kernel can fail; scp_ctx_set_near_pass(2) takes the kernel to them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0.8
TAU = 1e-6  # SCP_NEAR_TAU


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def cloud(N, K, D, seed, side=None, step=0.3):
    """seeded positions in a box with neighbours about R apart, and new positions a few tenths of R away"""
    rng = np.random.default_rng(seed)
    side = 1.2 * N ** (1.0 / D) if side is None else side
    prev = rng.uniform(0.0, side, (N, K, D))
    new = prev + step * R * rng.standard_normal((N, K, D))
    return prev, new


def reach_side(prev, new, k):
    """the cell side the kernel uses at step k: (R + 2 max |dP| + tau) (1 + 1e-6)"""
    m = np.sqrt(((new - prev)[:, k] ** 2).sum(-1)) * (1.0 + 1e-10)
    return (R + 2.0 * m.max() + TAU) * (1.0 + 1e-6)


def make_case(name):
    """-> dict(prev, new, and optionally q (begin, end), premark (fraction of the exhaustive list), cap, feas, fallback)"""
    if name == "one_pair":
        prev = np.array([[[1.0, 1.0]], [[1.5, 1.4]]])
        new = prev + np.array([[[0.1, 0.05]], [[-0.1, -0.02]]])
        return dict(prev=prev, new=new)
    if name == "n3_k2":
        prev, new = cloud(3, 2, 2, 11, side=1.5)
        return dict(prev=prev, new=new)
    if name == "n33_2d":
        prev, new = cloud(33, 3, 2, 12)
        return dict(prev=prev, new=new)
    if name == "n33_3d":
        prev, new = cloud(33, 3, 3, 13, side=2.6)
        return dict(prev=prev, new=new)
    if name == "n130_k7":  # three workgroups per time step, ~5 agents per cell
        prev, new = cloud(130, 7, 2, 14)
        return dict(prev=prev, new=new)
    if name == "n130_3d":
        prev, new = cloud(130, 2, 3, 15, side=4.5)
        return dict(prev=prev, new=new)
    if name == "range_inside_rows":  # row 0 of the triangle has 32 pairs: 40 and 300 lie inside rows 1 and 10
        prev, new = cloud(33, 3, 2, 16)
        return dict(prev=prev, new=new, q=(40, 300))
    if name == "empty_range":
        prev, new = cloud(33, 3, 2, 17)
        return dict(prev=prev, new=new, q=(100, 100), fallback=None)
    if name == "coincident":
        prev, new = cloud(33, 3, 2, 18)
        prev[1] = prev[0]
        prev[7, 1] = prev[20, 1]
        return dict(prev=prev, new=new)
    if name == "one_cell":
        prev, new = cloud(20, 2, 2, 19, side=1.0)
        return dict(prev=prev, new=new)
    if name == "one_cell_3d":
        prev, new = cloud(20, 2, 3, 20, side=1.0)
        return dict(prev=prev, new=new)
    if name == "cell_edges":  # agents on the arena's minimum corner, exactly on and next to cell edges
        prev, new = cloud(60, 2, 2, 21, side=9.0)
        delta = 0.2 * R * np.sign(new - prev)  # (every |dP| the same: the side is known)
        new = prev + delta
        for k in range(2):
            s = reach_side(prev, new, k)
            lo = prev[:, k].min(0)
            prev_k = prev[:, k]
            prev_k[0] = lo
            prev_k[1] = lo + [s, 0.0]
            prev_k[2] = lo + [2.0 * s, s]
            prev_k[3] = lo + [np.nextafter(s, 0.0), 0.3]
            prev_k[4] = lo + [np.nextafter(s, 9.0) + 0.5, 0.4]
            prev_k[5] = lo + [s - 0.6, 0.1]
            prev_k[6] = lo + [0.3, 0.3]
        return dict(prev=prev, new=prev + delta)
    if name == "huge_step":  # one agent moves 100 m: the grid collapses to one cell
        prev, new = cloud(40, 2, 2, 22)
        new[5, 0] += [100.0, -60.0]
        return dict(prev=prev, new=new)
    if name == "premarked":
        prev, new = cloud(130, 3, 2, 23)
        return dict(prev=prev, new=new, premark=0.5)
    if name == "short_list":
        prev, new = cloud(33, 3, 2, 24)
        return dict(prev=prev, new=new, cap=1)
    if name == "far_apart":  # nothing near anything and dP = 0: the maximum R - 5 is far below -tau / 2
        g = 5.0 * np.stack(np.meshgrid(np.arange(4.0), np.arange(3.0), indexing="ij"), -1).reshape(12, 1, 2)
        prev = np.repeat(g, 2, axis=1)
        return dict(prev=prev, new=prev.copy(), fallback=True)
    if name in ("nan", "inf"):
        prev, new = cloud(33, 3, 2, 25)
        new[4, 1, 0] = np.nan if name == "nan" else np.inf
        return dict(prev=prev, new=new, fallback=True)
    if name == "inf_prev":
        prev, new = cloud(33, 3, 2, 26)
        prev[9, 2, 1] = -np.inf
        return dict(prev=prev, new=new, fallback=True)
    raise KeyError(name)


def run_pass(ctx, mode, prev_t, new_t, N, K, D, q, feas, cap, premark_words):
    import torch

    nq = q[1] - q[0]
    words = max((K * nq + 31) // 32, 1)
    bitmap = torch.zeros(words, dtype=torch.int32, device=ctx.tdev)
    if premark_words is not None:
        bitmap.copy_(torch.as_tensor(premark_words.view(np.int32)))
    sel = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=ctx.tdev)
    ctx.set_near_pass(mode)
    before = ctx.near_pass_counts()
    ctx.check(ctx.lib.scp_collision_violations_at(ctx.h, N, K, D, R, q[0], q[1], prev_t.data_ptr(), new_t.data_ptr(), feas,
                                                  sel.data_ptr(), cap, bitmap.data_ptr(), ctx.stats.data_ptr()))
    stats = ctx.stats.cpu().numpy().view(np.uint64).copy()
    after = ctx.near_pass_counts()
    return dict(rows=sel.cpu().numpy(), n=int(stats[2]), max_bits=int(stats[3]), bitmap=bitmap.cpu().numpy().view(np.uint32),
                scratch=ctx.peek_scratch_map((K * nq + 31) // 32), near=after[0] - before[0], fell_back=after[1] - before[1])


CASES = ["one_pair", "n3_k2", "n33_2d", "n33_3d", "n130_k7", "n130_3d", "range_inside_rows", "empty_range", "coincident",
         "one_cell", "one_cell_3d", "cell_edges", "huge_step", "premarked", "short_list", "far_apart", "nan", "inf", "inf_prev"]


@pytest.mark.parametrize("name", CASES)
def test_near_pass_equals_the_exhaustive_pass(ctx, name):
    c = make_case(name)
    prev, new = c["prev"], c["new"]
    N, K, D = prev.shape
    q = c.get("q", (0, N * (N - 1) // 2))
    feas = c.get("feas", 1e-6)
    prev_t, new_t = ctx.tensor(prev), ctx.tensor(new)
    try:
        full = run_pass(ctx, 0, prev_t, new_t, N, K, D, q, feas, 1 << 16, None)  # the whole list, nothing pre-marked
        premark = None
        if "premark" in c:  # every other row of the exhaustive list is in the working set already
            premark = np.zeros(max((K * (q[1] - q[0]) + 31) // 32, 1), dtype=np.uint32)
            pairs = N * (N - 1) // 2
            for r in full["rows"][:full["n"]:2]:
                lr = (r // pairs) * (q[1] - q[0]) + (r % pairs - q[0])
                premark[lr >> 5] |= np.uint32(1 << (lr & 31))
        cap = c.get("cap", 1 << 16)
        off = run_pass(ctx, 0, prev_t, new_t, N, K, D, q, feas, cap, premark)
        on = run_pass(ctx, 2, prev_t, new_t, N, K, D, q, feas, cap, premark)
    finally:
        ctx.set_near_pass(1)
    fallback = c.get("fallback", False)
    print(f"{name}: n_selected={on['n']} (exhaustive {off['n']}) max bits {on['max_bits']:#x} / {off['max_bits']:#x} "
          f"near={on['near']} fell_back={on['fell_back']}")
    assert off["near"] == 0
    if fallback is None:  # an empty pair range: no pass runs at all
        assert on["near"] == 0 and on["n"] == 0
    else:
        assert on["near"] == 1 and on["fell_back"] == (1 if fallback else 0)
        if not fallback:  # (a kernel that marks nothing cannot pass)
            assert off["n"] > 0 and (premark is None or 0 < off["n"] < full["n"])
    np.testing.assert_array_equal(on["rows"], off["rows"])
    assert on["n"] == off["n"]
    assert on["max_bits"] == off["max_bits"]
    np.testing.assert_array_equal(on["bitmap"], off["bitmap"])
    assert not on["scratch"].any() and not off["scratch"].any()
    if "cap" in c:  # nothing stored, nothing merged, the count reported
        assert on["n"] > c["cap"] and (on["rows"] == -1).all() and not on["bitmap"].any()


def test_auto_mode_keeps_the_one_launch_form_for_small_problems(ctx):
    prev, new = cloud(33, 3, 2, 12)
    prev_t, new_t = ctx.tensor(prev), ctx.tensor(new)
    q = (0, 33 * 32 // 2)
    try:
        off = run_pass(ctx, 0, prev_t, new_t, 33, 3, 2, q, 1e-6, 1 << 16, None)
        auto = run_pass(ctx, 1, prev_t, new_t, 33, 3, 2, q, 1e-6, 1 << 16, None)
    finally:
        ctx.set_near_pass(1)
    assert auto["near"] == 0 and auto["n"] == off["n"] > 0
    np.testing.assert_array_equal(auto["rows"], off["rows"])
    assert auto["max_bits"] == off["max_bits"]


def test_auto_mode_takes_the_near_form_for_large_problems(ctx):
    """700 agents x 10 steps (2.4 M rows) is past the one-launch passes: auto mode runs the near kernel (11 workgroups per
    time step, the three-launch compaction), and a negative feas_tol keeps the exhaustive pass."""
    N, K = 700, 10
    prev, new = cloud(N, K, 2, 31)
    prev_t, new_t = ctx.tensor(prev), ctx.tensor(new)
    q = (0, N * (N - 1) // 2)
    try:
        off = run_pass(ctx, 0, prev_t, new_t, N, K, 2, q, 1e-6, 1 << 16, None)
        auto = run_pass(ctx, 1, prev_t, new_t, N, K, 2, q, 1e-6, 1 << 16, None)
        neg = run_pass(ctx, 1, prev_t, new_t, N, K, 2, q, -1e-3, 1 << 16, None)
    finally:
        ctx.set_near_pass(1)
    assert (auto["near"], auto["fell_back"], neg["near"]) == (1, 0, 0)
    assert auto["n"] == off["n"] > 0 and neg["n"] > off["n"]
    np.testing.assert_array_equal(auto["rows"], off["rows"])
    assert auto["max_bits"] == off["max_bits"]
    np.testing.assert_array_equal(auto["bitmap"], off["bitmap"])
    assert not auto["scratch"].any()


def test_forced_near_pass_solve_is_bit_identical():
    """a complete 40-agent solve with the near pass forced against off: the same accelerations, rounds and working rows"""
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP

    p0, pf, space = generate_grid_swap(40, seed=40000)
    out = []
    for mode in (0, 2):
        s = SCP(40, 10.0, 0.2, R, space, verbose=False)
        s._ctx.set_near_pass(mode)
        before = s._ctx.near_pass_counts()
        s.set_initial_states(p0)
        s.set_final_states(pf)
        traj = s.generate_trajectories(15)
        out.append((traj, s.last_info, s._ctx.near_pass_counts()[0] - before[0]))
    (t0, i0, n0), (t2, i2, n2) = out
    assert n0 == 0 and n2 > 0
    for key in ("accelerations", "positions", "velocities"):
        np.testing.assert_array_equal(t2[key], t0[key])
    assert i0["n_iterations"] == i2["n_iterations"] and len(i0["iterations"]) == len(i2["iterations"])
    for a, b in zip(i0["iterations"], i2["iterations"]):
        assert (a["rounds"], a["working_rows"], a["added"], a["iter"]) == (b["rounds"], b["working_rows"], b["added"], b["iter"])
