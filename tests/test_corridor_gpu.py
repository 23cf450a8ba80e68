"""Static obstacles on the GPU: the summed table, corridor boxes, state boxes, the bound overwrite and the corridor check
against tests/corridor_ref.py (integers exactly, doubles bit for bit), the pipeline choice and the QP with boxes against the
explicit-matrix oracle, and an end-to-end solve around a disc."""
import numpy as np
import pytest
import scipy.sparse as sp

import corridor_cases as cc
import corridor_ref as cr
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

pytestmark = pytest.mark.gpu

LIMITS = [-2.0, 2.0, -15.0, 15.0, -20.0, 20.0]
GRIDS = [((37, 29), 2), ((300, 70), 2), ((13, 11, 9), 3)]


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _torch():
    import torch

    return torch


def _grid(D, origin, cell, occ):
    from path_planning import _hip

    return _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])


def _itensor(ctx, a):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(ctx.tdev)


_CASES = {}


def _case(dims, D, N=5, K=7):
    """a random grid (about 8 % occupied), a random-walk reference through free cells and the reference's summed table"""
    key = (dims, D, N, K)
    if key not in _CASES:
        rng = np.random.default_rng(17 + len(dims) + dims[0])
        occ = cc.random_grid(rng, dims)
        origin, cell = [-1.5, 0.25, 2.0][:D], 0.4
        ref = cc.random_walk_reference(rng, occ, D, origin, cell, N, K)
        _CASES[key] = (occ, origin, cell, ref, cr.summed_table(occ))
    return _CASES[key]


@pytest.mark.parametrize("dims,D", GRIDS + [((1, 130), 2), ((65, 1), 2)])
def test_summed_table(ctx, dims, D):
    occ = cc.random_grid(np.random.default_rng(dims[0]), dims, 0.3)
    _, sat = ctx.occupancy_prepare(D, _grid(D, [0.0] * D, 1.0, occ), occ)
    want = occ.astype(np.int64)
    for ax in range(3):
        want = np.cumsum(want, axis=ax)
    np.testing.assert_array_equal(sat.cpu().numpy(), want)


def test_grid_errors(ctx):
    from path_planning import _hip

    occ = np.zeros((1, 4, 4), dtype=np.uint8)
    torch = _torch()
    d_occ = torch.zeros((1, 4, 4), dtype=torch.uint8, device=ctx.tdev)
    sat = torch.zeros((1, 4, 4), dtype=torch.int32, device=ctx.tdev)
    for bad in (dict(cell=0.0), dict(cell=np.inf), dict(dims=(4, 4, 2)), dict(dims=(0, 4, 1)), dict(dims=(4096, 4096, 2), D=3),
                dict(origin=[np.nan, 0.0])):
        g = _hip.occupancy_grid(2, bad.get("origin", [0.0, 0.0]), bad.get("cell", 1.0), bad.get("dims", (4, 4, 1)))
        assert ctx.lib.scp_occupancy_prepare(ctx.h, bad.get("D", 2), g, d_occ.data_ptr(), sat.data_ptr()) == -1
        assert ctx.lib.scp_last_error(ctx.h)
    g = _grid(2, [0.0, 0.0], 1.0, occ)
    ref = ctx.tensor(np.full((1, 3, 2), 0.5))
    with pytest.raises(_hip.HipError):
        ctx.corridor_boxes(1, 2, 2, g, sat, ref, 1025)
    with pytest.raises(_hip.HipError):
        ctx.corridor_boxes(1, 2, 2, g, sat, ref, -1)
    cells, _ = ctx.corridor_boxes(1, 2, 2, g, sat, ref, 0)
    with pytest.raises(_hip.HipError):
        ctx.corridor_state_boxes(1, 2, 2, g, cells, -0.1)


@pytest.mark.parametrize("dims,D", GRIDS)
def test_boxes_and_state_boxes_equal_the_reference(ctx, dims, D):
    occ, origin, cell, ref, sat_ref = _case(dims, D)
    N, K = ref.shape[0], ref.shape[1] - 1
    g = _grid(D, origin, cell, occ)
    _, sat = ctx.occupancy_prepare(D, g, occ)
    np.testing.assert_array_equal(sat.cpu().numpy(), sat_ref)
    for max_grow in (0, 1, 3, 8):
        cells, n_blocked = ctx.corridor_boxes(N, K, D, g, sat, ctx.tensor(ref), max_grow)
        want, want_blocked = cr.corridor_boxes(D, origin, cell, sat_ref, ref, max_grow)
        np.testing.assert_array_equal(cells.cpu().numpy(), want)
        assert int(n_blocked.item()) == want_blocked
        for shrink in (0.0, 0.07, 0.45):  # (0.45: more than half a cell -- one-cell intersections empty out)
            lo, hi, n_open = ctx.corridor_state_boxes(N, K, D, g, cells, shrink)
            wlo, whi, wopen = cr.state_boxes(D, origin, cell, want, shrink)
            np.testing.assert_array_equal(lo.cpu().numpy().view(np.uint64), wlo.view(np.uint64))
            np.testing.assert_array_equal(hi.cpu().numpy().view(np.uint64), whi.view(np.uint64))
            assert int(n_open.item()) == wopen
        if max_grow == 3:
            assert want_blocked > 0 or D == 2  # (diagonal steps of the walk span occupied cells)
            assert cr.state_boxes(D, origin, cell, want, 0.45)[2] > cr.state_boxes(D, origin, cell, want, 0.0)[2]


def test_forced_box_cases(ctx):
    occ = np.zeros((1, 6, 8), dtype=np.uint8)
    occ[0, 2, 3] = 1
    origin, cell = [0.0, 0.0], 1.0
    ref = np.array([
        [[0.5, 0.5], [1.5, 0.5], [3.5, 2.5]],     # second segment: a seed on the occupied cell
        [[0.5, 0.5], [-0.5, 0.5], [0.5, 0.5]],    # a reference point outside the grid
        [[0.5, 0.5], [np.nan, 0.5], [0.5, 0.5]],  # a NaN coordinate
        [[2.5, 1.5], [4.5, 3.5], [4.5, 3.5]],     # a seed range that spans the occupied cell; then a free seed
        [[7.5, 5.5], [7.5, 5.5], [8.0, 5.5]],     # the last cell; x = 8.0 is outside
        [[0.5, 0.5], [np.inf, 0.5], [1e300, -1e300]],
    ])
    for grid_occ in (occ, np.zeros_like(occ)):  # (the second: an all-free grid, every box reaches every face)
        g = _grid(2, origin, cell, grid_occ)
        _, sat = ctx.occupancy_prepare(2, g, grid_occ)
        for max_grow in (0, 2, 8, 1024):
            cells, n_blocked = ctx.corridor_boxes(ref.shape[0], 2, 2, g, sat, ctx.tensor(ref), max_grow)
            want, want_blocked = cr.corridor_boxes(2, origin, cell, cr.summed_table(grid_occ), ref, max_grow)
            np.testing.assert_array_equal(cells.cpu().numpy(), want)
            assert int(n_blocked.item()) == want_blocked
    assert (want[0, 0] == [0, 0, 0, 7, 5, 0]).all() and want_blocked == 7  # (the last round: all free, max_grow 1024)


def _qp(ctx, prob, **kw):
    from path_planning import _hip

    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**kw))
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    return qp


def bound_overwrite_case(D):
    """(prob, space, lo, hi): a small problem with non-zero start velocities and a random box pattern with -inf / +inf
    entries and boxes wider than the workspace [0, 20]^D (also the oracle's pattern: tests/test_oracle_boxes_cpu.py)"""
    rng = np.random.default_rng(D)
    N, K, h = 3, 6, 0.3
    space = [0.0] * D + [20.0] * D
    p0, pf = rng.uniform(2, 18, (N, D)), rng.uniform(2, 18, (N, D))
    v0 = rng.normal(0, 0.5, (N, D))
    prob = so.make_problem(N, (K + 0.5) * h, h, 0.5, space, p0, pf, v0=v0)
    assert prob.K == K
    lo = rng.uniform(-5, 12, (N, K, D))
    hi = lo + rng.uniform(0.1, 15, (N, K, D))
    lo[rng.random((N, K, D)) < 0.2] = -np.inf
    hi[rng.random((N, K, D)) < 0.2] = np.inf
    return prob, space, lo, hi


@pytest.mark.parametrize("D", [2, 3])
def test_bound_overwrite_bit_for_bit(ctx, D):
    prob, space, lo, hi = bound_overwrite_case(D)
    N, K, h = prob.N, prob.K, prob.h
    qp = _qp(ctx, prob)
    base = {k: qp.peek(k).cpu().numpy().copy() for k in ("lf", "uf")}
    C = N * D
    assert base["lf"].size == (4 * K - 1) * C
    qp.set_position_boxes(ctx.tensor(lo), ctx.tensor(hi))
    got = {k: qp.peek(k).cpu().numpy().reshape(4 * K - 1, C) for k in ("lf", "uf")}
    wl, wu = cr.position_rows(K, h, space, prob.p0, prob.v0, lo, hi)
    r0 = 3 * K - 1
    for k, want in (("lf", wl), ("uf", wu)):
        np.testing.assert_array_equal(got[k][r0:r0 + K - 1].view(np.uint64), want.view(np.uint64))
        keep = base[k].reshape(4 * K - 1, C)
        np.testing.assert_array_equal(got[k][:r0].view(np.uint64), keep[:r0].view(np.uint64))          # jerk, acc, vel
        np.testing.assert_array_equal(got[k][r0 + K - 1].view(np.uint64), keep[r0 + K - 1].view(np.uint64))  # final position
        assert not np.array_equal(got[k], keep)
    # all-infinite boxes reproduce set_problem bit for bit; set_problem clears the boxes
    for boxes in ((np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)), None):
        qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
        if boxes:
            qp.set_position_boxes(ctx.tensor(boxes[0]), ctx.tensor(boxes[1]))
        for k in ("lf", "uf"):
            np.testing.assert_array_equal(qp.peek(k).cpu().numpy().view(np.uint64), base[k].view(np.uint64))
    qp.set_position_boxes(None, None)  # a no-op
    with pytest.raises(ValueError):
        qp.set_position_boxes(ctx.tensor(lo), None)
    with pytest.raises(ValueError):
        qp.set_position_boxes(ctx.tensor(lo[:, 1:]), ctx.tensor(hi[:, 1:]))
    qp.close()


def test_pipeline_choice_with_boxes(ctx):
    """a QP with boxes never runs a lean persistent kernel (they re-derive the bounds from space and the states)"""
    torch = _torch()
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(16, 0.8, seed=3)
    prob = so.make_problem(16, 10.0, 0.2, 0.8, [0, 0, 20, 20], p0, pf)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(cg_iters=3, eps_abs=1e-6, eps_rel=1e-6))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    assert W.size > 0
    N, K, D = prob.N, prob.K, prob.D
    lo, hi = ctx.tensor(np.full((N, K, D), -1.0)), ctx.tensor(np.full((N, K, D), 21.0))  # (wider than the workspace)
    space = np.concatenate([prob.pos_min, prob.pos_max])
    states = (ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))

    def solve(qp):
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        return qp.solve()

    sols = {}
    for persistent, lean in ((1, "persistent8-lean"), (2, "persistent16"), (3, "persistent8-lean")):
        qp = _qp(ctx, prob, cg_iters=1, persistent=persistent)
        info = solve(qp)
        assert lean in info["pipeline"].split("+") and info["status_val"] == 1
        sols[persistent, "lean"] = qp.solution().cpu().numpy()
        qp.set_position_boxes(lo, hi)
        info = solve(qp)
        pipes = info["pipeline"].split("+")
        assert "persistent" in pipes and "persistent16" not in pipes and "persistent8-lean" not in pipes, info
        assert info["status_val"] == 1
        sols[persistent, "boxes"] = qp.solution().cpu().numpy()
        qp.set_problem(LIMITS, space, *states)  # a fresh problem: lean again
        info = solve(qp)
        assert lean in info["pipeline"].split("+")
        np.testing.assert_array_equal(qp.solution().cpu().numpy(), sols[persistent, "lean"])
        # a clone carries the boxes along
        qp.set_position_boxes(lo, hi)
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        from path_planning import _hip

        twin = _hip.QP(ctx, N, K, D, prob.h, qp.settings)
        twin.take_state_of(qp)
        pipes = twin.solve()["pipeline"].split("+")
        assert "persistent" in pipes and "persistent16" not in pipes and "persistent8-lean" not in pipes
        twin.close()
        qp.close()
    # boxes wider than the workspace leave the QP as it was: the round-2 kernel's solution, whatever persistent says
    np.testing.assert_array_equal(sols[1, "boxes"], sols[2, "boxes"])
    np.testing.assert_array_equal(sols[1, "boxes"], sols[3, "boxes"])


def boxed_qp_case():
    """ref_problem(4, 1, 10.0, 0.5) of tests/test_qp_gpu.py with a few position rows tightened so that they are active:
    (prob, lo, hi, l, u) with l / u the stacked bounds of so.stack_fixed with the same rows overridden"""
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(4, 0.8, seed=1)
    prob = so.make_problem(4, 10.0, 0.5, 0.8, [0, 0, 20, 20], p0, pf)
    N, K, D = prob.N, prob.K, prob.D
    C, l, u = so.stack_fixed(prob)
    free = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), C, l, u, eps_abs=1e-9, eps_rel=1e-9,
                            max_iter=20000)
    assert free["status_val"] == 1
    nj, na = N * (K - 1) * D, N * K * D
    kp1 = np.arange(1, K + 1, dtype=float)
    off = prob.p0[:, None, :] + (prob.h * kp1)[None, :, None] * prob.v0[:, None, :]
    state = (C[nj + 2 * na:] @ free["x"]).reshape(N, K, D) + off  # state[i, k] = the position of state k + 1
    lo, hi = np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)
    # (one row per (vehicle, coordinate): the columns are independent without collision rows, so each one is active)
    for i, j, d, shift in ((0, 8, 1, -0.3), (0, 15, 0, -0.2), (1, 12, 1, 0.3), (2, 5, 0, 0.2), (3, 14, 0, 0.25)):
        if shift < 0:
            hi[i, j, d] = state[i, j - 1, d] + shift  # the free optimum violates it: active
        else:
            lo[i, j, d] = state[i, j - 1, d] + shift
    lt, ut = cr.position_rows(K, prob.h, np.concatenate([prob.pos_min, prob.pos_max]), prob.p0, prob.v0, lo, hi)
    l2, u2 = l.copy(), u.copy()
    lp, up = l2[nj + 2 * na:].reshape(N, K, D), u2[nj + 2 * na:].reshape(N, K, D)
    lp[:, :K - 1] = lt.reshape(K - 1, N, D).transpose(1, 0, 2)
    up[:, :K - 1] = ut.reshape(K - 1, N, D).transpose(1, 0, 2)
    assert (l2 <= u2).all() and ((l2 != l) | (u2 != u)).sum() == 5
    return prob, lo, hi, C, l2, u2


def test_qp_with_boxes_matches_the_explicit_oracle(ctx):
    torch = _torch()
    prob, lo, hi, C, l, u = boxed_qp_case()
    P = 2 * sp.eye(prob.n, format="csc")
    r = qo.osqp_explicit(P, np.zeros(prob.n), C, l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    assert r["status_val"] == 1
    ax = C @ r["x"]
    tight = (l != so.stack_fixed(prob)[1]) | (u != so.stack_fixed(prob)[2])
    assert (np.minimum(ax - l, u - ax)[tight] < 1e-6).all()  # the tightened rows are active
    d_lo, d_hi = ctx.tensor(lo), ctx.tensor(hi)
    for use_mfma in (1, 0):
        for persistent in (1, 0):
            qp = _qp(ctx, prob, cg_iters=3, eps_abs=1e-8, eps_rel=1e-8, use_mfma=use_mfma, persistent=persistent)
            qp.set_position_boxes(d_lo, d_hi)
            qp.reset(None)
            info = qp.solve()
            x = qp.solution().cpu().numpy()
            qp.close()
            err = np.abs(x.ravel() - r["x"]).max()
            print(f"boxed QP#0 use_mfma={use_mfma} persistent={persistent}: {info['iter']} steps, {info['pipeline']}, "
                  f"max |x - explicit| = {err:.3e}")
            assert info["status_val"] == 1
            np.testing.assert_allclose(x.ravel(), r["x"], rtol=0, atol=1e-7)
    # with working collision rows at eps 1e-6: linearised around the boxed QP#0
    x0 = r["x"].reshape(prob.N, prob.K, prob.D)
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    assert W.size > 0
    A = sp.vstack([C, so.collision_matrix_explicit(prob, eta)[W]], format="csc")
    rc = qo.osqp_explicit(P, np.zeros(prob.n), A, np.hstack([l, l_col[W]]), np.hstack([u, np.full(W.size, np.inf)]),
                          x0=x0.ravel(), eps_abs=1e-9, eps_rel=1e-9, max_iter=100000)
    assert rc["status_val"] == 1
    sols = {}
    for persistent in (1, 0):
        qp = _qp(ctx, prob, cg_iters=1, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, persistent=persistent)
        qp.set_position_boxes(d_lo, d_hi)
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        info = qp.solve()
        sols[persistent] = qp.solution().cpu().numpy()
        qp.close()
        err = np.abs(sols[persistent].ravel() - rc["x"]).max()
        print(f"boxed joint QP persistent={persistent}: {info['iter']} steps, {info['pipeline']}, max |x - explicit| = {err:.3e}")
        assert info["status_val"] == 1 and info["working_rows"] == W.size
        assert info["pipeline"] == ("persistent" if persistent else "three-launch")
        assert err < 5e-4  # eps = 1e-6 ADMM point vs the exact minimiser
    print(f"round-2 persistent vs three-launch: max difference {np.abs(sols[1] - sols[0]).max():.3e}")
    np.testing.assert_allclose(sols[1], sols[0], rtol=0, atol=1e-12)


def test_check_kernel_bit_for_bit(ctx):
    rng = np.random.default_rng(23)
    occ, origin, cell, ref, sat_ref = _case((37, 29), 2)
    D, h = 2, 0.2
    N, K = ref.shape[0], ref.shape[1] - 1
    cells, _ = cr.corridor_boxes(D, origin, cell, sat_ref, ref, 3)
    cells[1, 2] = cells[3, 0] = cr.BLOCKED
    cells[4, :] = cr.BLOCKED  # a vehicle without a judged segment
    L, H = cr.segment_boxes_metres(D, origin, cell, cells)
    pos = ref[:, :K] + rng.normal(0, 0.2, (N, K, D))
    vel = rng.normal(0, 1.5, (N, K, D))
    acc = rng.uniform(-15, 15, (N, K, D))
    acc[0, 1] = 0.0                                   # a = 0: no interior candidate
    vel[0, 2], acc[0, 2] = [1.0, -1.0], [-10.0, 10.0]  # t* = 0.1: an interior extremum in both coordinates
    pos[2, 3], vel[2, 3], acc[2, 3] = [L[2, 3, 0], H[2, 3, 1]], 0.0, 0.0  # exactly on two faces: excess 0
    pos[2, 4] = 0.5 * (L[2, 4] + H[2, 4])
    vel[2, 4], acc[2, 4] = 0.0, 0.0                    # the centre: excess = -half the smaller width
    g = _grid(D, origin, cell, occ)
    for tol in (0.0, 0.3):
        got = ctx.check_corridor(N, K, D, h, g, _itensor(ctx, cells), ctx.tensor(pos), ctx.tensor(vel), ctx.tensor(acc), tol)
        want = cr.check_corridor(D, h, origin, cell, cells, pos, vel, acc, tol)
        for f in ("segment", "n_blocked", "n_outside"):
            np.testing.assert_array_equal(got[f], want[f], err_msg=f)
        np.testing.assert_array_equal(got["max_excess"].view(np.uint64), want["max_excess"].view(np.uint64))
    assert want["n_blocked"].tolist() == (cells[..., 3] < cells[..., 0]).sum(axis=1).tolist() and want["n_blocked"][4] == K
    assert want["n_blocked"][1] >= 1 and want["segment"][4] == cr.NO_SEGMENT and want["max_excess"][4] == -np.inf
    assert want["n_outside"].sum() > 0 and (got["n_outside"] <= cr.check_corridor(D, h, origin, cell, cells, pos, vel, acc, 0.0)["n_outside"]).all()
    # K beyond one wave's lanes: the lanes take several segments each, the lowest segment wins a tie
    K2 = 150
    cells2 = np.tile(np.array([[2, 2, 0, 9, 9, 0]], dtype=np.int32), (2, K2, 1))
    pos2 = np.full((2, K2, D), origin[0] + cell * 5.0)
    pos2[..., 1] = origin[1] + cell * 5.0
    pos2[0, [70, 140], 0] -= 0.3  # towards the nearer face: the same largest excess twice
    zero = np.zeros((2, K2, D))
    got = ctx.check_corridor(2, K2, D, h, g, _itensor(ctx, cells2), ctx.tensor(pos2), ctx.tensor(zero), ctx.tensor(zero), 0.0)
    want = cr.check_corridor(D, h, origin, cell, cells2, pos2, zero, zero, 0.0)
    assert want["segment"].tolist() == [70, 0]
    for f in ("segment", "n_blocked", "n_outside"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    np.testing.assert_array_equal(got["max_excess"].view(np.uint64), want["max_excess"].view(np.uint64))


@pytest.mark.parametrize("native", [True, False])
def test_end_to_end_around_a_disc(ctx, native):
    """Three vehicles, one disc: with corridors every segment stays inside its box (so outside the disc inflated by R / 2), the
    separation checks pass; without boxes the first vehicle flies through the disc, which no box contains."""
    from path_planning.solvers.scp import SCP

    E = cc.EndToEnd
    occ, origin, cell = E.grid()

    def solver():
        s = SCP(n_vehicles=E.N, time_horizon=E.T, time_step=E.h, min_distance=E.R, space_dims=E.space, native=native,
                verbose=False)
        assert s.K == E.K
        s.set_initial_states(E.p0)
        s.set_final_states(E.pf)
        s.set_obstacles(occ, origin, cell)
        return s

    s = solver()
    with pytest.raises(ValueError, match="blocked"):
        s.set_corridors()  # the straight line of vehicle 0 crosses the disc
    info = s.set_corridors(reference=E.reference(), max_grow=E.max_grow, pad=E.pad)
    assert info["n_blocked"] == 0 and info["n_open"] == 0 and info["shrink"] == 15.0 * E.h * E.h / 8.0 + E.pad
    traj = s.generate_trajectories(max_iterations=15)
    statuses = [s.last_info["qp0"]["status_val"]] + [it["status_val"] for it in s.last_info["iterations"]]
    assert set(statuses) <= {1, 2}, statuses
    pipes = {p for it in s.last_info["iterations"] for p in it["pipeline"].split("+")}
    assert not pipes & {"persistent16", "persistent8-lean"}, pipes
    rep = s.validate_solution(continuous=True)
    co = rep["corridor"]
    print(f"native={native}: corridor max_excess {co['max_excess']:.4e}, n_outside {co['n_outside']}, min distance "
          f"{rep['min_pair_distance']:.4f} / continuous {rep['min_pair_distance_continuous']:.4f}, pipelines {sorted(pipes)}")
    assert co["inside"] and co["n_outside"] == 0 and co["n_blocked"] == 0 and co["max_excess"] <= 0.0
    assert rep["collision_free"] and rep["collision_free_continuous"]
    # every sample keeps the body (radius R / 2) off the disc
    centre, radius = np.array(E.disc[:2]), E.disc[2]
    assert (np.linalg.norm(traj["positions"] - centre, axis=2) >= radius + E.R / 2).all()
    want = cr.check_corridor(E.D, E.h, origin, cell, s._corridor["cells"].cpu().numpy(), traj["positions"], traj["velocities"],
                             traj["accelerations"], 0.0)
    np.testing.assert_array_equal(co["vehicles"]["max_excess"].view(np.uint64), want["max_excess"].view(np.uint64))
    # the same problem without boxes, judged against the same cells
    s.set_position_boxes(None, None)
    free = s.generate_trajectories(max_iterations=15)
    out = s.validate_corridor()
    assert out["n_outside"] > 0 and not out["inside"] and out["vehicles"]["n_outside"][0] > 0
    assert (np.linalg.norm(free["positions"][0] - centre, axis=1) < radius).any()
    s.close()


def test_collision_rows_inside_one_corridor(ctx):
    """Two vehicles fly head-on through the SAME corridor over the disc: the joint QPs carry collision rows AND boxes, on the
    round-2 persistent kernel, in the native loop (scp_solver_solve: QP#0 and every step through the solver's helper) and in
    the Python-driven one (QP.set_position_boxes) -- the same calls, the same bits."""
    from path_planning.solvers.scp import SCP

    E = cc.EndToEnd
    occ, origin, cell = E.grid()
    p0, pf = np.array([[1.0, 5.0], [9.0, 5.6]]), np.array([[9.0, 5.0], [1.0, 5.6]])
    n = E.K + 1
    ref = np.stack([cc.polyline([p0[0], (5.0, 7.2), pf[0]], n), cc.polyline([p0[1], (5.0, 7.5), pf[1]], n)])
    out = {}
    for native in (True, False):
        s = SCP(n_vehicles=2, time_horizon=E.T, time_step=E.h, min_distance=E.R, space_dims=E.space, native=native, verbose=False)
        s.set_initial_states(p0)
        s.set_final_states(pf)
        s.set_obstacles(occ, origin, cell)
        info = s.set_corridors(reference=ref, max_grow=E.max_grow, pad=E.pad)
        assert info["n_blocked"] == 0 and info["n_open"] == 0
        traj = s.generate_trajectories(max_iterations=15)
        its = s.last_info["iterations"]
        statuses = [s.last_info["qp0"]["status_val"]] + [it["status_val"] for it in its]
        pipes = {p for it in its for p in it["pipeline"].split("+")}
        rep = s.validate_solution()
        print(f"native={native}: {len(its)} SCP iterations, statuses {statuses}, pipelines {sorted(pipes)}, corridor max_excess "
              f"{rep['corridor']['max_excess']:.4e}, min distance {rep['min_pair_distance']:.4f}")
        assert len(its) >= 1 and set(statuses) <= {1, 2}, statuses
        assert "persistent" in pipes and not pipes & {"persistent16", "persistent8-lean"}, pipes
        assert rep["corridor"]["inside"] and rep["collision_free"]
        out[native] = traj["accelerations"].copy()
        s.close()
    np.testing.assert_array_equal(out[True], out[False])


def test_python_api_errors(ctx):
    from path_planning.solvers.scp import SCP

    E = cc.EndToEnd
    s = SCP(n_vehicles=E.N, time_horizon=E.T, time_step=E.h, min_distance=E.R, space_dims=E.space, verbose=False)
    s.set_initial_states(E.p0)
    s.set_final_states(E.pf)
    with pytest.raises(ValueError, match="set_obstacles"):
        s.set_corridors()
    with pytest.raises(ValueError, match="set_corridors"):
        s.validate_corridor()
    occ, origin, cell = E.grid()
    with pytest.raises(ValueError):
        s.set_obstacles(occ[0, :, :, None, None], origin, cell)
    with pytest.raises(ValueError):
        s.set_obstacles(occ, origin, 0.0)
    s.set_obstacles(occ[0], origin, cell)  # [ny][nx] in 2-D
    with pytest.raises(ValueError, match="max_grow"):
        s.set_corridors(reference=E.reference(), max_grow=2000)
    with pytest.raises(ValueError, match="shape"):
        s.set_corridors(reference=E.reference()[:, :-1])
    info = s.set_corridors(allow_open=True)  # the straight lines: vehicle 0 and 1 are blocked at the disc
    assert info["n_blocked"] > 0 and info["n_open"] >= info["n_blocked"]
    lo = np.full((E.N, E.K, E.D), -np.inf)
    hi = np.full((E.N, E.K, E.D), np.inf)
    hi[1, 7, 0] = -1.0
    with pytest.raises(ValueError, match="vehicle 1, state 7"):
        s.set_position_boxes(lo, hi)
    with pytest.raises(ValueError):
        s.set_position_boxes(lo, None)
    s.close()
