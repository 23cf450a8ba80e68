"""Per-state position boxes in the numpy oracle (so.fixed_bounds / qo.admm_structured / qo.scp_solve, pos_boxes=): without
boxes nothing changes, with boxes the position block is the bound overwrite of scp_qp_set_position_boxes bit for bit
(tests/corridor_ref.py::position_rows), and the boxed solve lands on the minimiser the explicit-matrix oracle finds."""
import numpy as np
import pytest
import scipy.sparse as sp

import corridor_ref as cr
import persist_cases as pc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so
from test_corridor_gpu import bound_overwrite_case, boxed_qp_case

BLOCKS = ("jerk", "acc", "vel", "pos")


def _inf_boxes(prob):
    shape = (prob.N, prob.K, prob.D)
    return np.full(shape, -np.inf), np.full(shape, np.inf)


@pytest.mark.parametrize("D", [2, 3])
def test_no_boxes_changes_no_bound(D):
    """pos_boxes=None is the unchanged code path; all-infinite boxes give the same bits (as scp_qp_set_position_boxes does)"""
    prob = bound_overwrite_case(D)[0]
    base = so.fixed_bounds(prob)
    for b in (so.fixed_bounds(prob, None), so.fixed_bounds(prob, pos_boxes=None), so.fixed_bounds(prob, _inf_boxes(prob))):
        assert sorted(b) == sorted(base)
        for k in BLOCKS:
            for s in (0, 1):
                assert b[k][s].dtype == base[k][s].dtype and b[k][s].shape == base[k][s].shape
                np.testing.assert_array_equal(b[k][s].view(np.uint64), base[k][s].view(np.uint64))
    # the explicit stack is built from the same call
    _, l, u = so.stack_fixed(prob)
    np.testing.assert_array_equal(l, np.hstack([base[k][0].ravel() for k in BLOCKS]))
    np.testing.assert_array_equal(u, np.hstack([base[k][1].ravel() for k in BLOCKS]))


def test_no_boxes_changes_no_solve():
    sc = pc.TABLE_2D[3][0]  # circle, N = 9, K = 50
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    st = pc.step_settings(30, adaptive_rho=True, check_termination=25)
    runs = [qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W, **kw)
            for kw in ({}, {"pos_boxes": None}, {"pos_boxes": _inf_boxes(prob)})]
    x, y, info = runs[0]
    assert info["iter"] == 30
    for x2, y2, info2 in runs[1:]:
        np.testing.assert_array_equal(x2, x)
        for k in y:
            np.testing.assert_array_equal(y2[k], y[k])
        assert info2 == info


@pytest.mark.parametrize("D", [2, 3])
def test_boxed_position_block_bit_for_bit(D):
    prob, space, lo, hi = bound_overwrite_case(D)
    N, K = prob.N, prob.K
    assert np.isinf(lo).any() and np.isinf(hi).any() and (lo[:, 1:] < 0.0).any() and (hi[:, 1:] > 20.0).any()
    base = so.fixed_bounds(prob)
    b = so.fixed_bounds(prob, (lo, hi))
    wl, wu = cr.position_rows(K, prob.h, space, prob.p0, prob.v0, lo, hi)
    for s, want in ((0, wl), (1, wu)):
        got = pc.time_major(b["pos"][s])
        np.testing.assert_array_equal(got[:K - 1].view(np.uint64), want.view(np.uint64))
        np.testing.assert_array_equal(b["pos"][s][:, K - 1].view(np.uint64), base["pos"][s][:, K - 1].view(np.uint64))  # final
        assert not np.array_equal(b["pos"][s], base["pos"][s])
        for k in BLOCKS[:3]:
            np.testing.assert_array_equal(b[k][s].view(np.uint64), base[k][s].view(np.uint64))
    # state 0 is never read
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[:, 0], hi2[:, 0] = 7.0, 3.0
    for s in (0, 1):
        np.testing.assert_array_equal(so.fixed_bounds(prob, (lo2, hi2))["pos"][s], b["pos"][s])


def test_boxed_solve_matches_the_explicit_oracle():
    prob, lo, hi, C, l, u = boxed_qp_case()
    b = so.fixed_bounds(prob, (lo, hi))
    np.testing.assert_array_equal(np.hstack([b[k][0].ravel() for k in BLOCKS]), l)
    np.testing.assert_array_equal(np.hstack([b[k][1].ravel() for k in BLOCKS]), u)
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), C, l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    assert r["status_val"] == 1
    st = qo.Settings(eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    x, _, info = qo.admm_structured(prob, st=st, pos_boxes=(lo, hi))
    assert info["status_val"] == 1
    np.testing.assert_allclose(x.ravel(), r["x"], rtol=0, atol=1e-7)
    free, _, _ = qo.admm_structured(prob, st=st)
    assert np.abs(free.ravel() - r["x"]).max() > 1e-3  # (the boxes matter: the box-free minimiser is another point)


def test_scp_solve_passes_the_boxes_on():
    """boxes wide open: the loop of the unchanged path, bit for bit; a waypoint box: every QP sees it"""
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(4, 0.8, seed=1)
    prob = so.make_problem(4, 10.0, 0.5, 0.8, [0, 0, 20, 20], p0, pf)
    base = qo.scp_solve(prob, 15, qo.Settings(max_iter=10000))
    same = qo.scp_solve(prob, 15, qo.Settings(max_iter=10000), pos_boxes=_inf_boxes(prob))
    np.testing.assert_array_equal(same["accelerations"], base["accelerations"])
    lo, hi = _inf_boxes(prob)
    j = prob.K // 2
    lo[0, j, 0] = base["positions"][0, j, 0] + 1.0
    out = qo.scp_solve(prob, 15, qo.Settings(max_iter=10000), pos_boxes=(lo, hi))
    assert all(i["status_val"] == 1 for i in out["infos"])
    assert out["positions"][0, j, 0] >= lo[0, j, 0] - 3e-2 and np.abs(out["positions"] - base["positions"]).max() > 0.5
