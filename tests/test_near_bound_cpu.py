"""The criterion of the near violations pass (scp_near.hip), modelled in numpy on oracle data: a grid-swap problem of 64
agents, linearised at QP#0's solution and evaluated at the joint QP's solution.

    viol_r = (R - dist_r) - eta_r . (dP_i[k] - dP_j[k]) <= R - dist_r + |dP_i[k]| + |dP_j[k]|

A pair is examined when dist < R + m_i + m_j + tau (m = |dP|, rounded up); the kernel finds those pairs in the 3^D
neighbouring cells of a grid whose cells are at least rho_k = R + 2 max_i m_i[k] + tau wide."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

TAU = 1e-6        # SCP_NEAR_TAU (scp_common.h)
FEAS_TOL = 1e-6   # scp_solve_options.feasibility_tol's default
CAP = {2: 45, 3: 12}  # NearCap: cells per axis


@pytest.fixture(scope="module")
def data():
    from path_planning.scenarios.position_generator import generate_grid_swap

    p0, pf, space = generate_grid_swap(64, seed=64000)
    prob = so.make_problem(64, 10.0, 0.2, 0.8, space, p0, pf)
    x0, info0 = co.admm(prob, st=qo.Settings(max_iter=4000))
    assert info0["status_val"] in (1, 2)
    prev, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, prev)
    x1, info1 = co.admm(prob, eta, l_col, dist, x0=x0, st=qo.Settings(max_iter=10000))
    assert info1["status_val"] in (1, 2)
    new, _ = so.kinematics(prob, x1)
    return prob, prev, new, eta, dist


def model(prob, prev, new, eta, dist):
    """-> per row: viol (the exhaustive pass), examined, and per examined row whether the grid finds it"""
    N, K, D, R = prob.N, prob.K, prob.D, prob.R
    iu, ju = so.pair_index(N)
    pairs = iu.size
    dP = new - prev
    viol = np.empty(K * pairs)
    examined = np.zeros(K * pairs, dtype=bool)
    in_reach = np.ones(K * pairs, dtype=bool)
    neighbours = np.ones(K * pairs, dtype=bool)
    for k in range(K):
        sl = slice(k * pairs, (k + 1) * pairs)
        viol[sl] = (R - dist[sl]) - np.sum(eta[sl] * (dP[iu, k] - dP[ju, k]), axis=1)
        m = np.sqrt(np.sum(dP[:, k] ** 2, axis=1)) * (1.0 + 1e-10)
        diff = prev[iu, k] - prev[ju, k]
        ss = np.sum(diff * diff, axis=1)
        reach = R + m[iu] + m[ju] + TAU
        ex = ss < reach * reach * (1.0 + 1e-12)
        examined[sl] = ex
        # the grid of the step, as the kernel builds it
        side_min = (R + 2.0 * m.max() + TAU) * (1.0 + 1e-6)
        lo = prev[:, k].min(0)
        ext = prev[:, k].max(0) - lo
        n = np.minimum(np.floor(ext / side_min) + 1.0, CAP[D])
        side = np.maximum(side_min, ext / n * (1.0 + 1e-6))
        cell = np.minimum(np.maximum((prev[:, k] - lo) * (1.0 / side), 0.0), n - 1).astype(np.int64)
        in_reach[sl] = ~ex | (np.sqrt(ss) < R + 2.0 * m.max() + TAU)
        neighbours[sl] = ~ex | (np.abs(cell[iu] - cell[ju]).max(axis=1) <= 1)
    return viol, examined, in_reach, neighbours


def test_unexamined_rows_cannot_matter(data):
    prob, prev, new, eta, dist = data
    viol, examined, in_reach, neighbours = model(prob, prev, new, eta, dist)
    violated = viol > FEAS_TOL
    print(f"rows {viol.size}, examined {examined.sum()}, violated {violated.sum()}, max viol {viol.max():.3e}, "
          f"max unexamined {viol[~examined].max():.3e}")
    assert violated.any() and (~examined).any()          # the data exercises both sides
    assert not (viol[~examined] > -TAU).any()            # no unexamined row is closer to active than tau
    assert examined[violated].all()                      # every violated row is examined
    assert in_reach.all() and neighbours.all()           # every examined pair lies within rho_k, in neighbouring cells
    np.testing.assert_array_equal(np.nonzero(examined & violated)[0], np.nonzero(violated)[0])  # the same row set
    assert viol[examined].max() == viol.max() and viol.max() >= -0.5 * TAU  # the same maximum, and it is trusted
    assert examined.sum() < viol.size // 10              # (and the criterion does skip most rows)


def test_far_apart_pairs_take_the_fallback(data):
    """nothing moved and nobody is near anybody: no examined row reaches -tau / 2, the caller must run the exhaustive pass"""
    prob = data[0]
    N, K = prob.N, prob.K
    g = 5.0 * np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(N, 1, 2)
    prev = np.repeat(g, K, axis=1)
    eta, _, dist = so.linearize_pairs(prob, prev)
    viol, examined, _, _ = model(prob, prev, prev.copy(), eta, dist)
    assert not examined.any() and viol.max() < -0.5 * TAU
