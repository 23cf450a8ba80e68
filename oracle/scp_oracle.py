"""CPU oracle for the SCP hot path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
The shipped planner (ba-path-planning_amd/path_planning) never imports anything from oracle/.

This file restates, in plain numpy, the *assembly* half of the reference solver
(/root/reference/src/path_planning/solvers/scp.py): problem definition, fixed constraint rows and
bounds, kinematics, pairwise collision linearisation and the avoidance check.  Every function cites
the reference lines it follows.  The restatement is pinned against the imported reference by
tests/golden/make_golden.py (fixtures under tests/golden/*.npz) and tests/test_oracle_golden.py.

The QP half (OSQP, a third-party dependency that is absent from /root/reference and from this image)
lives in oracle/qp_oracle.py and is "parity unpinned" -- see its header.

Generalisation beyond the reference: D (space dimension) is a parameter.  D=2 reproduces the
reference exactly; D=3 is an extension checked by the z==0 metamorphic test.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.sparse as sp


@dataclasses.dataclass
class Problem:
    """Problem definition, mirrors SCP.__init__ / set_initial_states / set_final_states
    (scp.py:32-129).  Arrays are (N, D) float64."""

    N: int
    K: int
    h: float
    R: float
    p0: np.ndarray
    v0: np.ndarray
    pf: np.ndarray
    vf: np.ndarray
    pos_min: np.ndarray
    pos_max: np.ndarray
    vel_min: float = -2.0  # scp.py:67-68
    vel_max: float = 2.0
    acc_min: float = -15.0  # scp.py:70-71
    acc_max: float = 15.0
    jerk_min: float = -20.0  # scp.py:73-74
    jerk_max: float = 20.0
    convergence_tolerance: float = 1.5e-2  # scp.py:52

    @property
    def D(self) -> int:
        return int(self.p0.shape[1])

    @property
    def n(self) -> int:
        return self.N * self.K * self.D

    @property
    def pairs(self) -> int:
        return self.N * (self.N - 1) // 2

    @property
    def m_fixed(self) -> int:
        return self.N * self.D * (4 * self.K - 1)

    @property
    def m_col(self) -> int:
        return self.pairs * self.K


def make_problem(n_vehicles, time_horizon, time_step, min_distance, space_dims, p0, pf, v0=None, vf=None):
    """SCP(...) + set_initial_states + set_final_states (scp.py:32-129).  K = int(T/h) (scp.py:43).
    space_dims = [min_0..min_{D-1}, max_0..max_{D-1}] (scp.py:63-64 for D=2)."""
    p0 = np.asarray(p0, dtype=float)
    pf = np.asarray(pf, dtype=float)
    N, D = p0.shape
    assert N == n_vehicles
    if v0 is None:
        v0 = np.zeros((N, D))
    if vf is None:
        vf = np.zeros((N, D))
    sd = np.asarray(space_dims, dtype=float)
    assert sd.shape == (2 * D,)
    return Problem(
        N=N,
        K=int(time_horizon / time_step),
        h=float(time_step),
        R=float(min_distance),
        p0=p0,
        v0=np.asarray(v0, dtype=float),
        pf=pf,
        vf=np.asarray(vf, dtype=float),
        pos_min=sd[:D].copy(),
        pos_max=sd[D:].copy(),
    )


# --------------------------------------------------------------------------------------------
# a2: fixed constraint rows (scp.py:10-28, :182-257)
# --------------------------------------------------------------------------------------------
def time_blocks(K, h):
    """The four K-column blocks that every (agent, axis) shares (scp.py:10-28, :198-203, :227-232).

    J  (K-1, K): first difference / h                          -> jerk rows
    Id (K, K)                                                  -> acceleration rows
    V  (K, K):  V[k, m] = h            for m <= k              -> velocity rows (state k+1)
    S  (K, K):  S[k, m] = h^2 (k-m+.5) for m <= k              -> position rows (state k+1)
    S0 (K, K):  S0[k, m] = h^2 (k-m-.5) for m <  k             -> stored sample k (collision rows,
                                                                  scp.py:489-491, :586-593)
    """
    J = np.zeros((K - 1, K))
    for k in range(K - 1):
        J[k, k] = -1.0 / h
        J[k, k + 1] = 1.0 / h
    kk = np.arange(K)[:, None]
    mm = np.arange(K)[None, :]
    V = np.where(mm <= kk, h, 0.0)
    S = np.where(mm <= kk, h * h * (kk - mm + 0.5), 0.0)
    S0 = np.where(mm < kk, (h * h) * (kk - mm - 0.5), 0.0)
    return J, np.eye(K), V, S, S0


def fixed_matrices_explicit(prob: Problem):
    """Explicit CSC C_jerk, C_acc, C_vel, C_pos exactly as the reference builds them
    (scp.py:188, :193, :198-203, :227-232).  Variable index (i*K + k)*D + d."""
    N, K, D, h = prob.N, prob.K, prob.D, prob.h
    J, Id, V, S, _ = time_blocks(K, h)
    ID = sp.eye(D, format="csc")
    IN = sp.eye(N, format="csc")

    def lift(B):
        return sp.kron(IN, sp.kron(sp.csc_matrix(B), ID, format="csc"), format="csc")

    return lift(J), lift(Id), lift(V), lift(S)


def fixed_bounds(prob: Problem, pos_boxes=None):
    """Bounds of the fixed rows in the reference's stacking order jerk, acc, vel, pos
    (scp.py:189-190, :194-195, :206-224, :234-257, stacked at :342-358).

    Returns dict of (l, u) arrays; vel/pos/acc have shape (N, K, D), jerk (N, K-1, D); flattening
    each in C order gives the reference's row order.

    pos_boxes = (lo, hi), both (N, K, D) by state (not part of the reference: the per-state position boxes of
    scp_qp_set_position_boxes, include/scp_hip.h): position row k = 0 .. K-2 (state k + 1) becomes
    [max(lo, pos_min) - off, min(hi, pos_max) - off], each side selected first and the offset subtracted after; state 0
    and the final-position row are untouched.  None: every array is what it was without the argument."""
    N, K, D, h = prob.N, prob.K, prob.D, prob.h
    l_jerk = np.full((N, K - 1, D), float(prob.jerk_min))
    u_jerk = np.full((N, K - 1, D), float(prob.jerk_max))
    l_acc = np.full((N, K, D), float(prob.acc_min))
    u_acc = np.full((N, K, D), float(prob.acc_max))

    l_vel = np.empty((N, K, D))
    u_vel = np.empty((N, K, D))
    l_vel[:, : K - 1, :] = (prob.vel_min - prob.v0)[:, None, :]  # scp.py:218-221
    u_vel[:, : K - 1, :] = (prob.vel_max - prob.v0)[:, None, :]
    l_vel[:, K - 1, :] = prob.vf - prob.v0  # scp.py:223-224
    u_vel[:, K - 1, :] = prob.vf - prob.v0

    l_pos = np.empty((N, K, D))
    u_pos = np.empty((N, K, D))
    kp1 = np.arange(1, K + 1, dtype=float)
    # off = p0 + h*(k+1)*v0, evaluated as the reference does: (h * (k_idx + 1)) * v0  (scp.py:246-247)
    off = prob.p0[:, None, :] + (h * kp1)[None, :, None] * prob.v0[:, None, :]
    l_pos[:, : K - 1, :] = prob.pos_min[None, None, :] - off[:, : K - 1, :]  # scp.py:251-254
    u_pos[:, : K - 1, :] = prob.pos_max[None, None, :] - off[:, : K - 1, :]
    if pos_boxes is not None:
        lo, hi = (np.asarray(a, dtype=float) for a in pos_boxes)
        assert lo.shape == (N, K, D) and hi.shape == (N, K, D), (lo.shape, hi.shape)
        bl, bu = lo[:, 1:, :], hi[:, 1:, :]
        l_pos[:, : K - 1, :] = np.where(bl > prob.pos_min, bl, prob.pos_min) - off[:, : K - 1, :]
        u_pos[:, : K - 1, :] = np.where(bu < prob.pos_max, bu, prob.pos_max) - off[:, : K - 1, :]
    l_pos[:, K - 1, :] = prob.pf - off[:, K - 1, :]  # scp.py:256-257
    u_pos[:, K - 1, :] = prob.pf - off[:, K - 1, :]
    return {
        "jerk": (l_jerk, u_jerk),
        "acc": (l_acc, u_acc),
        "vel": (l_vel, u_vel),
        "pos": (l_pos, u_pos),
    }


def stack_fixed(prob: Problem):
    """(C, l, u) of QP#0 exactly as scp.py:332-358 stacks them."""
    Cj, Ca, Cv, Cp = fixed_matrices_explicit(prob)
    b = fixed_bounds(prob)
    C = sp.vstack([Cj, Ca, Cv, Cp], format="csc")
    l = np.hstack([b[k][0].ravel() for k in ("jerk", "acc", "vel", "pos")])
    u = np.hstack([b[k][1].ravel() for k in ("jerk", "acc", "vel", "pos")])
    return C, l, u


# --------------------------------------------------------------------------------------------
# a4 / a7: kinematics (scp.py:371-397, :559-595)
# --------------------------------------------------------------------------------------------
def kinematics(prob: Problem, accelerations):
    """positions, velocities (N, K, D) from accelerations (N, K, D) or flat.

    Same summation order as the reference (j ascending, starting from p0 + h*k*v0) so that the
    result is bitwise equal to scp.py:382-395 / :575-593 (checked by the golden test)."""
    N, K, D, h = prob.N, prob.K, prob.D, prob.h
    a = np.asarray(accelerations, dtype=float).reshape(N, K, D)
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    pos[:, 0, :] = prob.p0
    vel[:, 0, :] = prob.v0
    hh = h * h  # h**2 == h*h bitwise
    for k in range(1, K):
        v = prob.v0.copy()
        p = prob.p0 + (h * k) * prob.v0  # scp.py:393 self.h * k * init_vel  /  :587 k * h * v
        for j in range(k):
            v = v + h * a[:, j, :]
            p = p + (hh * (k - j - 0.5)) * a[:, j, :]
        vel[:, k, :] = v
        pos[:, k, :] = p
    return pos, vel


def free_positions(prob: Problem):
    """c_i[k] = p0_i + k*h*v0_i  (the acceleration-free part of p_i[k]), (N, K, D)."""
    k = np.arange(prob.K, dtype=float)
    return prob.p0[:, None, :] + (k * prob.h)[None, :, None] * prob.v0[:, None, :]


# --------------------------------------------------------------------------------------------
# a5: pairwise collision linearisation (scp.py:453-557)
# --------------------------------------------------------------------------------------------
def pair_index(N):
    """(i, j) arrays in the reference's lexicographic i<j order (scp.py:495-496)."""
    iu, ju = np.triu_indices(N, k=1)
    return iu.astype(np.int64), ju.astype(np.int64)


def linearize_pairs(prob: Problem, prev_positions, degenerate_direction=None):
    """Compact form of _add_collision_constraints (scp.py:453-557).

    Row r = k*pairs + idx(i, j), k-major then lexicographic i<j (scp.py:487-496).
    Returns eta (rows, D), l (rows,), dist (rows,) where row r of A_collision is
        +eta_r[d] * h^2 (k-m-.5) on a_i[m], -eta_r[d] * h^2 (k-m-.5) on a_j[m], m < k
    (scp.py:512-534), l_r = R + (eta.diff - dist) - (eta.(p0_i-p0_j) + eta.(v0_i-v0_j)*(k*h))
    (scp.py:543-550) and u_r = +inf (scp.py:479).

    Degenerate pairs (dist < 1e-6): the reference draws a random direction and sets dist = 1
    (scp.py:503-507).  That is not reproducible; the oracle (and the HIP path) use the fixed unit
    direction e_0 (or `degenerate_direction`) with the same dist = 1 rule.
    """
    N, K, D = prob.N, prob.K, prob.D
    P = np.asarray(prev_positions, dtype=float).reshape(N, K, D)
    iu, ju = pair_index(N)
    pairs = iu.size
    eta = np.empty((K * pairs, D))
    l = np.empty(K * pairs)
    dist_all = np.empty(K * pairs)
    dp0 = prob.p0[iu] - prob.p0[ju]
    dv0 = prob.v0[iu] - prob.v0[ju]
    e0 = np.zeros(D)
    e0[0] = 1.0
    if degenerate_direction is not None:
        e0 = np.asarray(degenerate_direction, dtype=float)
    for k in range(K):
        diff = P[iu, k, :] - P[ju, k, :]
        if D == 2:
            dist = np.hypot(diff[:, 0], diff[:, 1])  # scp.py:501
        else:
            dist = np.sqrt(np.sum(diff * diff, axis=1))
        deg = dist < 1e-6  # scp.py:503
        dist = np.where(deg, 1.0, dist)
        e = diff / dist[:, None]  # scp.py:509
        e[deg] = e0
        # eta @ x for D=2 is x0*y0 + x1*y1 evaluated left to right
        init_pos = np.sum(e * dp0, axis=1)  # scp.py:543
        init_vel = np.sum(e * dv0, axis=1) * (k * prob.h)  # scp.py:544
        lin = np.sum(e * diff, axis=1) - dist  # scp.py:547
        rhs = prob.R + lin - (init_pos + init_vel)  # scp.py:549
        sl = slice(k * pairs, (k + 1) * pairs)
        eta[sl] = e
        l[sl] = rhs
        dist_all[sl] = dist
    return eta, l, dist_all


def collision_matrix_explicit(prob: Problem, eta):
    """Explicit CSC A_collision from the compact eta (scp.py:512-534, :555).  Small sizes only."""
    N, K, D, h = prob.N, prob.K, prob.D, prob.h
    iu, ju = pair_index(N)
    pairs = iu.size
    rows, cols, vals = [], [], []
    for k in range(1, K):
        m = np.arange(k)
        w = (h * h) * (k - m - 0.5)  # scp.py:491
        for q in range(pairs):
            r = k * pairs + q
            for d in range(D):
                rows.append(np.full(k, r))
                cols.append((iu[q] * K + m) * D + d)
                vals.append(eta[r, d] * w)
                rows.append(np.full(k, r))
                cols.append((ju[q] * K + m) * D + d)
                vals.append(-eta[r, d] * w)
    if rows:
        rows = np.concatenate(rows)
        cols = np.concatenate(cols)
        vals = np.concatenate(vals)
    else:
        rows = cols = np.zeros(0, dtype=int)
        vals = np.zeros(0)
    return sp.coo_matrix((vals, (rows, cols)), shape=(K * pairs, N * K * D)).tocsc()


def collision_apply(prob: Problem, eta, x, rows=None):
    """(A_col x)[rows] through the structured form  eta_r . ((S0 x_i)[k] - (S0 x_j)[k])."""
    N, K, D = prob.N, prob.K, prob.D
    _, _, _, _, S0 = time_blocks(K, prob.h)
    Q = np.einsum("km,imd->ikd", S0, np.asarray(x).reshape(N, K, D))
    iu, ju = pair_index(N)
    pairs = iu.size
    if rows is None:
        rows = np.arange(K * pairs)
    k = rows // pairs
    q = rows % pairs
    return np.sum(eta[rows] * (Q[iu[q], k, :] - Q[ju[q], k, :]), axis=1)


def collision_apply_T(prob: Problem, eta, g, rows=None):
    """A_col[rows]^T g through the structured form  S0^T scatter(+-eta_r g_r)."""
    N, K, D = prob.N, prob.K, prob.D
    _, _, _, _, S0 = time_blocks(K, prob.h)
    iu, ju = pair_index(N)
    pairs = iu.size
    if rows is None:
        rows = np.arange(K * pairs)
    k = rows // pairs
    q = rows % pairs
    G = np.zeros((N, K, D))
    contrib = eta[rows] * np.asarray(g)[:, None]
    np.add.at(G, (iu[q], k), contrib)
    np.add.at(G, (ju[q], k), -contrib)
    return np.einsum("km,ikd->imd", S0, G).ravel()


# --------------------------------------------------------------------------------------------
# a8: avoidance check (scp.py:597-615)
# --------------------------------------------------------------------------------------------
def check_avoidance(prob: Problem, positions):
    """Returns (is_feasible, first_violation) where first_violation = (k, i, j, dist) of the first
    pair in k -> i -> j order with ||p_i - p_j|| < R - 0.01 (scp.py:602-615), or None."""
    N, K, D = prob.N, prob.K, prob.D
    P = np.asarray(positions, dtype=float).reshape(N, K, D)
    iu, ju = pair_index(N)
    thr = prob.R - 0.01
    for k in range(K):
        diff = P[iu, k, :] - P[ju, k, :]
        dist = np.sqrt(np.sum(diff * diff, axis=1))  # np.linalg.norm (scp.py:609)
        bad = np.nonzero(dist < thr)[0]
        if bad.size:
            q = int(bad[0])
            return False, (k, int(iu[q]), int(ju[q]), float(dist[q]))
    return True, None


def min_pair_distance(prob: Problem, positions):
    N, K, D = prob.N, prob.K, prob.D
    P = np.asarray(positions, dtype=float).reshape(N, K, D)
    iu, ju = pair_index(N)
    best = np.inf
    for k in range(K):
        diff = P[iu, k, :] - P[ju, k, :]
        best = min(best, float(np.sqrt(np.sum(diff * diff, axis=1)).min()))
    return best
