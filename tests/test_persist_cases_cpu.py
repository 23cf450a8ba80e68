"""CPU checks behind tests/test_persist_iterates_gpu.py: the oracle's state snapshots are the state a solve stopped at that
step ends in, every case of tests/persist_cases.py reaches the edge it claims, and the GPU tolerance can see a 1e-6 error
in one collision row at the last agent."""
import numpy as np
import pytest

import persist_cases as pc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

ARRAYS = ("x", "zf", "yf", "zc", "yc")


@pytest.mark.parametrize("adaptive", [False, True])
def test_snapshot_is_the_state_of_a_solve_stopped_there(adaptive):
    """snap_out[m] == the state of admm_structured(max_iter = m), bit for bit, at step counts on and off the check cadence
    (check_termination = 6: m = 1, 7, 13 are not multiples), and across an adaptive-rho update (m = 50 with adaptive rho)."""
    sc = pc.RHO_2D  # 2-D, N = 17, K = 50
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    steps = (1, 6, 7, 13, 50, 53) if adaptive else (1, 6, 7, 13)
    kw = dict(adaptive_rho=True, adaptive_rho_interval=50, check_termination=25) if adaptive else {}
    snaps = {}
    _, y_all, info_all = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=pc.step_settings(max(steps), **kw), rows0=W,
                                            snapshots=set(steps), snap_out=snaps)
    assert sorted(snaps) == sorted(steps)
    if adaptive:
        assert snaps[50]["rho"] != pc.step_settings(1).rho  # the update at step 50 is in the snapshot
    for m in steps:
        x, y, info = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=pc.step_settings(m, **kw), rows0=W)
        assert info["iter"] == m and info["status_val"] == -2
        s = snaps[m]
        np.testing.assert_array_equal(s["x"], x)
        for i, blk in enumerate(("jerk", "acc", "vel", "pos")):
            np.testing.assert_array_equal(s["yf"][i], y[blk])
        np.testing.assert_array_equal(s["yc"], y["col"])
        np.testing.assert_array_equal(s["rows"], y["col_rows"])
        assert s["rho"] == info["rho"] and s["round"] == 1
    # the final snapshot is the run's own final state; results do not depend on asking for snapshots
    x_plain, y_plain, info_plain = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=pc.step_settings(max(steps), **kw),
                                                      rows0=W)
    np.testing.assert_array_equal(snaps[max(steps)]["x"], x_plain)
    info_all.pop("checks", None), info_plain.pop("checks", None)
    assert info_all == info_plain


def test_snapshot_round_of_constraint_generation():
    """Snapshots count steps over all rounds and record the round: a margin of 0.05 leaves rows out of round 1 that the
    solution violates, so round 2 starts at the step after round 1 ended, with the new rows in the working set."""
    sc = pc.RHO_2D  # 2-D, N = 17, K = 50
    prob, x0, eta, l_col, dist, _ = pc.setup(sc)
    st = qo.Settings(cg_iters=1, max_iter=10000, margin=0.05)
    _, _, info = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st)
    assert info["rounds"] >= 2 and info["added"][0] > 0
    snaps = {}
    steps = set(range(1, info["iter"] + 1))
    qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, snapshots=steps, snap_out=snaps)
    n1 = max(m for m in snaps if snaps[m]["round"] == 1)
    assert snaps[n1 + 1]["round"] == 2 and snaps[n1 + 1]["rows"].size == snaps[n1]["rows"].size + info["added"][0]


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_case_reaches_its_edge(case):
    sc = case.scen
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    per = pc.apb(case.kernel, sc.dim)
    assert sc.N % per == case.n_tail and sc.K % 16 == case.k_tail
    assert prob.K == sc.K and abs(sc.T - sc.K * pc.H) < 1e-8
    assert W.size > 0  # (the persistent kernels run joint QPs only)
    k, wi, wj = qo.working_rows(prob, W)
    if sc.N > per:  # at least one working row joins two agents in different workgroups
        assert np.any(wi // per != wj // per)
    last = (wi == sc.N - 1) | (wj == sc.N - 1)  # ... and one touches the last agent of the last workgroup
    assert last.any()
    # the working set fits the kernel's LDS entry tables (else the solve runs on the three-launch pipeline)
    assert pc.block_entries(prob, W, per).max() < pc.entry_cap(case.kernel, sc.N, sc.K, sc.dim)
    # every compared step is reached: no termination, no certificate
    snaps, info = pc.cached_snapshots(sc)
    assert info["status_val"] == -2 and info["iter"] == max(case.steps) and sorted(snaps) == sorted(case.steps)


def sensitivity_row(sc):
    """a working row at the last agent that is active (A x < l) at every compared step of the oracle run"""
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    snaps, _ = pc.cached_snapshots(sc)
    _, wi, wj = qo.working_rows(prob, W)
    ok = (wi == sc.N - 1) | (wj == sc.N - 1)
    slack = np.full(W.size, np.inf)
    for m in pc.STEPS:
        s = so.collision_apply(prob, eta, snaps[m]["x"].ravel())[W] - l_col[W]
        ok &= s < 0
        slack = np.minimum(slack, -s)
    assert ok.any(), "no working row at the last agent is active at every compared step"
    return int(W[np.argmax(np.where(ok, slack, -np.inf))])


@pytest.mark.parametrize("sc", pc.SCENARIOS, ids=lambda s: s.label)
def test_sensitivity_control(sc):
    """l_col of one active row at the last agent moved by 1e-6: at every compared step some compared array of the oracle
    state moves by at least 100 x the tolerance the GPU comparison allows that array.  (At m = 1 only z, y can move: the
    first x-update reads l only through the initial z = max(A x0, l).)"""
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    base, _ = pc.cached_snapshots(sc)
    r = sensitivity_row(sc)
    l2 = l_col.copy()
    l2[r] += 1e-6
    moved, _ = pc.oracle_snapshots(sc, l_col=l2)
    for m in pc.STEPS:
        ra, rb = pc.reference_arrays(prob, base[m]), pc.reference_arrays(prob, moved[m])
        tol = pc.tolerances(prob, ra, base[m]["rho"])  # what the GPU comparison allows, entry by entry
        best = max(float(np.max(np.abs(ra[k] - rb[k]) / tol[k], initial=0.0)) for k in ARRAYS)
        assert best >= 100.0, (m, r, best)


def test_settings_match_gpu_side():
    st = pc.step_settings(12)
    g = pc.gpu_step_settings(3, 12)
    for k in ("cg_iters", "max_iter", "check_termination", "eps_abs", "eps_rel"):
        assert getattr(st, k) == g[k]
    assert bool(st.adaptive_rho) == bool(g["adaptive_rho"])
