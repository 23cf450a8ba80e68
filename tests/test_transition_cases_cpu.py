"""CPU checks behind tests/test_transitions_gpu.py: every case of tests/transition_cases.py reaches the transition it claims,
the tables cover the pipelines they are there for, the tolerance floor 100 d stays below 1e-8, and the comparison can fail: at
every compared step the oracle snapshot differs by more than 100 tolerances in some compared array from what the wrong
transition would give:

  continuation   the state after m2 steps alone (a second solve that had reset)
  round two      the added rows in the working set from step 0, and the rows never joining, at the same total step count
  rho            the run with adaptive_rho = False at the same m
"""
import numpy as np
import pytest

import persist_cases as pc
import pipeline_cases as qc
import transition_cases as tc
from oracle import c_oracle as co
from oracle import qp_oracle as qo

FLOOR_MAX = 1e-8  # a group whose floor 100 d alone exceeds this gets another scenario


def _ids(cases):
    return [c.id for c in cases]


def one_per_oracle_run(cases):
    return list({(c.scen, c.cg_iters, c.start): c for c in cases}.values())


# ---- 1. continuation ------------------------------------------------------------------------------------------------------
def test_continuation_table_covers_the_code_paths():
    def shapes(group, **kw):
        return {(c.scen.N, c.scen.dim, c.scen.K) for c in tc.CONT if c.group == group and all(getattr(c, k) == v for k, v in kw.items())}

    for p in (0, 1):
        assert {(9, 2, 65), (9, 2, 120)} <= shapes("A", persistent=p)
    assert (6, 3, 65) in shapes("A") and {(9, 2, 121), (6, 3, 129)} <= shapes("B")
    assert {(c.cg_iters, c.use_mfma) for c in tc.CONT if c.group == "C"} == {(2, 1), (3, 0), (1, 2)}
    for start in ("zero", "random"):
        assert {K for _, _, K in shapes("D", start=start)} == {64, 65, 121}
    for dim, kernels in ((2, {4, 3, 2}), (3, {4, 3})):
        got = {c.persistent for c in tc.CONT if c.group == "P" and c.scen.dim == dim}
        assert got == kernels and all(c.scen in pc.SCENARIOS for c in tc.CONT if c.group == "P")
    # the first solve stops before, on and after a check; every count is a snapshot
    assert {m1 % pc.CHECK for m1, _ in tc.SPLITS_ROWS} >= {5, 0, 1} and {m1 % pc.CHECK for m1, _ in tc.SPLITS_QP0} == {5, 0, 1}
    assert {m1 + m2 for m1, m2 in tc.SPLITS_ROWS} == {2, 12} and {m1 + m2 for m1, m2 in tc.SPLITS_QP0} == {12}
    assert {m for s in tc.SPLITS_ROWS + tc.SPLITS_QP0 for m in s + (sum(s),)} <= set(tc.CONT_STEPS)


@pytest.mark.parametrize("case", tc.CONT, ids=_ids(tc.CONT))
def test_continuation_case(case):
    sc = case.scen
    prob, x0, eta, l_col, dist, W = tc.problem(case)
    assert prob.K == sc.K
    if case.group == "P":  # a case of the persistent table: that kernel runs this scenario
        assert any(c.scen == sc and c.kernel == case.persistent for c in pc.CASES) and case.pipeline == pc.PIPELINE[case.persistent]
        assert pc.block_entries(prob, W, pc.apb(case.persistent, sc.dim)).max() <= pc.entry_cap(case.persistent, sc.N, sc.K, sc.dim)
    else:
        assert case.pipeline == qc.expected_pipeline(sc.K, sc.N * sc.dim, case.rows, case.cg_iters, case.use_mfma)
        assert case.pipeline == {"A": "three-launch", "B": "three-launch-bigK", "C": "generic",
                                 "D": "qp0" if sc.K <= 120 else "generic"}[case.group]
    assert (W.size > 0) == case.rows
    st, g = pc.step_settings(12, cg_iters=case.cg_iters, margin=sc.margin), case.gpu_settings(12)
    for k in ("cg_iters", "max_iter", "check_termination", "eps_abs", "eps_rel"):
        assert getattr(st, k) == g[k], k
    assert not st.adaptive_rho and not g["adaptive_rho"] and (g["use_mfma"], g["persistent"]) == (case.use_mfma, case.persistent)
    snaps, info = tc.cont_snapshots(case)
    assert info["status_val"] == -2 and info["iter"] == 12 and sorted(snaps) == sorted(tc.CONT_STEPS)
    if case.group == "C":
        assert info["cg_total"] == case.cg_iters * 12
    for m1, m2 in tc.splits(case):
        m = m1 + m2
        d = tc.cont_d(case, m)
        assert 100.0 * d <= FLOOR_MAX, (m, d)
        tol = lambda ref: pc.tolerances(prob, ref, snaps[m]["rho"], floor=100.0 * d)
        # a second solve that had reset would end in the state after m2 steps alone
        assert tc.worst_ratio(prob, snaps[m], snaps[m2], tol) > 100.0, (m1, m2)


# ---- 2. rows joining a live state ---------------------------------------------------------------------------------------------
def test_round_two_table_covers_the_pipelines():
    a = {(c.scen.dim, qc.band(c.scen.K), c.persistent) for c in tc.ROUND2 if c.group == "A"}
    assert {(2, b, p) for b in ("65..96", "97..120") for p in (0, 1)} | {(3, "65..96", 0)} <= a
    b = {(c.scen.dim, c.scen.K) for c in tc.ROUND2 if c.group == "B"}
    assert (2, 121) in b and any(dim == 3 and K > 120 for dim, K in b)
    assert {(c.cg_iters, c.use_mfma) for c in tc.ROUND2 if c.group == "C"} == {(2, 1), (3, 0)}
    assert [qc.band(c.scen.K) for c in tc.QP0_ROWS] == ["<=64", "65..96", "121..1024"]
    assert all(c.scen.margin == tc.NO_ROWS and c.persistent == 0 for c in tc.QP0_ROWS)
    for c in tc.ROUND2 + tc.QP0_ROWS:
        assert c.pipeline == c.pipeline_of(True) == {"A": "three-launch", "B": "three-launch-bigK", "C": "generic"}[c.group]
    assert [c.pipeline_of(False) for c in tc.QP0_ROWS] == ["qp0", "qp0", "generic"]
    # the clone cases: A with the global inverse, B, C, and every persistent kernel at K <= 64
    assert [(c.group, qc.band(c.scen.K)) for c in tc.CLONE_R2[:3]] == [("A", "97..120"), ("B", "121..1024"), ("C", "<=64")]
    assert [(c.group, c.persistent, qc.band(c.scen.K)) for c in tc.CLONE_R2[3:]] == [("P", k, "<=64") for k in (4, 3, 2)]
    assert all(c.scen.dim == 2 for c in tc.CLONE_R2 if c.persistent == 2)  # (kernel 2 is 2-D only)


R2_RUNS = one_per_oracle_run(tc.ROUND2 + tc.QP0_ROWS + tc.CLONE_R2)


@pytest.mark.parametrize("case", R2_RUNS, ids=_ids(R2_RUNS))
def test_round_two_case(case):
    sc, cg = case.scen, case.cg_iters
    prob, x0, eta, l_col, dist, W1 = pc.setup(sc)
    r2 = tc.round_two(sc, cg)
    io, n1 = r2.info, r2.n1
    assert io["status_val"] == 1 and io["rounds"] >= 2 and io["added"][0] > 0 and io["iter"] > n1 + max(tc.R2_STEPS)
    assert (W1.size == 0) == (sc.margin == tc.NO_ROWS)
    assert r2.snaps[n1]["round"] == 1 and all(r2.snaps[n1 + m]["round"] == 2 for m in tc.R2_STEPS)
    new = tc.added_rows(sc, cg)
    assert new.size == io["added"][0] and np.array_equal(r2.snaps[n1]["rows"], W1)
    # the C oracle ends round 1 at the same step (the floor's d compares like with like)
    _, i1 = co.admm(prob, eta, l_col, dist, x0=x0, st=tc.r2_settings(sc, cg, tc.MAX_ITER, max_rounds=1))
    assert i1["iter"] == n1 and i1["status_val"] == 1
    for c in tc.CLONE_R2:  # the persistent kernels that run this scenario: both working sets fit the LDS entry tables
        if c.group == "P" and (c.scen, c.cg_iters) == (sc, cg):
            per = pc.apb(c.persistent, sc.dim)
            assert pc.block_entries(prob, r2.snaps[n1 + 1]["rows"], per).max() <= pc.entry_cap(c.persistent, sc.N, sc.K, sc.dim)
    # an added row at an agent in another 16-column block than an old row's agent (no old rows: the added ones span two)
    assert sc.N * sc.dim > 16
    blocks = lambda rows: {frozenset(qc.column_blocks(int(a), sc.dim)) for a in np.concatenate(qo.working_rows(prob, rows)[1:])}
    assert any(bn != bo for bn in blocks(new) for bo in (blocks(W1) if W1.size else blocks(new)))
    ctl = tc.r2_controls(sc, cg)
    assert all(np.array_equal(ctl["never"][n1][k], r2.snaps[n1][k]) for k in ("x", "zc", "yc"))  # round 1, bit for bit
    for m in tc.R2_STEPS:
        assert 100.0 * tc.r2_d(sc, cg, m) <= FLOOR_MAX, (m, tc.r2_d(sc, cg, m))
        base, tol = r2.snaps[n1 + m], tc.r2_tolerances(sc, cg, m)
        assert np.array_equal(ctl["joined"][n1 + m]["rows"], base["rows"])
        assert tc.worst_ratio(prob, base, ctl["joined"][n1 + m], tol) > 100.0, ("rows in the set from step 0", m)
        never = ctl["never"][n1 + m]
        if W1.size:  # (the rows the two runs share)
            shared = dict(base, **{k: base[k][np.searchsorted(base["rows"], W1)] for k in ("rows", "zc", "yc")})
            assert tc.worst_ratio(prob, shared, never, tol) > 100.0, ("rows never join", m)
        else:
            assert tc.worst_ratio(prob, base, never, tol, ("x", "zf", "yf")) > 100.0, ("rows never join", m)


# ---- 3. adaptive rho on the host path -------------------------------------------------------------------------------------
def test_rho_table():
    assert [(c.group, c.persistent, c.cg_iters, c.use_mfma) for c in tc.RHO] == [("A", 0, 1, 1), ("B", 0, 1, 1), ("C", 0, 2, 1)]
    assert [qc.band(c.scen.K) for c in tc.RHO] == ["97..120", "121..1024", "65..96"] and tc.RHO_STEPS == (55, 100)
    st = tc.rho_settings(tc.RHO[0], 55)
    assert st.adaptive_rho and st.check_fine == 5 and st.eps_abs == st.eps_rel == 1e-12 and st.adaptive_rho_interval == 50
    # the clone after the update: at 55, continued to 100 (no further test of rho: the second solve counts from 0)
    assert tc.CLONE_RHO_SPLIT[0] == 55 and sum(tc.CLONE_RHO_SPLIT) == 100 and tc.CLONE_RHO_SPLIT[1] < st.adaptive_rho_interval


@pytest.mark.parametrize("case", tc.RHO, ids=_ids(tc.RHO))
def test_rho_case(case):
    prob = pc.setup(case.scen)[0]
    for m in tc.RHO_STEPS:
        snaps, info, d = tc.rho_run(case, m)
        assert snaps[50]["rho"] != qo.Settings().rho and info["rho_updates"] >= 1 and info["iter"] == m
        assert info["status_val"] == -2 and 100.0 * d <= FLOOR_MAX, (m, d)
        off, ioff, _ = tc.rho_run(case, m, False)
        assert ioff["rho_updates"] == 0 and off[m]["rho"] == qo.Settings().rho
        tol = lambda ref: pc.tolerances(prob, ref, snaps[m]["rho"], floor=100.0 * d)
        assert tc.worst_ratio(prob, snaps[m], off[m], tol) > 100.0, m
    # (the clone at 55 carries the rho of step 50 to step 100: the oracle does not change it again on the way)
    if case is tc.RHO[0]:
        assert tc.rho_run(case, 100)[0][100]["rho"] == tc.rho_run(case, 55)[0][55]["rho"]


# ---- 4. the clone cases -------------------------------------------------------------------------------------------------------
def test_clone_tables():
    assert [(c.group, c.persistent) for c in tc.CLONE_PLAIN] == [("A", 0), ("P", 3)] and set(tc.CLONE_PLAIN) <= set(tc.CONT)
    assert tc.CLONE_SPLIT in tc.SPLITS_ROWS
    src, other = tc.CLONE_USED
    assert src in tc.CONT and (other.N, other.K, other.dim) == (src.scen.N, src.scen.K, src.scen.dim) and other != src.scen
    assert not np.array_equal(pc.setup(other)[5], pc.setup(src.scen)[5]) and tc.CLONE_USED_RHO != qo.Settings().rho
    e = tc.CLONE_ERR
    shape = lambda c: (c.scen.N, c.scen.K, c.scen.dim)
    assert shape(e["K"])[1] != shape(e["src"])[1] and shape(e["K"])[::2] == shape(e["src"])[::2]
    assert shape(e["N"])[0] != shape(e["src"])[0] and shape(e["N"])[1:] == shape(e["src"])[1:]
    assert shape(e["same"]) == shape(e["src"]) and pc.setup(e["src"].scen)[5].size > 1
    for c in e.values():  # each solves a fresh problem afterwards: one step against the oracle
        assert 1 in tc.cont_snapshots(c)[0] and 100.0 * tc.cont_d(c, 1) <= FLOOR_MAX
