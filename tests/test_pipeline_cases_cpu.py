"""CPU checks behind tests/test_pipeline_iterates_gpu.py: every case of tests/pipeline_cases.py reaches the edge it claims,
the table covers the shapes and thresholds it is there for, the oracle runs with the GPU side's settings, and the comparison
can fail: an oracle with one working row dropped, or with one column's S0 x read as zero for a single step, leaves the
tolerance of the GPU comparison by more than a factor 100 at every compared step.  (The QP#0 cases have no rows, so the two
controls do not apply to them.)"""
import numpy as np
import pytest

import persist_cases as pc
import pipeline_cases as qc
from oracle import qp_oracle as qo

ARRAYS = ("x", "zf", "yf", "zc", "yc")


@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c.id)
def test_case_reaches_its_edge(case):
    sc = case.scen
    prob, x0, eta, l_col, dist, W = qc.problem(case)
    C = sc.N * sc.dim
    assert prob.K == sc.K and abs(sc.T - sc.K * qc.H) < 1e-8
    assert (C % 16, sc.K % 16, qc.band(sc.K)) == (case.c_tail, case.k_tail, case.band)
    assert case.pipeline == qc.expected_pipeline(sc.K, C, case.rows, case.cg_iters, case.use_mfma)
    want = {"A": ("65..96", "97..120"), "B": ("121..1024", ">1024"), "C": qc.BANDS, "D": qc.BANDS[:4]}[case.group]
    assert case.band in want
    if case.group == "A":
        assert case.pipeline == "three-launch" and case.persistent in (0, 1)
    elif case.group == "B":
        assert case.pipeline == ("three-launch-bigK" if sc.K <= 1024 else "generic")
    elif case.group == "C":
        assert case.pipeline == "generic" and (case.cg_iters > 1 or case.use_mfma != 1)
    else:
        assert case.pipeline == ("qp0" if sc.K <= 120 else "generic") and W.size == 0
    # every compared step is reached: no termination, no certificate
    snaps, info = qc.snapshots(case)
    assert info["status_val"] == -2 and info["iter"] == max(case.steps) and sorted(snaps) == sorted(case.steps)
    if case.group == "C":
        assert info["cg_total"] == case.cg_iters * max(case.steps)  # (what the GPU test asserts of cg_iters_total)
    if not case.rows:
        return
    assert W.size > 0 and np.array_equal(snaps[max(case.steps)]["rows"], W)
    _, wi, wj = qo.working_rows(prob, W)
    if C > 16:  # a working row joins two agents whose columns lie in different 16-column blocks
        assert any(qc.column_blocks(int(a), sc.dim) != qc.column_blocks(int(b), sc.dim) for a, b in zip(wi, wj))
    assert np.any((wi == sc.N - 1) | (wj == sc.N - 1))  # a row at the last agent ...
    assert qc.active_last_rows(case).size > 0  # ... that is active (A x < l) at every compared step


def test_table_covers_the_shapes_and_thresholds():
    def shapes(group, **kw):
        return {(c.scen.N, c.scen.dim, c.scen.K) for c in qc.CASES
                if c.group == group and all(getattr(c, k) == v for k, v in kw.items())}

    for p in (0, 1):  # A: both settings of `persistent`
        a = shapes("A", persistent=p)
        assert {(9, 2, K) for K in (65, 80, 96, 97, 120)} <= a
        assert {(N, D, K) for N, D in ((8, 2), (9, 2), (17, 2), (6, 3), (11, 3)) for K in (65, 120)} <= a
    b = shapes("B")
    assert {(N, D, K) for N, D in ((9, 2), (6, 3)) for K in (121, 128, 129, 250)} | {(3, 2, 1024), (3, 2, 1025)} <= b
    assert {c.steps for c in qc.CASES if c.scen.K >= 1024} == {qc.STEPS_1024}
    for cg, mf in qc.CG_MFMA:  # C: every settings pair at K = 50 in 2-D, every K with (2, 1), both dimensions
        assert (9, 2, 50) in shapes("C", cg_iters=cg, use_mfma=mf)
    assert {(N, D, K) for N, D in ((9, 2), (5, 3)) for K in (17, 50, 65, 130)} <= shapes("C", cg_iters=2, use_mfma=1)
    for start in ("zero", "random"):  # D: reset(None) and reset(x0)
        d = shapes("D", start=start)
        assert {(9, 2, K) for K in (3, 50, 64, 65, 120, 121)} <= d
        assert {(N, D, K) for N, D in ((8, 2), (17, 2), (6, 3), (11, 3)) for K in (65, 120)} <= d
        assert {c.steps for c in qc.CASES if c.group == "D"} == {qc.STEPS_QP0}
    # every pipeline bit outside the persistent kernels (tests/persist_cases.py) and the retired "fused" one is asserted by name
    assert {c.pipeline for c in qc.CASES} == {"three-launch", "three-launch-bigK", "generic", "qp0"}
    # both sides of 96 | 97, 120 | 121 and 1024 | 1025 with rows, of 64 | 65 and 120 | 121 without (64 with rows: the control
    # rows of tests/test_persist_iterates_gpu.py)
    with_rows = {c.scen.K for c in qc.CASES if c.rows and c.cg_iters == 1 and c.use_mfma == 1}
    assert {65, 96, 97, 120, 121, 1024, 1025} <= with_rows and 64 in {s.K for s in pc.SCENARIOS}
    assert {64, 65, 120, 121} <= {c.scen.K for c in qc.CASES if not c.rows}
    assert {96, 97} <= set(qc.KKT_K) and sorted(qc.EVICT_SCEN) == [50, 97]
    assert all(sc.K == K for K, sc in qc.EVICT_SCEN.items()) and len(set(qc.EVICT_RHOS)) == 34 > 32


@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c.id)
def test_settings_match_gpu_side(case):
    m = max(case.steps)
    st, g = case.oracle_settings(m), case.gpu_settings(m)
    for k in ("cg_iters", "max_iter", "check_termination", "eps_abs", "eps_rel"):
        assert getattr(st, k) == g[k], k
    assert bool(st.adaptive_rho) == bool(g["adaptive_rho"]) and not st.adaptive_rho
    assert (g["use_mfma"], g["persistent"], g["check_termination"]) == (case.use_mfma, case.persistent, qc.CHECK)
    assert st.sigma == qc.SIGMA and st.margin == case.scen.margin


def _worst(case, m, base, other, rows_other=None):
    """largest |base - other| / (tolerance of the GPU comparison) over the compared arrays after m steps"""
    prob = qc.problem(case)[0]
    order = None if rows_other is None else np.searchsorted(base["rows"], rows_other)
    ra, rb = pc.reference_arrays(prob, base, order), pc.reference_arrays(prob, other)
    tol = qc.case_tolerances(case, m, ra)
    return max(float(np.max(np.abs(ra[k] - rb[k]) / tol[k], initial=0.0)) for k in ARRAYS)


ROW_CASES = list({(c.scen, c.cg_iters, c.steps): c for c in qc.CASES if c.rows}.values())  # one per oracle run


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c.id)
def test_sensitivity_control(case):
    """(a) The oracle without the most active working row at the last agent, (b) the oracle whose collision rows read S0 x of
    the last agent's first column as zero during step 1: after every compared step some compared array differs from the true
    state by more than 100 x what the GPU comparison allows it (pc.tolerances with the floor 100 d_m).  (In (a) the rows the
    two runs share are compared.)"""
    prob, x0, eta, l_col, dist, W = qc.problem(case)
    base, _ = qc.snapshots(case)
    r = int(qc.active_last_rows(case)[0])
    kw = dict(cg_iters=case.cg_iters, margin=case.scen.margin)
    dropped, _ = pc.oracle_snapshots(case.scen, case.steps, rows=W[W != r], **kw)
    stale, _ = pc.oracle_snapshots(case.scen, case.steps, zero_qx=(1, (prob.N - 1) * prob.D), **kw)
    for m in case.steps:
        assert _worst(case, m, base[m], dropped[m], dropped[m]["rows"]) > 100.0, ("row dropped", m, r)
        assert _worst(case, m, base[m], stale[m]) > 100.0, ("S0 x zeroed", m)
