"""CPU checks behind tests/test_box_iterates_gpu.py: every case of tests/box_cases.py keeps the claims the table makes, the
table covers the shapes and pipelines it is there for, the d_box rule tracks the numpy-vs-C-oracle distance it stands in for,
and the comparison can fail: the oracle without the last agent's box leaves the tolerance of the GPU comparison."""
import time

import numpy as np
import pytest

import box_cases as bc
import corridor_ref as cr
import persist_cases as pc
import pipeline_cases as qc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_case_keeps_its_claims(case):
    from path_planning.solvers.scp import check_position_boxes

    sc = case.scen
    prob, x0, eta, l_col, dist, W = bc.problem(case)
    N, K, D = prob.N, prob.K, prob.D
    C = N * D
    assert K == sc.K and case.pattern in bc.PATTERNS
    assert case.pipeline == bc.expected_pipeline(K, C, case.rows, case.persistent, case.cg_iters, case.use_mfma)
    assert (W.size > 0) == case.rows and (case.start == "qp0") == case.rows
    lo, hi = bc.case_boxes(case)
    got = check_position_boxes(N, K, D, prob.pos_min, prob.pos_max, lo, hi)
    assert np.array_equal(got[0], lo) and np.array_equal(got[1], hi)
    # the boxed oracle run: quick, and every compared step is reached (no termination, no certificate)
    t0 = time.perf_counter()
    snaps, info = bc._boxed.__wrapped__(*bc._key(case), False)
    assert time.perf_counter() - t0 < 10.0
    assert info["status_val"] == -2 and info["iter"] == max(case.steps) and sorted(snaps) == sorted(case.steps)
    if case.rows:
        assert np.array_equal(snaps[max(case.steps)]["rows"], W)
    free, _ = bc.free_snapshots(case)
    n_wg, n_blk = -(-N // case.apb), -(-C // 16)
    for m in case.steps:
        what = f"{case.id} m={m}"
        ref_free = pc.reference_arrays(prob, free[m])
        if m == 1:  # z starts as A x unclamped and y = 0: a box first acts on x in step 2
            assert np.array_equal(free[m]["x"], snaps[m]["x"]), what
            continue
        act = bc.active_boxed(case, m)
        assert (act[:, 0] == N - 1).any(), (what, "no active boxed row at the last agent")
        assert {int(a) // case.apb for a in act[:, 0]} == set(range(n_wg)), (what, "workgroups")
        assert {(int(a) * D + int(d)) // 16 for a, _, d in act} == set(range(n_blk)), (what, "16-column blocks")
        differ = bc.worst_ratio(prob, snaps[m], ref_free, snaps[m]["rows"], ("x",), 100.0 * bc.d_box(case, m))
        assert differ >= bc.DIFFER_MIN, (what, differ)
        if case.pattern == "all-states":  # many rows of one column on their bounds at once
            assert (act[:, 0] == 0).sum() >= 8, (what, int((act[:, 0] == 0).sum()))


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_patterns_are_what_they_say(case):
    prob = bc.problem(case)[0]
    N, K, D = prob.N, prob.K, prob.D
    lo, hi = bc.case_boxes(case)
    # state 0 carries no box -- but for the wider-than-the-workspace entries of "mixed", which nothing may read
    assert case.pattern == "mixed" or (np.isinf(lo[:, 0]).all() and np.isinf(hi[:, 0]).all())
    fl, fh = np.isfinite(lo), np.isfinite(hi)
    inside = (fl & (lo > prob.pos_min)) | (fh & (hi < prob.pos_max))  # entries that tighten the workspace
    agents = range(1, N) if case.pattern == "all-states" else range(N)
    for i in agents:
        assert inside[i].sum() == 1
    if case.pattern == "slab":
        assert np.array_equal(fl, fh) and np.allclose((hi - lo)[fl], bc.SLAB, rtol=0, atol=1e-12)
    elif case.pattern == "mixed":
        wider = (fl & (lo < prob.pos_min)) | (fh & (hi > prob.pos_max))
        assert wider.sum() > 0 and (~fl).sum() > 0 and (~fh).sum() > 0
        b, base = so.fixed_bounds(prob, (lo, hi))["pos"], so.fixed_bounds(prob)["pos"]
        k = np.argwhere(wider[:, 1:] & ~inside[:, 1:])
        for s in (0, 1):  # the workspace wins there: the row keeps its box-free bound, bit for bit
            assert np.array_equal(b[s][k[:, 0], k[:, 1], k[:, 2]], base[s][k[:, 0], k[:, 1], k[:, 2]])
    elif case.pattern == "all-states":
        assert fl[0, 1:].all() and fh[0, 1:].all() and np.allclose((hi - lo)[0, 1:], 2 * bc.ALL_HALF, rtol=0, atol=1e-12)
    else:
        assert (fl ^ fh)[inside].all() and inside.sum() == N
    # the bounds the GPU test compares "lf" / "uf" with: the position rows are those of the bound overwrite, bit for bit
    lf, uf = (a.reshape(4 * K - 1, N * D) for a in bc.oracle_bounds(case))
    wl, wu = cr.position_rows(K, prob.h, np.concatenate([prob.pos_min, prob.pos_max]), prob.p0, prob.v0, lo, hi)
    r0 = 3 * K - 1
    assert np.array_equal(lf[r0:r0 + K - 1].view(np.uint64), wl.view(np.uint64))
    assert np.array_equal(uf[r0:r0 + K - 1].view(np.uint64), wu.view(np.uint64))
    assert (lf <= uf).all()


def test_table_covers_the_shapes_and_pipelines():
    def shapes(group, **kw):
        return {(c.scen.N, c.scen.dim, c.scen.K) for c in bc.CASES
                if c.group == group and all(getattr(c, k) == v for k, v in kw.items())}

    assert len(bc.CASES) <= 48 and len({c.id for c in bc.CASES}) == len(bc.CASES)
    assert {c.pattern for c in bc.CASES} == set(bc.PATTERNS)
    for g in ("P", "D"):
        assert {c.pattern for c in bc.CASES if c.group == g} == set(bc.PATTERNS)
    assert {c.group for c in bc.CASES if c.pattern == "all-states"} == {"P", "T", "D"}
    assert {c.scen.dim for c in bc.CASES if c.pattern == "all-states"} == {2, 3}
    p = shapes("P")
    assert {(N, 2, 50) for N in (7, 8, 9, 17, 33)} | {(9, 2, K) for K in (3, 16, 17, 64)} <= p
    assert {(N, 3, 50) for N in (4, 5, 9)} | {(5, 3, K) for K in (16, 17, 64)} <= p
    assert {N % 8 for N, D, K in p if D == 2} >= {7, 0, 1} and max(-(-N // 8) for N, D, K in p if D == 2) == 5
    assert {N % 4 for N, D, K in p if D == 3} >= {0, 1}
    for c in bc.CASES:
        if c.group == "P":
            assert c.pipeline == "persistent" and c.persistents == (1, 2, 3, 4)
            for per in c.persistents:  # whatever settings.persistent says
                assert bc.expected_pipeline(c.scen.K, c.scen.N * c.scen.dim, True, per) == "persistent"
        elif c.group == "T":
            assert c.pipeline == "three-launch" and c.persistents == (0,) and (c.scen.N, c.scen.dim, c.scen.K) in p
    assert len(shapes("T")) == 2 and {D for _, D, _ in shapes("T")} == {2, 3}
    a = shapes("A")
    assert {(N, 2, K) for N in (8, 9) for K in (65, 120)} | {(6, 3, 65), (6, 3, 120)} <= a
    assert {c.pipeline for c in bc.CASES if c.group == "A"} == {"three-launch"}
    assert {K for _, _, K in shapes("B")} == {121, 250}
    assert {c.pipeline for c in bc.CASES if c.group == "B"} == {"three-launch-bigK"}
    for K in (50, 65):
        assert (9, 2, K) in shapes("C", cg_iters=2, use_mfma=1) and (9, 2, K) in shapes("C", cg_iters=3, use_mfma=0)
    assert {c.pipeline for c in bc.CASES if c.group == "C"} == {"generic"}
    for start in ("zero", "random"):
        d = {c.scen.K: c for c in bc.CASES if c.group == "D" and c.start == start}
        assert {50, 65, 120, 121} <= set(d)
        assert all(c.cg_iters == 1 and c.steps == bc.STEPS_QP0 for c in d.values())
        assert [d[K].pipeline for K in (50, 65, 120, 121)] == ["qp0", "qp0", "qp0", "generic"]
    assert {c.pipeline for c in bc.CASES} == {"persistent", "three-launch", "three-launch-bigK", "generic", "qp0"}


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_settings_match_gpu_side(case):
    m = max(case.steps)
    st = case.oracle_settings(m)
    for per in case.persistents:
        g = case.gpu_settings(m, per)
        for k in ("cg_iters", "max_iter", "check_termination", "eps_abs", "eps_rel"):
            assert getattr(st, k) == g[k], k
        assert bool(st.adaptive_rho) == bool(g["adaptive_rho"]) and not st.adaptive_rho
        assert (g["use_mfma"], g["persistent"], g["check_termination"]) == (case.use_mfma, per, pc.CHECK)
    assert st.margin == case.scen.margin


CALIBRATION = (pc.RHO_2D, pc.TABLE_2D[3][0], bc._find(pc.TABLE_3D, 9, 50))


@pytest.mark.parametrize("sc", CALIBRATION, ids=lambda s: s.label)
def test_d_box_rule_tracks_d_m(sc):
    """On box-free QPs, where both exist, the perturbation distance lies within a factor 4 of pipeline_cases.d_m (numpy against
    the C oracle) at every m of pc.STEPS (measured: within 1.6)."""
    assert [s.label for s in CALIBRATION] == ["circle2d-N17-K50-s17", "circle2d-N9-K50-s9", "near3d-N9-K50-s3501"]
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    d = bc.perturbation_distance(prob, x0, eta, l_col, dist, W, pc.step_settings(max(pc.STEPS), margin=sc.margin), pc.STEPS)
    snaps, _ = pc.oracle_snapshots(sc, pc.STEPS, margin=sc.margin)
    for m in pc.STEPS:
        d_m = float(np.abs(qc._d_m(sc, 1, "qp0", m) - snaps[m]["x"]).max())
        print(f"{sc.label} m={m}: d_m {d_m:.2e}, perturbation {d[m]:.2e}, ratio {d[m] / d_m:.2f}")
        assert d_m / 4.0 <= d[m] <= 4.0 * d_m, (m, d_m, d[m])


CONTROL = [next(c for c in bc.CASES if c.group == g) for g in bc.GROUPS]


@pytest.mark.parametrize("case", CONTROL, ids=lambda c: c.id)
def test_the_comparison_can_fail(case):
    """The oracle WITHOUT the box of the last agent, pushed through the comparison of the GPU test (bc.worst_ratio): above 1.0
    at every m >= 2 -- what the GPU control shows of a solve that was never given that box."""
    prob, x0, eta, l_col, dist, W = bc.problem(case)
    lo, hi = bc.drop_agent(*bc.case_boxes(case), prob.N - 1)
    assert not np.array_equal(lo, bc.case_boxes(case)[0]) or not np.array_equal(hi, bc.case_boxes(case)[1])
    other, _ = bc._run(prob, x0, eta, l_col, dist, W, case.oracle_settings(max(case.steps)), case.steps, (lo, hi))
    snaps, _ = bc.snapshots(case)
    for m in case.steps:
        got, floor = pc.reference_arrays(prob, other[m]), 100.0 * bc.d_box(case, m)
        r = bc.worst_ratio(prob, snaps[m], got, snaps[m]["rows"], bc.STATE, floor)
        assert r > 1.0, (case.id, m, r)  # (m = 1: in z and y of the row itself; x follows in step 2)
        assert (bc.worst_ratio(prob, snaps[m], got, snaps[m]["rows"], ("x",), floor) > 1.0) == (m > 1), (case.id, m)


@pytest.mark.parametrize("name", sorted(bc.SCP_SHAPES))
def test_scp_shapes_solve_on_the_oracle(name):
    """the boxed SCP scenarios of tests/test_box_scp_gpu.py: the host check accepts the waypoint boxes, every QP of the boxed
    oracle loop ends "solved" within 10 s, the loop iterates, and the boxes move the plan and are active at its end"""
    from path_planning.solvers.scp import check_position_boxes

    n, dim = bc.SCP_SHAPES[name][:2]
    p0, pf, space, prob, lo, hi, free = bc.scp_scenario(name)
    assert (prob.N, prob.D) == (n, dim) and prob.K <= 40
    check_position_boxes(prob.N, prob.K, prob.D, prob.pos_min, prob.pos_max, lo, hi)
    t0 = time.perf_counter()
    out = qo.scp_solve(prob, 15, qo.Settings(max_iter=10000), pos_boxes=(lo, hi))
    assert time.perf_counter() - t0 < 10.0
    assert [i["status_val"] for i in out["infos"]] == [1] * len(out["infos"]) and out["iterations"] >= 1
    excess = float(np.maximum(lo - out["positions"], out["positions"] - hi)[np.isfinite(lo)].max())
    assert np.abs(out["positions"] - free).max() > 0.15 and -1e-3 < excess <= 3e-2, excess
