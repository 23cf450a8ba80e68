"""What happens between two solves of one QP object, step by step, against the QP oracle (cases: tests/transition_cases.py):

  1  a second scp_qp_solve without a reset, on every pipeline;
  2  rows joining a live state (constraint generation, round two), and QP#0 followed by rows;
  3  the adaptive-rho update on the host path beyond K = 64, and the hit in the per-rho cache in a later solve;
  4  scp_qp_clone_state at each of those points, into fresh and used objects, and its error paths.

Every comparison is entry by entry on x, z / y of the fixed and the working collision rows, and on the carried F x and S0 x
where they are part of the state (the single-step pipelines and the persistent kernels).  Tolerance: pc.tolerances with the
floor 100 d, d = the largest difference in x between the numpy and the C oracle after the same total number of steps with the
same settings, rounds and margin.  Nothing is fitted to the GPU's result; tests/test_transition_cases_cpu.py shows that each
comparison fails by more than a factor 100 on the state a wrong transition would leave.

Measured on an MI355X, largest error / tolerance: second solve 0.21 (QP#0 on the generic pipeline, K = 121), 0.11 (qp0), at
most 0.04 with rows; rows join 0.28 (bigK, K = 121), 0.21 (three-launch, K = 80), 0.04 (generic); QP#0 then rows 0.22 (K =
129); rho update 0.08 / 0.05 / 0.01 (bigK / three-launch / generic), cached equal to built; clone 0.28 (bigK, rows join), at
most 0.04 elsewhere (test_report_margins lists all of them)."""
import numpy as np
import pytest

import persist_cases as pc
import transition_cases as tc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so
from test_pipeline_iterates_gpu import CARRIED, STATE, compare_state, load, peek_state

pytestmark = pytest.mark.gpu
RATIOS = {}  # (transition, pipeline, K) -> largest error / tolerance seen
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -3, -4  # include/scp_hip.h


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def new_qp(ctx, prob, row_capacity=None, **st):
    from path_planning import _hip

    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**st), row_capacity=row_capacity)
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(pc.LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    return qp


def add(ctx, qp, rows, eta, l_col):
    import torch

    rows = np.asarray(rows, dtype=np.int64)
    qp.add_rows(torch.as_tensor(rows, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[rows]), ctx.tensor(l_col[rows]))


def names_of(case):
    return STATE + (CARRIED if case.carries else ())


def record(transition, case, worst):
    key = (transition, case.pipeline, case.scen.K)
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)


def violated(prob, qp, eta, l_col, rows):
    """the rows outside `rows` that the solution violates (the oracle's constraint-generation test)"""
    viol = so.collision_apply(prob, eta, qp.solution().cpu().numpy().ravel()) < l_col - qo.Settings().feas_tol
    viol[rows] = False
    return np.nonzero(viol)[0]


# ---- 1. a second solve without a reset ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CONT, ids=lambda c: c.id)
def test_second_solve_without_reset(ctx, case):
    """reset, rows, m1 steps; max_iter = m2, solve again: the oracle's state after m1 + m2 steps (fixed rho, eps = 1e-12: the
    checks cannot change the state, so the restart of the step count and of the check cadence is immaterial)"""
    prob, x0, eta, l_col, dist, W = tc.problem(case)
    snaps, _ = tc.cont_snapshots(case)
    qp = new_qp(ctx, prob, **case.gpu_settings(1))
    try:
        for m1, m2 in tc.splits(case):
            what = f"{case.pipeline} ({case.id}) {m1} + {m2} steps"
            qp.update_settings(max_iter=m1)
            load(ctx, qp, x0, W, eta, l_col)
            first = qp.solve()
            assert first["pipeline"] == case.pipeline and first["iter"] == m1, (what, first)
            qp.update_settings(max_iter=m2)
            info = qp.solve()
            assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
            assert info["iter"] == m2 and info["status_val"] == -2 and info["working_rows"] == W.size, (what, info)
            if case.group == "C":
                assert info["cg_iters_total"] == case.cg_iters * m2, (what, info)
            d = tc.cont_d(case, m1 + m2)
            worst = compare_state(qp, prob, snaps[m1 + m2], W, names_of(case), 100.0 * d, what)
            record("second solve", case, worst)
            print(f"transition second-solve {case.id} {m1}+{m2} d={d:.2e} max err/tol = {worst:.3g}")
    finally:
        qp.close()


# ---- 2. rows joining a live state ---------------------------------------------------------------------------------------------
def run_rounds(ctx, qp, prob, x0, eta, l_col, W1, cap2=None):
    """the oracle's rounds on one QP object: solve, add the violated rows to the live state, solve again; cap2: stop after a
    second solve of cap2 steps.  Returns the rows in the GPU's order and every solve's info."""
    rows, infos = W1.copy(), []
    qp.update_settings(max_iter=tc.MAX_ITER)
    load(ctx, qp, x0, rows, eta, l_col)
    while True:
        infos.append(qp.solve())
        if cap2 is not None and len(infos) == 2:
            return rows, infos
        new = violated(prob, qp, eta, l_col, rows)
        if new.size == 0 or len(infos) >= qo.Settings().max_rounds:
            return rows, infos
        add(ctx, qp, new, eta, l_col)
        rows = np.concatenate([rows, new])
        qp.update_settings(max_iter=cap2 if cap2 is not None else tc.MAX_ITER - sum(i["iter"] for i in infos))


@pytest.mark.parametrize("case", tc.ROUND2 + tc.QP0_ROWS, ids=lambda c: c.id)
def test_rows_join_a_live_state(ctx, case):
    """Round 1 converges at the default eps and leaves out rows its solution violates (the QP#0 cases: it has no rows at all);
    they join the live state.  Rounds, working rows and steps of the complete run as the oracle's, round 1 in the oracle's n1
    steps, and the state 1, 6 and 7 steps into round 2 against the oracle's snapshots at n1 + m."""
    sc, cg = case.scen, case.cg_iters
    prob, x0, eta, l_col, dist, W1 = pc.setup(sc)
    r2 = tc.round_two(sc, cg)
    io, n1 = r2.info, r2.n1
    pipes = [case.pipeline_of(W1.size > 0)] + [case.pipeline] * (io["rounds"] - 1)
    qp = new_qp(ctx, prob, **case.gpu_default_settings())
    try:
        rows, infos = run_rounds(ctx, qp, prob, x0, eta, l_col, W1)
        assert [i["pipeline"] for i in infos] == pipes, (case.id, infos)
        assert (len(infos), rows.size, sum(i["iter"] for i in infos)) == (io["rounds"], io["working_rows"], io["iter"]), (infos, io)
        assert infos[0]["iter"] == n1 and infos[-1]["status_val"] == 1, (infos, n1)
        for m in tc.R2_STEPS:
            what = f"{case.pipeline} ({case.id}) round 2 m={m}"
            rows, infos = run_rounds(ctx, qp, prob, x0, eta, l_col, W1, cap2=m)
            assert [i["iter"] for i in infos] == [n1, m] and [i["pipeline"] for i in infos] == pipes[:2], (what, infos)
            assert infos[1]["working_rows"] == r2.snaps[n1 + m]["rows"].size, (what, infos)
            d = tc.r2_d(sc, cg, m)
            worst = compare_state(qp, prob, r2.snaps[n1 + m], rows, names_of(case), 100.0 * d, what)
            record("rows join" if W1.size else "QP#0 then rows", case, worst)
            print(f"transition round-two {case.id} n1={n1} m={m} d={d:.2e} max err/tol = {worst:.3g}")
    finally:
        qp.close()


# ---- 3. adaptive rho on the host path -------------------------------------------------------------------------------------
def rho_gpu_settings(case, max_iter):
    return dict(cg_iters=case.cg_iters, use_mfma=case.use_mfma, persistent=case.persistent, eps_abs=1e-12, eps_rel=1e-12,
                check_fine=5, max_iter=max_iter)


@pytest.mark.parametrize("case", tc.RHO, ids=lambda c: c.id)
def test_rho_update_on_the_host_path(ctx, case):
    """adaptive rho on, check_fine = 5, m = 55 and 100: past the update at step 50.  A fresh object per m; its first solve
    meets the new rho with no cached blocks (qp_on_rho_changed(false) + scp_qp_build_kkt drop the carried row values and
    build at the new rho_c), its second finds them in the per-rho cache.  Both end in the oracle's state at m."""
    prob, x0, eta, l_col, dist, W = pc.setup(case.scen)
    for m in tc.RHO_STEPS:
        snaps, im, d = tc.rho_run(case, m)
        qp = new_qp(ctx, prob, **rho_gpu_settings(case, m))
        try:
            for solve in ("blocks built", "blocks cached"):
                what = f"{case.pipeline} ({case.id}) m={m} rho update, {solve}"
                load(ctx, qp, x0, W, eta, l_col)
                info = qp.solve()
                assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
                assert info["iter"] == m and info["rho_updates"] == im["rho_updates"], (what, info, im)
                assert info["rho"] == snaps[m]["rho"], (what, info["rho"], snaps[m]["rho"])
                worst = compare_state(qp, prob, snaps[m], W, names_of(case), 100.0 * d, what)
                record(f"rho update, {solve}", case, worst)
                print(f"transition rho {case.id} m={m} {solve} d={d:.2e} max err/tol = {worst:.3g}")
        finally:
            qp.close()


# ---- 4. scp_qp_clone_state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CLONE_R2, ids=lambda c: c.id)
def test_clone_when_the_rows_do_not_fit(ctx, case):
    """The source's row capacity is exactly its round-1 working set.  Adding the round-2 rows fails with SCP_ERR_CAPACITY and
    leaves the source's state bit for bit; a larger object takes the state, the rows and m steps: the oracle's state at
    n1 + m, at the source's rho, on the case's pipeline (after a persistent exit: the persistent kernel again)."""
    from path_planning import _hip

    sc, cg = case.scen, case.cg_iters
    prob, x0, eta, l_col, dist, W1 = pc.setup(sc)
    r2 = tc.round_two(sc, cg)
    n1, new = r2.n1, tc.added_rows(sc, cg)
    rows = np.concatenate([W1, new])
    src = new_qp(ctx, prob, row_capacity=W1.size, **case.gpu_default_settings())
    try:
        load(ctx, src, x0, W1, eta, l_col)
        i1 = src.solve()
        assert (i1["pipeline"], i1["iter"], i1["status_val"]) == (case.pipeline, n1, 1), (case.id, i1)
        assert np.array_equal(violated(prob, src, eta, l_col, W1), new)
        before = peek_state(src)
        with pytest.raises(_hip.HipError) as err:
            add(ctx, src, new, eta, l_col)
        assert err.value.code == ERR_CAPACITY, err.value
        after = peek_state(src)
        assert all(np.array_equal(before[k], after[k]) for k in STATE), case.id
        for m in tc.R2_STEPS:
            what = f"{case.pipeline} ({case.id}) cloned after round 1, m={m}"
            dst = new_qp(ctx, prob, **case.gpu_default_settings())
            try:
                dst.take_state_of(src)
                add(ctx, dst, new, eta, l_col)
                dst.update_settings(max_iter=m)
                info = dst.solve()
                assert (info["pipeline"], info["iter"], info["working_rows"]) == (case.pipeline, m, rows.size), (what, info)
                assert info["rho"] == i1["rho"] == r2.snaps[n1 + m]["rho"], (what, info["rho"], i1["rho"])
                d = tc.r2_d(sc, cg, m)
                worst = compare_state(dst, prob, r2.snaps[n1 + m], rows, names_of(case), 100.0 * d, what)
                record("clone, rows join", case, worst)
                print(f"transition clone-round-two {case.id} n1={n1} m={m} d={d:.2e} max err/tol = {worst:.3g}")
            finally:
                dst.close()
    finally:
        src.close()


@pytest.mark.parametrize("case", tc.CLONE_PLAIN, ids=lambda c: c.id)
def test_clone_without_new_rows(ctx, case):
    """clone after m1 steps, m2 steps on the clone: the oracle's state after m1 + m2; the source stays usable and, continued
    by m2 steps itself, ends there too (each against the oracle: the source may still hold S0 x and F x of its last check,
    the clone rebuilds them, so the two need not agree bit for bit)"""
    prob, x0, eta, l_col, dist, W = tc.problem(case)
    snaps, _ = tc.cont_snapshots(case)
    m1, m2 = tc.CLONE_SPLIT
    d = tc.cont_d(case, m1 + m2)
    src, dst = new_qp(ctx, prob, **case.gpu_settings(m1)), new_qp(ctx, prob, **case.gpu_settings(m2))
    try:
        load(ctx, src, x0, W, eta, l_col)
        first = src.solve()
        assert (first["pipeline"], first["iter"]) == (case.pipeline, m1), first
        dst.take_state_of(src)
        for qp, who in ((dst, "the clone"), (src, "the source")):
            what = f"{case.pipeline} ({case.id}) {m1} + {m2} steps, {who}"
            qp.update_settings(max_iter=m2)
            info = qp.solve()
            assert (info["pipeline"], info["iter"], info["working_rows"]) == (case.pipeline, m2, W.size), (what, info)
            worst = compare_state(qp, prob, snaps[m1 + m2], W, names_of(case), 100.0 * d, what)
            record(f"clone, no rows added: {who}", case, worst)
            print(f"transition clone-plain {case.id} {who} d={d:.2e} max err/tol = {worst:.3g}")
    finally:
        src.close()
        dst.close()


def test_clone_into_a_used_object(ctx):
    """dst has itself solved another scenario of the same shape, with another working set and another rho (set_rho): after
    the clone and the same continued steps every peeked array matches a clone into a fresh object bit for bit (and the
    oracle within tolerance) -- nothing of what dst held before survives: lists, carried values, cache slot, problem data."""
    case, other = tc.CLONE_USED
    prob, x0, eta, l_col, dist, W = tc.problem(case)
    prob_o, x0_o, eta_o, l_o, _, W_o = pc.setup(other)
    snaps, _ = tc.cont_snapshots(case)
    m1, m2 = tc.CLONE_SPLIT
    src = new_qp(ctx, prob, **case.gpu_settings(m1))
    used, fresh = new_qp(ctx, prob_o, **case.gpu_settings(3)), new_qp(ctx, prob, **case.gpu_settings(m2))
    try:
        load(ctx, used, x0_o, W_o, eta_o, l_o)
        used.set_rho(tc.CLONE_USED_RHO)
        iu = used.solve()
        assert (iu["pipeline"], iu["iter"], iu["rho"], iu["working_rows"]) == (case.pipeline, 3, tc.CLONE_USED_RHO, W_o.size), iu
        load(ctx, src, x0, W, eta, l_col)
        assert src.solve()["iter"] == m1
        states = []
        for dst in (used, fresh):
            dst.take_state_of(src)
            dst.update_settings(max_iter=m2)
            info = dst.solve()
            assert (info["pipeline"], info["iter"], info["rho"], info["working_rows"]) == (case.pipeline, m2, 0.1, W.size), info
            states.append(peek_state(dst, STATE + CARRIED))
        for name in STATE + CARRIED:
            assert np.array_equal(states[0][name], states[1][name]), name
        what = f"{case.pipeline} ({case.id}) cloned into a used object"
        worst = compare_state(used, prob, snaps[m1 + m2], W, names_of(case), 100.0 * tc.cont_d(case, m1 + m2), what)
        record("clone into a used object", case, worst)
    finally:
        for qp in (src, used, fresh):
            qp.close()


def test_clone_after_the_rho_update(ctx):
    """the source of part 3 stops at step 55, past its rho update; the clone rebuilds the KKT blocks for the source's rho (not
    settings.rho) and continues to step 100 (45 steps: no further test of rho on either side)"""
    case = tc.RHO[0]
    prob, x0, eta, l_col, dist, W = pc.setup(case.scen)
    m1, m2 = tc.CLONE_RHO_SPLIT
    s55, _, _ = tc.rho_run(case, m1)
    s100, i100, d = tc.rho_run(case, m1 + m2)
    src, dst = new_qp(ctx, prob, **rho_gpu_settings(case, m1)), new_qp(ctx, prob, **rho_gpu_settings(case, m2))
    try:
        load(ctx, src, x0, W, eta, l_col)
        first = src.solve()
        assert first["rho_updates"] == i100["rho_updates"] >= 1 and first["rho"] == s55[m1]["rho"] != 0.1, first
        dst.take_state_of(src)
        dst.update_settings(max_iter=m2)
        info = dst.solve()
        what = f"{case.pipeline} ({case.id}) cloned at step {m1}, continued to {m1 + m2}"
        assert (info["pipeline"], info["iter"], info["rho_updates"]) == (case.pipeline, m2, 0), (what, info)
        assert info["rho"] == first["rho"] == s100[m1 + m2]["rho"], (what, info["rho"], first["rho"])
        worst = compare_state(dst, prob, s100[m1 + m2], W, names_of(case), 100.0 * d, what)
        record("clone after the rho update", case, worst)
        print(f"transition clone-rho {case.id} d={d:.2e} max err/tol = {worst:.3g}")
    finally:
        src.close()
        dst.close()


def test_clone_error_paths(ctx):
    """another K or N: SCP_ERR_INVALID; a source without a reset: SCP_ERR_STATE; a capacity below the source's rows:
    SCP_ERR_CAPACITY.  After each, the object that refused still solves a fresh problem: one step against the oracle."""
    from path_planning import _hip

    cases = tc.CLONE_ERR
    prob, x0, eta, l_col, dist, W = tc.problem(cases["src"])
    src, unset = new_qp(ctx, prob, **cases["src"].gpu_settings(1)), new_qp(ctx, prob, **cases["src"].gpu_settings(1))
    qps = [src, unset]
    try:
        load(ctx, src, x0, W, eta, l_col)
        # (name of the refusing object, the sources it refuses and the code of each)
        for name, refused in (("K", [(src, ERR_INVALID)]), ("N", [(src, ERR_INVALID)]),
                              ("same", [(unset, ERR_STATE), (src, ERR_CAPACITY)])):
            case = cases[name]
            prob_d, x0_d, eta_d, l_d, _, W_d = tc.problem(case)
            dst = new_qp(ctx, prob_d, row_capacity=W.size - 1 if name == "same" else None, **case.gpu_settings(1))
            qps.append(dst)
            for source, code in refused:
                with pytest.raises(_hip.HipError) as err:
                    dst.take_state_of(source)
                assert err.value.code == code, (name, err.value)
            load(ctx, dst, x0_d, W_d, eta_d, l_d)
            info = dst.solve()
            what = f"{case.pipeline} ({case.id}) after a refused clone"
            assert (info["pipeline"], info["iter"], info["working_rows"]) == (case.pipeline, 1, W_d.size), (what, info)
            worst = compare_state(dst, prob_d, tc.cont_snapshots(case)[0][1], W_d, names_of(case), 100.0 * tc.cont_d(case, 1), what)
            record("after a refused clone", case, worst)
    finally:
        for qp in qps:
            qp.close()


def test_report_margins(record_property):
    """largest error / tolerance per (transition, pipeline, K) over the tests above (pytest -rA or --junitxml shows them)"""
    for (transition, pipe, K), r in sorted(RATIOS.items()):
        record_property(f"{transition}: {pipe} K={K}", f"{r:.3g}")
        print(f"transition-margin {transition:34s} {pipe:18s} K={K:4d} max err/tol = {r:.3g}")
