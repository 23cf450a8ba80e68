"""Whole solves of joint QPs with per-state position boxes against the boxed QP oracle, on the three pipelines such a QP takes
at K <= 64: the round-2 persistent kernel, the three-launch pipeline (settings.persistent = 0) and the generic one
(cg_iters = 2).  Each test mirrors a box-free one of tests/test_persist_iterates_gpu.py / tests/test_transitions_gpu.py.

The reference is qo.admm_structured(pos_boxes=...).  The C oracle takes no boxes, so where those tests use the numpy-vs-C
distance d, these use box_cases.perturbation_distance: the boxed numpy oracle against its rerun from x0 (1 + 2^-52 s)."""
import functools

import numpy as np
import pytest

import box_cases as bc
import persist_cases as pc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so
from test_pipeline_iterates_gpu import compare_state, load, new_qp, peek_state
from test_transitions_gpu import ERR_CAPACITY, add, violated
from test_transitions_gpu import new_qp as new_qp_cap

pytestmark = pytest.mark.gpu
LEAN = {"persistent16", "persistent8-lean"}
PIPES = {"persistent": dict(persistent=1, cg_iters=1), "three-launch": dict(persistent=0, cg_iters=1),
         "generic": dict(persistent=1, cg_iters=2)}
RATIOS = {}  # (what, pipeline) -> largest error / tolerance seen


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def set_problem(ctx, qp, prob):
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(pc.LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))


def names_of(pipe):
    return bc.STATE + (bc.CARRIED if pipe != "generic" else ())


# ---- adaptive rho across an update, boxed -------------------------------------------------------------------------------
# 3-D, N = 9 (4 + 4 + 1 agents), K = 50, the "mixed" pattern.  Chosen with the oracle: an active box keeps the primal residual
# up, so the box-free update at step 50 does not happen -- on no scenario and pattern tried; here rho first changes at step 250,
# with one and with two PCG steps.
LONG = pc.Scenario("grid", 51, 9, 50, 3)
LONG_PATTERN = "mixed"
RHO_STEPS = (55, 100, 255, 300)  # 55 / 100: the steps of the box-free test (no update crossed here); 255 / 300: past the first one


@functools.lru_cache(maxsize=None)
def long_boxes():
    prob, x0 = pc.setup(LONG)[:2]
    pos, _ = so.kinematics(prob, x0)
    return bc.boxes(LONG_PATTERN, LONG.seed, pos, prob.pos_min, prob.pos_max)


@functools.lru_cache(maxsize=None)
def rho_reference(cg, m):
    """(oracle state after m steps, info, d) of a solve with max_iter = m: adaptive rho on, check_fine = 5, eps = 1e-12"""
    prob, x0, eta, l_col, dist, W = pc.setup(LONG)
    st = qo.Settings(cg_iters=cg, max_rounds=1, eps_abs=1e-12, eps_rel=1e-12, adaptive_rho=True, check_fine=5, max_iter=m,
                     margin=LONG.margin)
    snaps, info = bc._run(prob, x0, eta, l_col, dist, W, st, (m,), long_boxes())
    noisy, _ = bc._run(prob, bc._ulp_noise(x0), eta, l_col, dist, W, st, (m,), long_boxes())
    return snaps[m], info, float(np.abs(snaps[m]["x"] - noisy[m]["x"]).max())


@pytest.mark.parametrize("pipe", PIPES)
def test_rho_switch_and_adaptive_cadence(ctx, pipe):
    """tests/test_persist_iterates_gpu.py::test_rho_switch_and_adaptive_cadence with boxes: per m a fresh object, two solves
    (the first meets a new rho on the host path; on the second the persistent kernel has its blocks cached and switches by
    itself).  Tolerance: floor 100 d under pc.tolerances, d the perturbation distance of the same solve."""
    prob, x0, eta, l_col, dist, W = pc.setup(LONG)
    lo, hi = (ctx.tensor(a) for a in long_boxes())
    cg = PIPES[pipe]["cg_iters"]
    assert rho_reference(cg, 100)[1]["rho_updates"] == 0 and rho_reference(cg, 255)[1]["rho_updates"] >= 1
    for m in RHO_STEPS:
        snap, im, d = rho_reference(cg, m)
        qp = new_qp(ctx, prob, eps_abs=1e-12, eps_rel=1e-12, check_fine=5, max_iter=m, **PIPES[pipe])
        try:
            qp.set_position_boxes(lo, hi)
            for solve in ("host path", "in kernel"):
                load(ctx, qp, x0, W, eta, l_col)
                info = qp.solve()
                what = f"{pipe} ({LONG.label}, {LONG_PATTERN}) m={m} rho switch {solve}"
                assert pipe in info["pipeline"].split("+") and not set(info["pipeline"].split("+")) & LEAN, (what, info)
                assert info["iter"] == m and info["rho_updates"] == im["rho_updates"], (what, info, im)
                assert info["rho"] == snap["rho"], (what, info["rho"], snap["rho"])
                worst = compare_state(qp, prob, snap, W, names_of(pipe), 100.0 * d, what)
                RATIOS["rho", pipe, m] = max(RATIOS.get(("rho", pipe, m), 0.0), worst)
                print(f"box-rho {pipe} m={m} {solve}: rho {info['rho']:.4f}, {info['rho_updates']} updates, d={d:.2e}, "
                      f"max err/tol = {worst:.3g}")
                if pipe == "persistent":
                    if solve == "host path" or im["rho_updates"] == 0:
                        assert info["rho_switches_in_kernel"] == 0, (what, info)
                    else:
                        assert 1 <= info["rho_switches_in_kernel"] <= im["rho_updates"], (what, info)
        finally:
            qp.close()


# ---- solved, and iteration caps ------------------------------------------------------------------------------------------
# The joint QP of SCP iteration 2 of the boxed 3-D grid swap (box_cases.SCP_SHAPES["grid3d"]: N = 8, K = 20, waypoint boxes on
# vehicles 0, 3, 6, 7).  Chosen with the oracle: "solved" after 55 steps across the rho update at step 50, with one and with
# two PCG steps, four boxed entries on their bounds at the solution.  (The step-level patterns do not serve: with a bound
# 0.25 m inside x0 none of them reaches "solved" within 1500 steps at N = 9 .. 17, and none that does crosses an update.)
SOLVED = ("grid3d", 2)
CAP_EVERY = 5  # (the spacing of the box-free test; it includes the caps 25 and 50)


def scp_qp(which, cg):
    name, it = which
    return bc.scp_joint_qp(name, cg, it) + (bc.scp_scenario(name)[4:6],)


@functools.lru_cache(maxsize=None)
def solved_reference(cg):
    """(x, info, d, {cap: status}) of the oracle; d: the same solve from the perturbed start"""
    prob, x0, eta, l_col, dist, W, pb = scp_qp(SOLVED, cg)
    kw = dict(rows0=W, pos_boxes=pb)
    st = qo.Settings(cg_iters=cg, max_iter=10000, max_rounds=1)
    xo, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, **kw)
    xn, _, inn = qo.admm_structured(prob, eta, l_col, dist, x0=bc._ulp_noise(x0), st=st, **kw)
    assert inn["iter"] == io["iter"]
    caps = {cap: qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=qo.Settings(cg_iters=cg, max_iter=cap, max_rounds=1),
                                    **kw)[2]["status_val"] for cap in range(CAP_EVERY, io["iter"], CAP_EVERY)}
    return xo, io, float(np.abs(xo - xn).max()), caps


@pytest.mark.parametrize("pipe", PIPES)
def test_solved_and_iteration_cap(ctx, pipe):
    """tests/test_persist_iterates_gpu.py::test_solved_and_iteration_cap with boxes: status, iter, rho_updates and working
    rows as the oracle, x within max(1e-8, 100 d); every cap below the solve's length gives the oracle's status, 2 and -2
    both among them.  The QP: SCP iteration 2 of the boxed 3-D grid swap (N = 8, K = 20, waypoint boxes), 55 steps with the rho
    update at step 50 (one PCG step: d = 2.6e-8, the GPU 7e-9 off the oracle; two: 9e-14 and 7e-14)."""
    cg = PIPES[pipe]["cg_iters"]
    prob, x0, eta, l_col, dist, W, (lo, hi) = scp_qp(SOLVED, cg)
    xo, io, d, caps = solved_reference(cg)
    assert io["status_val"] == 1 and io["rho_updates"] >= 1 and io["iter"] <= 1500
    assert io["working_rows"] == W.size + io["added"][0]
    pos, _ = so.kinematics(prob, xo)
    assert ((np.abs(np.maximum(lo - pos, pos - hi)) < 3e-2) & np.isfinite(lo)).sum() >= 2  # boxes active at the solution
    assert {2, -2} <= set(caps.values()) and {25, 50} <= set(caps)
    qp = new_qp(ctx, prob, max_iter=10000, **PIPES[pipe])
    try:
        qp.set_position_boxes(ctx.tensor(lo), ctx.tensor(hi))
        load(ctx, qp, x0, W, eta, l_col)
        info = qp.solve()
        assert info["pipeline"] == pipe, info
        assert (info["status_val"], info["iter"], info["rho_updates"], info["working_rows"]) == (
            1, io["iter"], io["rho_updates"], W.size), (info, io)
        err = float(np.abs(qp.solution().cpu().numpy() - xo).max())
        print(f"box-solved {pipe}: {info['iter']} steps, {info['rho_updates']} rho updates, d={d:.2e}, "
              f"max |x - oracle| = {err:.3e}")
        assert err <= max(1e-8, 100 * d)
        for cap, status in caps.items():
            qp.update_settings(max_iter=cap)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            assert pipe in info["pipeline"].split("+") and not set(info["pipeline"].split("+")) & LEAN, (cap, info)
            assert info["status_val"] == status and info["iter"] == cap, (cap, info, status)
    finally:
        qp.close()


# ---- rows join a live boxed state; the clone -------------------------------------------------------------------------------
# The joint QP of SCP iteration 2 of the boxed N = 10, K = 40 scenario (two workgroups): round 1 ends "solved" and leaves out
# rows its solution violates; they join the live state.
ROUND2 = ("n10", 2)
R2_STEPS = (1, 6, 7)


@functools.lru_cache(maxsize=None)
def round_two_reference(cg):
    """(x, info, n1, new rows, {m: snapshot n1 + m}, {m: d}) of the oracle's rounds"""
    prob, x0, eta, l_col, dist, W1, pb = scp_qp(ROUND2, cg)
    run = lambda start, **kw: qo.admm_structured(prob, eta, l_col, dist, x0=start, pos_boxes=pb, **kw)
    xo, yo, io = run(x0, st=qo.Settings(cg_iters=cg, max_iter=10000))
    n1 = run(x0, st=qo.Settings(cg_iters=cg, max_iter=10000, max_rounds=1))[2]["iter"]
    st = qo.Settings(cg_iters=cg, max_iter=n1 + max(R2_STEPS))
    snaps, noisy = {}, {}
    run(x0, st=st, snapshots={n1 + m for m in R2_STEPS}, snap_out=snaps)
    run(bc._ulp_noise(x0), st=st, snapshots={n1 + m for m in R2_STEPS}, snap_out=noisy)
    assert all(snaps[n1 + m]["round"] == noisy[n1 + m]["round"] == 2 for m in R2_STEPS)
    d = {m: float(np.abs(snaps[n1 + m]["x"] - noisy[n1 + m]["x"]).max()) for m in R2_STEPS}
    return xo, io, n1, np.setdiff1d(snaps[n1 + 1]["rows"], W1), {m: snaps[n1 + m] for m in R2_STEPS}, d


def boxed(ctx, qp, lo, hi):
    qp.set_position_boxes(ctx.tensor(lo), ctx.tensor(hi))
    return qp


@pytest.mark.parametrize("pipe", PIPES)
def test_constraint_generation_round_two(ctx, pipe):
    """tests/test_persist_iterates_gpu.py::test_constraint_generation_round_two with boxes: rounds, working rows and steps as
    the oracle, the final x at 1e-8, and the state 1, 6 and 7 steps into round 2 against the oracle's snapshots."""
    cg = PIPES[pipe]["cg_iters"]
    prob, x0, eta, l_col, dist, W1, (lo, hi) = scp_qp(ROUND2, cg)
    xo, io, n1, new, snaps, d = round_two_reference(cg)
    assert io["rounds"] >= 2 and io["added"][0] == new.size > 0 and io["status_val"] == 1
    feas_tol, max_rounds = qo.Settings().feas_tol, qo.Settings().max_rounds

    def gpu_rounds(qp, cap2=None):
        rows = W1.copy()
        qp.update_settings(max_iter=10000)
        load(ctx, qp, x0, rows, eta, l_col)
        pipes, total, rounds = set(), 0, 0
        while True:
            info = qp.solve()
            rounds += 1
            total += info["iter"]
            pipes.update(info["pipeline"].split("+"))
            if cap2 is not None and rounds == 2:
                return rows, rounds, total, pipes, info
            fresh = violated(prob, qp, eta, l_col, rows)
            if fresh.size == 0 or rounds >= max_rounds:
                return rows, rounds, total, pipes, info
            add(ctx, qp, fresh, eta, l_col)
            rows = np.concatenate([rows, fresh])
            qp.update_settings(max_iter=cap2 if cap2 is not None else 10000 - total)

    assert feas_tol == 1e-6
    qp = boxed(ctx, new_qp(ctx, prob, max_iter=10000, **PIPES[pipe]), lo, hi)
    try:
        rows, rounds, total, pipes, info = gpu_rounds(qp)
        assert pipe in pipes and not pipes & LEAN and (pipe == "three-launch" or "three-launch" not in pipes), pipes
        assert (rounds, rows.size, total) == (io["rounds"], io["working_rows"], io["iter"]), (rounds, rows.size, total, io)
        np.testing.assert_allclose(qp.solution().cpu().numpy(), xo, rtol=0, atol=1e-8)
        for m in R2_STEPS:
            rows, rounds, total, pipes, info = gpu_rounds(qp, cap2=m)
            assert total == n1 + m and info["iter"] == m and np.array_equal(np.sort(rows[W1.size:]), new)
            assert info["pipeline"] == pipe, info["pipeline"]
            what = f"{pipe} ({ROUND2[0]}, SCP iteration {ROUND2[1]}) round 2 m={m}"
            worst = compare_state(qp, prob, snaps[m], rows, names_of(pipe), 100.0 * d[m], what)
            RATIOS["round 2", pipe, m] = worst
            print(f"box-round-two {pipe} n1={n1} m={m} d={d[m]:.2e} max err/tol = {worst:.3g}")
    finally:
        qp.close()


@pytest.mark.parametrize("pipe", PIPES)
def test_clone_when_the_rows_do_not_fit(ctx, pipe):
    """tests/test_transitions_gpu.py::test_clone_when_the_rows_do_not_fit with boxes.  The twin never hears of the boxes but
    through take_state_of: it reports no lean pipeline, its lf / uf are the source's bit for bit, and its next m steps with the
    round-2 rows are the oracle's."""
    from path_planning import _hip

    cg = PIPES[pipe]["cg_iters"]
    prob, x0, eta, l_col, dist, W1, (lo, hi) = scp_qp(ROUND2, cg)
    xo, io, n1, new, snaps, d = round_two_reference(cg)
    rows = np.concatenate([W1, new])
    src = boxed(ctx, new_qp_cap(ctx, prob, row_capacity=W1.size, max_iter=10000, **PIPES[pipe]), lo, hi)
    try:
        load(ctx, src, x0, W1, eta, l_col)
        i1 = src.solve()
        assert (i1["pipeline"], i1["iter"], i1["status_val"]) == (pipe, n1, 1), i1
        assert np.array_equal(violated(prob, src, eta, l_col, W1), new)
        before = peek_state(src)
        with pytest.raises(_hip.HipError) as err:
            add(ctx, src, new, eta, l_col)
        assert err.value.code == ERR_CAPACITY, err.value
        after = peek_state(src)
        assert all(np.array_equal(before[k], after[k]) for k in bc.STATE)
        bounds = {k: src.peek(k).cpu().numpy() for k in ("lf", "uf")}
        for m in R2_STEPS:
            what = f"{pipe} ({ROUND2[0]}) cloned after round 1, m={m}"
            dst = new_qp_cap(ctx, prob, max_iter=10000, **PIPES[pipe])  # (set_problem only: no boxes of its own)
            try:
                dst.take_state_of(src)
                for k in ("lf", "uf"):
                    np.testing.assert_array_equal(dst.peek(k).cpu().numpy().view(np.uint64), bounds[k].view(np.uint64))
                add(ctx, dst, new, eta, l_col)
                dst.update_settings(max_iter=m)
                info = dst.solve()
                assert (info["pipeline"], info["iter"], info["working_rows"]) == (pipe, m, rows.size), (what, info)
                assert info["rho"] == i1["rho"] == snaps[m]["rho"], (what, info["rho"], i1["rho"])
                worst = compare_state(dst, prob, snaps[m], rows, names_of(pipe), 100.0 * d[m], what)
                RATIOS["clone", pipe, m] = worst
                print(f"box-clone {pipe} n1={n1} m={m} d={d[m]:.2e} max err/tol = {worst:.3g}")
            finally:
                dst.close()
    finally:
        src.close()


# ---- primal infeasible by a box ------------------------------------------------------------------------------------------
INFEASIBLE = bc._find(pc.TABLE_2D, 9, 16)  # near2d-N9-K16-s2161


@functools.lru_cache(maxsize=None)
def infeasible_case():
    """The last agent's state 2 (t = 0.4 s) must lie 3 m beyond where x0 has it: out of reach at 2 m/s, yet the box is not
    empty inside the workspace, so the host check lets it pass.  -> (lo, hi, {cg_iters: oracle info})"""
    from path_planning.solvers.scp import check_position_boxes

    prob, x0, eta, l_col, dist, W = pc.setup(INFEASIBLE)
    N, K, D = prob.N, prob.K, prob.D
    pos, _ = so.kinematics(prob, x0)
    lo, hi = np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)
    lo[N - 1, 2, 0] = pos[N - 1, 2, 0] + 3.0
    check_position_boxes(N, K, D, prob.pos_min, prob.pos_max, lo, hi)
    infos = {}
    for cg in (1, 2):
        st = qo.Settings(cg_iters=cg, max_iter=10000, max_rounds=1, margin=INFEASIBLE.margin)
        infos[cg] = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W, pos_boxes=(lo, hi))[2]
    return lo, hi, infos


@pytest.mark.parametrize("pipe", PIPES)
def test_primal_infeasible_by_a_box(ctx, pipe):
    """Status -3 on every pipeline; iter as the oracle's with two PCG steps, within +-50 of it with one (the allowance
    tests/test_scp_gpu.py::test_scp_matches_oracle grants the single-PCG-step path).  The same QP object after a fresh
    set_problem and set_position_boxes(None, None) solves: the box alone made it infeasible."""
    assert INFEASIBLE.label == "near2d-N9-K16-s2161"
    prob, x0, eta, l_col, dist, W = pc.setup(INFEASIBLE)
    lo, hi, infos = infeasible_case()
    cg = PIPES[pipe]["cg_iters"]
    io = infos[cg]
    assert io["status_val"] == -3, io
    qp = new_qp(ctx, prob, max_iter=10000, **PIPES[pipe])
    try:
        qp.set_position_boxes(ctx.tensor(lo), ctx.tensor(hi))
        load(ctx, qp, x0, W, eta, l_col)
        info = qp.solve()
        print(f"box-infeasible {pipe}: status {info['status_val']} at step {info['iter']} (oracle {io['iter']}), "
              f"{info['pipeline']}")
        assert info["pipeline"] == pipe, info
        assert info["status_val"] == -3, (info, io)
        assert (info["iter"] == io["iter"]) if cg > 1 else (abs(info["iter"] - io["iter"]) <= 50), (info, io)
        set_problem(ctx, qp, prob)
        qp.set_position_boxes(None, None)
        load(ctx, qp, x0, W, eta, l_col)
        free = qp.solve()
        assert free["status_val"] in (1, 2), free
    finally:
        qp.close()


def test_report_margins(record_property):
    """largest error / tolerance per (test, pipeline, m) over the tests above (pytest -rA or --junitxml shows them)"""
    for (what, pipe, m), r in sorted(RATIOS.items()):
        record_property(f"{what} {pipe} m={m}", f"{r:.3g}")
        print(f"box-solve-margin {what:8s} {pipe:14s} m={m:4d} max err/tol = {r:.3g}")
