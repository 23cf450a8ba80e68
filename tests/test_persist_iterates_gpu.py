"""The persistent single-step ADMM kernels, step by step, against the QP oracle (cases: tests/persist_cases.py).

For every case and every m in STEPS, a solve with max_iter = m on the case's kernel must report that kernel in
info["pipeline"] and leave x, z / y of the fixed and the working collision rows, and the carried F x and S0 x, within
1e-11 * max(1, |oracle|_max) of the oracle's state after m steps.  The three-launch pipeline runs the same table as a
control.  Then, per kernel: adaptive rho across its first update (host path and in-kernel switch), solved, iteration
caps, primal infeasibility, constraint generation (2-D kernels) and the EXIT_OVERFLOW fallback."""
import numpy as np
import pytest

import persist_cases as pc
from oracle import c_oracle as co
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

pytestmark = pytest.mark.gpu
PEEK = ("x", "zf", "yf", "zc", "yc", "fx", "qx")
RATIOS = {}  # (kernel name, m) -> largest error / tolerance seen


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def new_qp(ctx, prob, **st):
    from path_planning import _hip

    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**st))
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(pc.LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    return qp


def load(ctx, qp, x0, rows, eta, l_col):
    qp.reset(ctx.tensor(x0))
    add(ctx, qp, rows, eta, l_col)


def add(ctx, qp, rows, eta, l_col):
    import torch

    rows = np.asarray(rows, dtype=np.int64)
    qp.add_rows(torch.as_tensor(rows, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[rows]), ctx.tensor(l_col[rows]))


def compare_state(qp, prob, snap, gpu_rows, what, tol_abs=0.0, record=None):
    """every peeked array against the oracle snapshot, entry by entry within pc.tolerances; the message names kernel, m,
    array and the worst index"""
    order = np.searchsorted(snap["rows"], gpu_rows)
    assert np.array_equal(snap["rows"][order], gpu_rows), what
    ref = pc.reference_arrays(prob, snap, order)
    tols = pc.tolerances(prob, ref, snap["rho"], floor=tol_abs)
    worst = 0.0
    for name in PEEK:
        got = qp.peek(name).cpu().numpy()
        r, tol = ref[name], tols[name]
        assert got.shape == r.shape, (what, name, got.shape, r.shape)
        q = np.abs(got - r) / tol
        i = int(np.argmax(q)) if q.size else 0
        worst = max(worst, float(q[i]) if q.size else 0.0)
        assert q.size == 0 or q[i] <= 1.0, (f"{what}: array {name}: |gpu - oracle| = {abs(got[i] - r[i]):.3e} > {tol[i]:.3e} "
                                            f"at {pc.where(prob, name, i, gpu_rows)} (gpu {got[i]!r}, oracle {r[i]!r})")
    if record is not None:
        RATIOS[record] = max(RATIOS.get(record, 0.0), worst)
    return worst


# ---- 3. the state after m steps ---------------------------------------------------------------------------------------
CONTROL = [pc.Case(sc, 0, 0, sc.K % 16) for sc in pc.SCENARIOS]


@pytest.mark.parametrize("case", pc.CASES + CONTROL, ids=lambda c: c.id)
def test_state_after_m_steps(ctx, case):
    sc = case.scen
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    snaps, _ = pc.cached_snapshots(sc)
    name = pc.kernel_name(case.kernel, sc.dim)
    qp = new_qp(ctx, prob, **pc.gpu_step_settings(case.kernel, 1))
    try:
        for m in case.steps:
            qp.update_settings(max_iter=m)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            what = f"{name} ({case.id}) m={m}"
            assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
            assert info["iter"] == m and info["status_val"] == -2, (what, info)
            compare_state(qp, prob, snaps[m], W, what, record=(name, m))
    finally:
        qp.close()


# ---- 4. longer runs and exit reasons, per kernel ------------------------------------------------------------------------
# a partial last workgroup in every shape: 2-D N = 17 (17 = 2 x 8 + 1 = 16 + 1), 3-D N = 9 (9 = 2 x 4 + 1 = 8 + 1)
LONG_3D = pc.Scenario("grid", 51, 9, 50, 3)  # (a rho update at step 50; numpy and C oracle within 2e-12 after 100 steps)
LONG = [(pc.RHO_2D, k) for k in (4, 3, 2)] + [(LONG_3D, k) for k in (4, 3)]
LONG_IDS = [f"p{k}-{sc.label}" for sc, k in LONG]


def long_settings(**kw):
    base = dict(cg_iters=1, max_rounds=1, eps_abs=1e-12, eps_rel=1e-12, adaptive_rho=True, check_fine=5)
    base.update(kw)
    return qo.Settings(**base)


@pytest.mark.parametrize("sc,kernel", LONG, ids=LONG_IDS)
def test_rho_switch_and_adaptive_cadence(ctx, sc, kernel):
    """adaptive rho on, check_fine = 5, m = 55 and 100: past the first rho update (step 50), on the host path (first solve:
    no cached blocks for the new rho) and inside the kernel (second solve of the same object).  Tolerance per m: floor
    100 d_m under pc.tolerances, d_m = the largest difference in x between the numpy and the C oracle after m steps (same
    settings, same margin): the oracle's own sensitivity to the order of summation.  No step count is cut."""
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    name = pc.kernel_name(kernel, sc.dim)
    for m in (55, 100):
        st = long_settings(max_iter=m, margin=sc.margin)
        snaps = {}
        _, _, im = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W, snapshots={50, m}, snap_out=snaps)
        assert snaps[50]["rho"] != qo.Settings().rho and im["rho_updates"] >= 1  # the update at step 50 is crossed
        xc, ic = co.admm(prob, eta, l_col, dist, x0=x0, st=st)
        assert ic["iter"] == m
        d_m = float(np.abs(xc - snaps[m]["x"]).max())
        # a fresh object per m: its first solve is the first to meet the new rho
        qp = new_qp(ctx, prob, cg_iters=1, persistent=kernel, eps_abs=1e-12, eps_rel=1e-12, check_fine=5, max_iter=m)
        try:
            for solve in ("host path", "in kernel"):
                load(ctx, qp, x0, W, eta, l_col)
                info = qp.solve()
                what = f"{name} ({sc.label}) m={m} rho switch {solve}"
                assert pc.PIPELINE[kernel] in info["pipeline"].split("+"), (what, info["pipeline"])
                assert info["iter"] == m and info["rho_updates"] == im["rho_updates"], (what, info, im)
                assert info["rho"] == snaps[m]["rho"], what
                compare_state(qp, prob, snaps[m], W, what, tol_abs=100 * d_m, record=(name, f"{m}-rho"))
                if solve == "host path":
                    assert info["rho_switches_in_kernel"] == 0, (what, info)
                else:  # the blocks of the new rho were cached: the kernel switched by itself at step 50
                    assert 1 <= info["rho_switches_in_kernel"] <= im["rho_updates"], (what, info)
        finally:
            qp.close()


@pytest.mark.parametrize("sc,kernel", LONG, ids=LONG_IDS)
def test_solved_and_iteration_cap(ctx, sc, kernel):
    """Solved at eps = 1e-3: status, iter, rho_updates and working rows as the numpy oracle, x within max(1e-8, 100 d), d =
    the numpy vs C oracle difference of the same solve (2-D N = 17: 75 steps across a rho update, d = 7e-10, the GPU 4e-8).  Iteration caps
    below that (every 5 steps): status 2 (solved inaccurate) and -2 at the same caps as the numpy and the C oracle."""
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    st = qo.Settings(cg_iters=1, max_iter=10000, max_rounds=1, margin=sc.margin)
    xo, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W)
    assert io["status_val"] == 1 and io["rho_updates"] >= 1
    # (with max_rounds = 1 the oracle still appends the rows its solution violates before it returns)
    assert io["working_rows"] == W.size + io["added"][0]
    qp = new_qp(ctx, prob, cg_iters=1, persistent=kernel, max_iter=10000)
    try:
        load(ctx, qp, x0, W, eta, l_col)
        info = qp.solve()
        assert info["pipeline"] == pc.PIPELINE[kernel]
        assert (info["status_val"], info["iter"], info["rho_updates"], info["working_rows"]) == (
            1, io["iter"], io["rho_updates"], W.size), (info, io)
        d = float(np.abs(co.admm(prob, eta, l_col, dist, x0=x0, st=st)[0] - xo).max())
        np.testing.assert_allclose(qp.solution().cpu().numpy(), xo, rtol=0, atol=max(1e-8, 100 * d))
        seen = set()
        for cap in range(5, io["iter"], 5):
            sti = qo.Settings(cg_iters=1, max_iter=cap, max_rounds=1, margin=sc.margin)
            _, _, ion = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=sti, rows0=W)
            _, ic = co.admm(prob, eta, l_col, dist, x0=x0, st=sti)
            qp.update_settings(max_iter=cap)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            assert pc.PIPELINE[kernel] in info["pipeline"].split("+")
            assert info["status_val"] == ion["status_val"] == ic["status_val"], (cap, info, ion, ic)
            assert info["iter"] == cap
            seen.add(info["status_val"])
        assert {2, -2} <= seen, seen
    finally:
        qp.close()


@pytest.mark.parametrize("kernel", [4, 3, 2])
def test_constraint_generation_round_two(ctx, kernel):
    """2-D N = 17, margin 0.05: round 1 leaves out rows its solution violates; they join the live state of the same QP
    object (round 2: the lean kernels' v = z~ + y / rho).  Rounds, working rows and steps as the oracle, the final x at
    1e-8, and the state 1, 6 and 7 steps into round 2 against the oracle's snapshots (floor 100 d, d = numpy vs C oracle
    at that step).  (No 3-D shape here: no 3-D case of the table adds rows in round 2.)"""
    sc = pc.RHO_2D
    prob, x0, eta, l_col, dist, _ = pc.setup(sc)
    st = qo.Settings(cg_iters=1, max_iter=10000, margin=0.05)
    xo, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st)
    assert io["rounds"] >= 2 and io["added"][0] > 0
    name = pc.kernel_name(kernel, sc.dim)
    W1 = np.nonzero(dist - prob.R < 0.05)[0]

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
            ax = so.collision_apply(prob, eta, qp.solution().cpu().numpy().ravel())
            viol = ax < l_col - st.feas_tol
            viol[rows] = False
            new = np.nonzero(viol)[0]
            if new.size == 0 or rounds >= st.max_rounds:
                return rows, rounds, total, pipes, info
            add(ctx, qp, new, eta, l_col)
            rows = np.concatenate([rows, new])
            qp.update_settings(max_iter=cap2 if cap2 is not None else 10000 - total)

    qp = new_qp(ctx, prob, cg_iters=1, persistent=kernel, max_iter=10000)
    try:
        rows, rounds, total, pipes, info = gpu_rounds(qp)
        assert pc.PIPELINE[kernel] in pipes and "three-launch" not in pipes, pipes
        assert (rounds, rows.size, total) == (io["rounds"], io["working_rows"], io["iter"]), (rounds, rows.size, total, io)
        np.testing.assert_allclose(qp.solution().cpu().numpy(), xo, rtol=0, atol=1e-8)
        n1 = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=qo.Settings(cg_iters=1, max_iter=10000, margin=0.05,
                                                                              max_rounds=1))[2]["iter"]
        steps = (1, 6, 7)
        snaps = {}
        qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=qo.Settings(cg_iters=1, max_iter=n1 + max(steps), margin=0.05),
                           snapshots={n1 + m for m in steps}, snap_out=snaps)
        for m in steps:
            assert snaps[n1 + m]["round"] == 2
            xc, _ = co.admm(prob, eta, l_col, dist, x0=x0, st=qo.Settings(cg_iters=1, max_iter=n1 + m, margin=0.05))
            d = float(np.abs(xc - snaps[n1 + m]["x"]).max())
            rows, rounds, total, pipes, info = gpu_rounds(qp, cap2=m)
            assert total == n1 + m and info["iter"] == m
            assert info["pipeline"] == pc.PIPELINE[kernel], info["pipeline"]
            compare_state(qp, prob, snaps[n1 + m], rows, f"{name} ({sc.label}) round 2 m={m}", tol_abs=100 * d,
                          record=(name, f"r2+{m}"))
    finally:
        qp.close()


def _cluster(N, dim, seed):
    """N agents on a sphere of radius 3 m crossing its centre: every pair comes within R"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(N, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p0 = 10.0 + 3.0 * u
    pf = 10.0 - 3.0 * u + rng.uniform(-0.3, 0.3, (N, dim))
    return so.make_problem(N, 10.0, 0.2, 0.8, [0.0] * dim + [20.0] * dim, p0, pf)


@pytest.mark.parametrize("kernel,dim", [(4, 2), (3, 2), (2, 2), (4, 3), (3, 3)])
def test_overflow_falls_back_and_reset_rearms(ctx, kernel, dim):
    """(a) Every collision row of a dense cluster (margin 1e9): the largest block of agents holds more than twice the
    kernel's LDS entry capacity (pc.entry_cap, the formula of scp_qp_cg1_persist), so the kernel leaves with EXIT_OVERFLOW
    and every step runs on the three-launch pipeline, with the oracle's state after 12 steps.  (c) After reset the same
    object runs a working set below half the capacity on the persistent kernel again, with the oracle's state.  (Case (b)
    of the issue, an overflow first met in round 2, is not covered.)"""
    N = 17
    prob = _cluster(N, dim, 5)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(eps_abs=1e-6, eps_rel=1e-6))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    per = pc.apb(kernel, dim)
    cap = pc.entry_cap(kernel, N, prob.K, dim)
    k_all = np.arange(prob.m_col) // (N * (N - 1) // 2)
    Wall = np.arange(prob.m_col)
    Wfit = np.nonzero((dist - prob.R < 0.0) & (k_all % 16 == 0))[0]
    assert pc.block_entries(prob, Wall, per).max() > 2 * cap
    assert Wfit.size > 0 and pc.block_entries(prob, Wfit, per).max() < cap / 2
    name = pc.kernel_name(kernel, dim)
    qp = new_qp(ctx, prob, **pc.gpu_step_settings(kernel, 12))
    try:
        for W, pipe in ((Wall, "three-launch"), (Wfit, pc.PIPELINE[kernel])):
            snaps = {}
            qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=pc.step_settings(12), rows0=W, snapshots={12},
                               snap_out=snaps)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            what = f"{name} cluster {dim}-D, {W.size} rows"
            assert info["pipeline"] == pipe and (info["persist_launches"] == 0) == (pipe == "three-launch"), (what, info)
            assert info["iter"] == 12 and info["status_val"] == -2, (what, info)
            compare_state(qp, prob, snaps[12], W, what, record=(name, "ovf" if pipe == "three-launch" else "ovf-reset"))
    finally:
        qp.close()


@pytest.mark.parametrize("kernel", [4, 3, 2])
def test_primal_infeasible_on_every_kernel(ctx, kernel):
    """The first linearised QP of the reference's demo (3 vehicles crossing in T = 3 s) is primal infeasible
    (tests/test_qp_gpu.py::test_primal_infeasibility_certificate): every kernel forced, status -3 at the oracle's step."""
    p0 = np.array([[-2.0, -2.0], [0.0, -2.0], [2.0, -2.0]])
    pf = np.array([[2.0, 2.0], [0.0, 2.0], [-2.0, 2.0]])
    prob = so.make_problem(3, 3.0, 0.2, 0.5, [-5, -5, 500, 200], p0, pf)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(max_iter=4000))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    st = qo.Settings(max_iter=10000, max_rounds=1)
    W = np.nonzero(dist - prob.R < st.margin)[0]
    _, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W)
    assert io["status_val"] == -3
    qp = new_qp(ctx, prob, cg_iters=1, persistent=kernel, max_iter=10000)
    try:
        load(ctx, qp, x0, W, eta, l_col)
        info = qp.solve()
        assert info["pipeline"] == pc.PIPELINE[kernel]
        assert info["status_val"] == -3 and info["iter"] == io["iter"], (info, io)
    finally:
        qp.close()


def test_report_margins(record_property):
    """largest error / tolerance per kernel and m over the tests above (pytest -rA or --junitxml shows them)"""
    for (name, m), r in sorted(RATIOS.items(), key=lambda t: (t[0][0], str(t[0][1]))):
        record_property(f"{name} m={m}", f"{r:.3g}")
        print(f"persist-margin {name:32s} m={m!s:>8s} max err/tol = {r:.3g}")
