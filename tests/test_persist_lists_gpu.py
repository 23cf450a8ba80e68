"""The persistent ADMM kernels with entry tables they build themselves (PersistArgs::own_lists) against the same kernels
loading the host-built incidence lists and row values (scp_qp_debug_set "persist_host_lists" = 1): bit for bit.

The same QP runs twice, hook off and hook on; after m in {1, 6, 7, 12} steps x, zf, yf, fx, qx, zc, yc must be array_equal
and the info fields the same.  The working sets are those of tests/test_persist_lists_cpu.py, which checks the numpy
statement of the tables and that every set has a cell with >= 3 entries (two entries of a cell commute in every sum: only
three detect a wrong order), a row inside one block of agents and a row across blocks; the assertions are repeated here on
the row list that is actually loaded.

Row values: the kernel's own first row values (rho_c z_c - y_c) - rho_c ax against rows_value_kernel<D, true> cannot be
read after zero steps (a launch with no step to run returns before the kernel starts), so they are compared through the
first iterate: m = 1, also at rho = 0.3 (collision-row rho = 3, so that a wrong association of the two products shows).
That is the equality of the state above, not a separate quantity."""
import numpy as np
import pytest

import persist_cases as pc
import test_persist_lists_cpu as ref

pytestmark = pytest.mark.gpu
PEEK = ("x", "zf", "yf", "fx", "qx", "zc", "yc")
INFO = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "r_prim", "r_dual", "rho", "pipeline",
        "persist_launches", "persist_gave_up", "rho_switches_in_kernel")
STEPS = (1, 6, 7, 12)


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def new_qp(ctx, prob, hook, **st):
    from path_planning import _hip

    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**st))
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(pc.LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    assert qp.debug_set("persist_host_lists", hook) == hook
    return qp


def load(ctx, qp, x0, batches, eta, l_col):
    import torch

    qp.reset(ctx.tensor(x0))
    for rows in batches:
        rows = np.asarray(rows, dtype=np.int64)
        qp.add_rows(torch.as_tensor(rows, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[rows]), ctx.tensor(l_col[rows]))


def states(ctx, prob, x0, eta, l_col, batches, kernel, hook, steps=STEPS, **st):
    """{m: ({array name: values}, info)} of one object: a fresh load and a solve of m steps per m"""
    qp = new_qp(ctx, prob, hook, **pc.gpu_step_settings(kernel, 1, **st))
    out = {}
    try:
        for m in steps:
            qp.update_settings(max_iter=m)
            load(ctx, qp, x0, batches, eta, l_col)
            info = qp.solve()
            out[m] = ({k: qp.peek(k).cpu().numpy() for k in PEEK}, {k: info[k] for k in INFO})
    finally:
        qp.close()
    return out


def assert_same(off, on, what):
    for m in off:
        assert off[m][1] == on[m][1], (what, m, off[m][1], on[m][1])
        for k in PEEK:
            a, b = off[m][0][k], on[m][0][k]
            assert a.shape == b.shape and np.array_equal(a, b), (
                f"{what} m={m}: array {k} differs in {int((a != b).sum())} of {a.size} values, "
                f"largest difference {float(np.abs(a - b).max()):.3e}")


SETS = [(case, kernel, label) for case in ref.CASES for kernel in case.kernels for label in ref.set_labels(case)]


@pytest.mark.parametrize("case,kernel,label", SETS, ids=lambda v: v.scen.label if isinstance(v, ref.ListCase) else str(v))
def test_own_tables_equal_host_lists(ctx, case, kernel, label):
    prob, x0, eta, l_col, _, _ = pc.setup(case.scen)
    batches = dict(ref.working_sets(case))[label]
    wk, wi, wj = ref.rows_of(prob, np.concatenate(batches))
    ref.assert_inputs_detect_order(prob.K, prob.N, wk, wi, wj, pc.apb(kernel, prob.D))
    what = f"{pc.kernel_name(kernel, prob.D)} {case.scen.label} {label}"
    off = states(ctx, prob, x0, eta, l_col, batches, kernel, 0)
    on = states(ctx, prob, x0, eta, l_col, batches, kernel, 1)
    for m in STEPS:
        assert off[m][1]["pipeline"] == pc.PIPELINE[kernel] and off[m][1]["iter"] == m, (what, off[m][1])
    assert_same(off, on, what)


@pytest.mark.parametrize("kernel", [4, 3, 2])
def test_first_row_values_at_rho_c_3(ctx, kernel):
    """rho = 0.3: rho_c z_c, rho_c ax are no longer the operands themselves (see the module docstring)"""
    case = ref.CASES[0]
    prob, x0, eta, l_col, _, W = pc.setup(case.scen)
    off = states(ctx, prob, x0, eta, l_col, [W], kernel, 0, steps=(1, 6), rho=0.3)
    on = states(ctx, prob, x0, eta, l_col, [W], kernel, 1, steps=(1, 6), rho=0.3)
    assert off[1][1]["pipeline"] == pc.PIPELINE[kernel] and off[1][1]["rho"] == 0.3
    assert_same(off, on, f"{pc.kernel_name(kernel, 2)} rho=0.3")


@pytest.mark.parametrize("kernel", [4, 3, 2])
def test_relaunch_in_one_solve_carries_the_row_values(ctx, kernel):
    """adaptive rho, 55 steps of a fresh object: the kernel returns at step 50 for blocks of a rho the host has not built
    yet and is launched again in the same solve; a second solve of the object switches inside the kernel.  Both as with
    host lists."""
    sc = pc.RHO_2D
    prob, x0, eta, l_col, _, W = pc.setup(sc)
    res = {}
    for hook in (0, 1):
        qp = new_qp(ctx, prob, hook, cg_iters=1, persistent=kernel, eps_abs=1e-12, eps_rel=1e-12, check_fine=5, max_iter=55)
        try:
            res[hook] = {}
            for solve in ("host path", "in kernel"):
                load(ctx, qp, x0, [W], eta, l_col)
                info = qp.solve()
                res[hook][solve] = ({k: qp.peek(k).cpu().numpy() for k in PEEK}, {k: info[k] for k in INFO})
        finally:
            qp.close()
    assert res[0]["host path"][1]["persist_launches"] >= 2 and res[0]["host path"][1]["rho_updates"] >= 1, res[0]
    assert res[0]["in kernel"][1]["rho_switches_in_kernel"] >= 1, res[0]
    assert_same(res[0], res[1], pc.kernel_name(kernel, 2))


@pytest.mark.parametrize("kernel", [4, 3, 2])
def test_overflow_decision_from_own_counts(ctx, kernel):
    """N = 16, K = 50, all 6000 rows: 6000 entries around a block of 8 agents, 12000 around the block of 16, capacities of
    1.1 - 1.3 k: every workgroup leaves on its own count, the three-launch pipeline runs, nobody gave up."""
    prob, x0, eta, l_col, _, _ = pc.setup(ref.OVERFLOW)
    W = np.arange(prob.m_col)
    off = states(ctx, prob, x0, eta, l_col, [W], kernel, 0, steps=(12,))
    on = states(ctx, prob, x0, eta, l_col, [W], kernel, 1, steps=(12,))
    info = off[12][1]
    assert info["pipeline"] == "three-launch" and info["persist_gave_up"] == 0 and info["persist_launches"] == 0, info
    assert info["iter"] == 12 and info["working_rows"] == 6000
    assert_same(off, on, f"{pc.kernel_name(kernel, 2)} overflow")


@pytest.mark.parametrize("kernel,row_free", [(4, False), (3, False), (2, False), (3, True)])
def test_two_rounds_through_the_solver_step(monkeypatch, kernel, row_free):
    """One SCP step (scp_solver_step) of a grid swap of 33 agents with a working-set margin of 0.05: constraint generation
    adds rows in a second round to the live QP (the oracle: 2 rounds, 115 steps, 104 rows; the circle scenario of 33 agents
    runs into the iteration limit in round 1 instead).  (row_free: the rows come through the small install, whose lists the
    kernel loads either way; otherwise they are appended and the kernel builds its own tables.)"""
    from path_planning.solvers.scp import SCP

    sc = pc.Scenario("grid", 1, 33, 50, 2)
    prob = pc.make_problem(sc)
    space = list(prob.pos_min) + list(prob.pos_max)
    res = {}
    for hook in (0, 1):
        monkeypatch.setenv("SCP_PERSIST_HOST_LISTS", str(hook))
        solver = SCP(sc.N, sc.T, pc.H, pc.R, space, dim=2, device=0, verbose=False, working_set_margin=0.05,
                     row_free=row_free, reuse_native=False, qp_settings={"persistent": kernel})
        try:
            solver.set_initial_states(prob.p0)
            solver.set_final_states(prob.pf)
            solver._precompute_constraint_matrices()
            acc0 = solver._solve_initial_trajectory()
            new, info = solver.scp_iteration(acc0)
            res[hook] = (new.cpu().numpy(), {k: info[k] for k in ("iter", "working_rows", "rounds", "added", "pipeline",
                                                                   "status_val", "rho", "rel_step", "persist_gave_up")})
        finally:
            solver.close()
    assert res[0][1]["rounds"] >= 2 and pc.PIPELINE[kernel] in res[0][1]["pipeline"].split("+"), res[0][1]
    assert res[0][1] == res[1][1], (res[0][1], res[1][1])
    assert np.array_equal(res[0][0], res[1][0])
