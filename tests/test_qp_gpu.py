"""GPU parity of the joint QP (a3/a6/a9) through the C-ABI against oracle/qp_oracle.py.

The QP boundary of the reference is OSQP ("parity unpinned", see oracle/qp_oracle.py): the HIP solver is
compared (i) with the oracle's line-by-line statement of the same algorithm (admm_structured) at 1e-9 and
(ii) with the independent explicit-matrix OSQP restatement run to 1e-9 accuracy, i.e. the unique minimiser."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import qp_oracle as qo
from oracle import scp_oracle as so

pytestmark = pytest.mark.gpu
LIMITS = [-2.0, 2.0, -15.0, 15.0, -20.0, 20.0]


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def ref_problem(n, seed, T=10.0, h=0.2, R=0.8):
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(n, R, seed=seed)
    return so.make_problem(n, T, h, R, [0, 0, 20, 20], p0, pf)


def make_qp(ctx, prob, **kw):
    from path_planning import _hip

    kw.setdefault("cg_iters", 3)
    st = _hip.default_settings(**kw)
    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, st)
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    return qp


def oracle_settings(**kw):
    base = dict(cg_iters=3)
    base.update(kw)
    return qo.Settings(**base)


@pytest.mark.parametrize("use_mfma", [1, 0])
@pytest.mark.parametrize("n,seed,T,h", [(4, 1, 10.0, 0.5), (20, 20, 10.0, 0.2)])
def test_qp0_matches_oracle(ctx, n, seed, T, h, use_mfma):
    prob = ref_problem(n, seed, T, h)
    for eps in (1e-3, 1e-8):
        qp = make_qp(ctx, prob, eps_abs=eps, eps_rel=eps, use_mfma=use_mfma)
        qp.reset(None)
        info = qp.solve()
        x = qp.solution().cpu().numpy()
        xo, yo, io = qo.admm_structured(prob, st=oracle_settings(eps_abs=eps, eps_rel=eps))
        assert info["status_val"] == 1 and io["status_val"] == 1
        assert info["iter"] == io["iter"] and info["rho_updates"] == io["rho_updates"]
        np.testing.assert_allclose(x, xo, rtol=0, atol=1e-9)
        assert abs(info["rho"] - io["rho"]) <= 1e-5 * io["rho"]  # rho is a ratio of 1e-9-size residuals
        # duals in the reference stacking order
        yf, _ = qp.duals()
        yo_flat = np.hstack([yo[k].ravel() for k in ("jerk", "acc", "vel", "pos")])
        np.testing.assert_allclose(yf.cpu().numpy(), yo_flat, rtol=0, atol=1e-8)
        qp.close()
    # exact minimiser: explicit-matrix OSQP restatement at 1e-9
    C, l, u = so.stack_fixed(prob)
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), C, l, u, eps_abs=1e-9, eps_rel=1e-9,
                         max_iter=20000)
    assert r["status_val"] == 1
    np.testing.assert_allclose(x.ravel(), r["x"], rtol=0, atol=1e-7)


@pytest.mark.parametrize("cg,use_mfma", [(1, 1), (2, 1), (3, 2), (3, 0)])
def test_collision_qp_paths_and_pcg_steps(ctx, cg, use_mfma):
    """One PCG step per ADMM step on the default single-step pipeline, 2 and 3 on the generic pipeline (MFMA products with
    use_mfma 1 and 2, VALU with 0): all follow the oracle iterate for iterate."""
    import torch

    prob = ref_problem(10, 7, 10.0, 0.2)
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-8, eps_rel=1e-8))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    st = oracle_settings(max_iter=10000, max_rounds=1, cg_iters=cg)
    xo, yo, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W)
    qp = make_qp(ctx, prob, max_iter=10000, cg_iters=cg, use_mfma=use_mfma)
    qp.reset(ctx.tensor(x0))
    qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
    info = qp.solve()
    assert info["status_val"] == io["status_val"] == 1 and info["iter"] == io["iter"]
    assert info["cg_iters_total"] == cg * info["iter"]
    if cg > 1:
        assert info["pipeline"] == "generic", info["pipeline"]
    np.testing.assert_allclose(qp.solution().cpu().numpy(), xo, rtol=0, atol=1e-8)
    qp.close()


@pytest.mark.parametrize("cg,use_mfma", [(1, 1), (2, 1), (3, 2), (3, 0)])
def test_every_qp_path_is_deterministic(ctx, cg, use_mfma):
    """No atomics on floating-point data anywhere in the iteration: A_W^T g is a gather over sorted incidence lists on every
    path (single-step, generic MFMA / VALU), so two solves of the same QP agree bit for bit -- primal and duals.
    (Round 1 scattered with atomics on the cg_iters >= 2 and generic paths.)"""
    import torch

    prob = ref_problem(24, 5, 10.0, 0.2)
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-6, eps_rel=1e-6))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    assert len(W) > 100
    runs = []
    for _ in range(2):
        qp = make_qp(ctx, prob, max_iter=10000, cg_iters=cg, use_mfma=use_mfma)
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        info = qp.solve()
        yf, yc = qp.duals()
        runs.append((info["iter"], qp.solution().cpu().numpy(), yf.cpu().numpy(), yc.cpu().numpy()))
        qp.close()
    assert runs[0][0] == runs[1][0] and runs[0][0] >= 25
    for a, b in zip(runs[0][1:], runs[1][1:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("persistent", [4, 2, 3])
def test_in_kernel_rho_switch_equals_host_path(ctx, persistent):
    """Adaptive rho: the first solve of a QP object finds no cached blocks for the new rho values, so the persistent kernel
    returns and the host builds them (build_kkt + rows_value_kernel); a second solve of the SAME problem on the same object
    finds them cached and the kernel switches by itself (operands reloaded, row values recomputed in LDS).  Same
    iterates bit for bit, same number of rho updates, and the oracle's count."""
    import torch

    prob = ref_problem(18, 1, 10.0, 0.2)  # two rho updates in 250 ADMM steps
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-6, eps_rel=1e-6))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    st = oracle_settings(max_iter=10000, max_rounds=1, cg_iters=1, eps_abs=1e-5, eps_rel=1e-5)
    _, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W)
    assert io["rho_updates"] == 2 and io["status_val"] == 1
    qp = make_qp(ctx, prob, max_iter=10000, cg_iters=1, eps_abs=1e-5, eps_rel=1e-5, persistent=persistent)
    runs = []
    for _ in range(3):
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        info = qp.solve()
        yf, yc = qp.duals()
        assert {4: "persistent", 2: "persistent16", 3: "persistent8-lean"}[persistent] in info["pipeline"].split("+")
        runs.append((info["iter"], info["rho_updates"], info["status_val"], qp.solution().cpu().numpy(), yf.cpu().numpy(),
                     yc.cpu().numpy(), info["rho_switches_in_kernel"]))
    qp.close()
    assert runs[0][:3] == runs[1][:3] == runs[2][:3] == (io["iter"], io["rho_updates"], 1)
    assert runs[0][6] == 0 and runs[1][6] == runs[2][6] == io["rho_updates"]  # host path first, then inside the kernel
    for r in runs[1:]:
        for a, b in zip(runs[0][3:6], r[3:6]):
            # (the lean kernels keep v = z~ + y / rho per row: their in-kernel switch repeats the arithmetic of leaving with
            # z, y and re-entering with the new rho, so both paths give the same bits there too)
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("n,seed,T,h,margin", [(4, 1, 10.0, 0.5, 0.5), (10, 7, 10.0, 0.2, 0.5), (4, 1, 10.0, 0.5, 1e9)])
def test_collision_qp_matches_oracle(ctx, n, seed, T, h, margin):
    """First SCP iteration's joint QP, working set fixed by `margin` (1e9 = every collision row)."""
    from path_planning import _hip

    prob = ref_problem(n, seed, T, h)
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-8, eps_rel=1e-8))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < margin)[0]
    for eps, max_iter in ((1e-3, 10000), (1e-6, 20000)):
        st = oracle_settings(eps_abs=eps, eps_rel=eps, max_iter=max_iter, max_rounds=1)
        xo, yo, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W)
        qp = make_qp(ctx, prob, eps_abs=eps, eps_rel=eps, max_iter=max_iter)
        qp.reset(ctx.tensor(x0))
        import torch

        rows = torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev)
        qp.add_rows(rows, ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        info = qp.solve()
        x = qp.solution().cpu().numpy()
        assert info["status_val"] == io["status_val"] == 1
        assert info["iter"] == io["iter"], (info, io)
        assert info["working_rows"] == W.size
        np.testing.assert_allclose(x, xo, rtol=0, atol=1e-8)
        _, yc = qp.duals()
        np.testing.assert_allclose(yc.cpu().numpy(), yo["col"], rtol=0, atol=1e-7)
        qp.close()
    # against the exact minimiser of the same (working-set) QP, explicit matrices
    C, lf, uf = so.stack_fixed(prob)
    A = sp.vstack([C, so.collision_matrix_explicit(prob, eta)[W]], format="csc")
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), A, np.hstack([lf, l_col[W]]),
                         np.hstack([uf, np.full(W.size, np.inf)]), x0=x0.ravel(), eps_abs=1e-9, eps_rel=1e-9,
                         max_iter=100000)
    assert r["status_val"] == 1
    assert np.abs(x.ravel() - r["x"]).max() < 5e-4  # eps = 1e-6 ADMM point vs the exact minimiser


def test_primal_infeasibility_certificate(ctx):
    """OSQP's delta-y certificate: (i) an unreachable goal makes QP#0 infeasible; (ii) the FIRST linearised QP of the
    reference's own __main__ demo (3 vehicles crossing in T = 3 s, scp.py:844-862) is primal infeasible -- the
    explicit-matrix OSQP restatement says so too.  GPU, numpy oracle and C oracle stop at the same iteration."""
    import torch

    from oracle import c_oracle as co

    far = so.make_problem(2, 1.0, 0.2, 0.5, [0, 0, 20, 20], np.array([[1.0, 1.0], [3.0, 3.0]]),
                          np.array([[19.0, 19.0], [15.0, 3.0]]))
    qp = make_qp(ctx, far, cg_iters=1)
    qp.reset(None)
    info = qp.solve()
    _, _, io = qo.admm_structured(far, st=qo.Settings(max_iter=4000))
    assert info["status_val"] == io["status_val"] == -3 and info["status"] == "primal infeasible"
    assert info["iter"] == io["iter"] == co.admm(far, st=qo.Settings(max_iter=4000))[1]["iter"]
    qp.close()

    p0 = np.array([[-2.0, -2.0], [0.0, -2.0], [2.0, -2.0]])
    pf = np.array([[2.0, 2.0], [0.0, 2.0], [-2.0, 2.0]])
    prob = so.make_problem(3, 3.0, 0.2, 0.5, [-5, -5, 500, 200], p0, pf)
    x0, _, i0 = qo.admm_structured(prob, st=qo.Settings(max_iter=4000))
    assert i0["status_val"] == 1
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    st = qo.Settings(max_iter=10000)
    _, _, io = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st)
    W = np.nonzero(dist - prob.R < st.margin)[0]
    qp = make_qp(ctx, prob, cg_iters=1, max_iter=10000)
    qp.reset(ctx.tensor(x0))
    qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
    info = qp.solve()
    assert info["status_val"] == io["status_val"] == -3 and info["iter"] == io["iter"]
    C, lf, uf = so.stack_fixed(prob)
    A = sp.vstack([C, so.collision_matrix_explicit(prob, eta)], format="csc")
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), A, np.hstack([lf, l_col]),
                         np.hstack([uf, np.full(l_col.size, np.inf)]), x0=x0.ravel(), max_iter=10000)
    assert r["status_val"] == -3
    qp.close()


def test_qp_3d_z0_metamorphic(ctx):
    """D=3 with z == 0 everywhere reproduces the D=2 solution."""
    prob2 = ref_problem(6, 3, 10.0, 0.5)
    z = np.zeros((prob2.N, 1))
    prob3 = so.make_problem(prob2.N, 10.0, 0.5, prob2.R, [0, 0, -5, 20, 20, 5], np.hstack([prob2.p0, z]),
                            np.hstack([prob2.pf, z]))
    xs = []
    for prob in (prob2, prob3):
        qp = make_qp(ctx, prob, eps_abs=1e-8, eps_rel=1e-8)
        qp.reset(None)
        assert qp.solve()["status_val"] == 1
        xs.append(qp.solution().cpu().numpy())
        qp.close()
    np.testing.assert_allclose(xs[1][:, :, :2], xs[0], rtol=0, atol=1e-10)
    assert np.abs(xs[1][:, :, 2]).max() < 1e-12


def test_qp_errors(ctx):
    from path_planning import _hip

    prob = ref_problem(4, 1, 10.0, 0.5)
    st = _hip.default_settings()
    qp = _hip.QP(ctx, prob.N, prob.K, 2, prob.h, st, row_capacity=4)
    with pytest.raises(_hip.HipError):  # reset before set_problem
        qp.reset(None)
    space = np.concatenate([prob.pos_min, prob.pos_max])
    qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
    qp.reset(None)
    import torch

    rows = torch.arange(5, dtype=torch.int64, device=ctx.tdev)
    with pytest.raises(_hip.HipError) as e:  # capacity
        qp.add_rows(rows, ctx.tensor(np.ones((5, 2))), ctx.tensor(np.zeros(5)))
    assert e.value.code == _hip.SCP_ERR_CAPACITY
    with pytest.raises(_hip.HipError):
        _hip.QP(ctx, 4, 20, 4, 0.5)  # D = 4
    qp.close()


@pytest.mark.parametrize("n,seed,dim", [(10, 7, 2), (24, 5, 2), (7, 3, 3)])
def test_persistent_kernel_equals_three_launch_pipeline(ctx, n, seed, dim):
    """settings.persistent: the persistent single-step kernel (state on chip, tagged-granule exchanges) and the
    three-launch pipeline run the same arithmetic -- after 12 ADMM steps (two launches of the persistent kernel with a
    termination check in between) every piece of solver state agrees to rounding, and both agree with the oracle.
    (Only the summation order of the line-search partials differs; over hundreds of steps the single-step ADMM map can
    amplify that 1e-16 -- see test_scp_sweep_vs_oracle -- so the comparison is made early.)"""
    import torch
    from path_planning.scenarios.position_generator import generate_grid_swap

    if dim == 2 and n == 10:
        prob = ref_problem(n, seed)
    else:
        p0, pf, space = generate_grid_swap(n, seed=seed, dim=dim)
        prob = so.make_problem(n, 10.0, 0.2, 0.8, space, p0, pf)
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-8, eps_rel=1e-8))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    assert W.size > 0
    space = np.concatenate([prob.pos_min, prob.pos_max])
    states = {}
    for persistent in (4, 0, 3) + ((2,) if dim == 2 else ()):  # 4: the round-2 kernel, 2: the lean 16-agent kernel (2-D), 3: its 8-agent form
        from path_planning import _hip

        st = _hip.default_settings(cg_iters=1, persistent=persistent, max_iter=12, check_termination=6, adaptive_rho=0,
                                   eps_abs=1e-12, eps_rel=1e-12)
        qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, st)
        qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        info = qp.solve()
        assert info["iter"] == 12 and info["status_val"] == -2
        assert info["pipeline"] == {4: "persistent", 0: "three-launch", 2: "persistent16",
                                    3: "persistent8-lean"}[persistent]
        states[persistent] = {k: qp.peek(k).cpu().numpy() for k in ("x", "zf", "yf", "fx", "qx", "zc", "yc", "gval")}
        states[persistent]["sol"] = qp.solution().cpu().numpy()
        qp.close()
    for which in states:
        if which == 0:
            continue
        for k in states[which]:
            scale = max(1.0, np.abs(states[0][k]).max())
            np.testing.assert_allclose(states[which][k], states[0][k], rtol=0, atol=1e-11 * scale, err_msg=f"{which}:{k}")
    so_ = oracle_settings(cg_iters=1, max_iter=12, check_termination=6, adaptive_rho=False, eps_abs=1e-12, eps_rel=1e-12,
                          max_rounds=1)
    xo, _, _ = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=so_, rows0=W)
    np.testing.assert_allclose(states[4]["sol"], xo, rtol=0, atol=1e-8)
    np.testing.assert_allclose(states[3]["sol"], xo, rtol=0, atol=1e-8)


def test_status_solved_inaccurate(ctx):
    """OSQP returns "solved inaccurate" (2) when max_iter is reached with the 10 x looser tolerances met; the reference
    accepts it like "solved" (scp.py:363, :446).  GPU, numpy oracle and C oracle agree on where that happens."""
    from oracle import c_oracle as co

    prob = ref_problem(10, 7)
    full = qo.admm_structured(prob, st=oracle_settings(cg_iters=1))[2]
    assert full["status_val"] == 1 and full["iter"] > 50
    hit = None
    for cap in range(25, full["iter"], 25):  # first cap at which the loose test holds but the tight one does not yet
        st = oracle_settings(cg_iters=1, max_iter=cap)
        xo, _, io = qo.admm_structured(prob, st=st)
        qp = make_qp(ctx, prob, cg_iters=1, max_iter=cap)
        qp.reset(None)
        info = qp.solve()
        x = qp.solution().cpu().numpy()
        qp.close()
        _, ic = co.admm(prob, st=st)
        assert info["status_val"] == io["status_val"] == ic["status_val"], (cap, info, io, ic)
        assert info["status"] == qo.STATUS_TEXT[io["status_val"]]
        np.testing.assert_allclose(x, xo, rtol=0, atol=1e-9)
        if io["status_val"] == 2:
            hit = cap
            break
    assert hit is not None, "no iteration cap produced status 2"


@pytest.mark.parametrize("persistent", [4, 2, 3])
def test_persistent_kernel_give_up_falls_back(ctx, persistent):
    """A persistent launch whose workgroups cannot all make progress (here: it is told to wait for a workgroup that does
    not exist) must time out in its bounded spins, leave WITHOUT writing state back, and the solve must carry on from the
    same state on the three-launch pipeline: same result as a solve that never used the persistent kernel."""
    import torch
    from path_planning import _hip

    prob = ref_problem(10, 7)
    x0, _, _ = qo.admm_structured(prob, st=oracle_settings(eps_abs=1e-8, eps_rel=1e-8))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < 0.5)[0]
    space = np.concatenate([prob.pos_min, prob.pos_max])
    out = {}
    for mode in ("fault", "three_launch"):
        st = _hip.default_settings(cg_iters=1, persistent=persistent if mode == "fault" else 0, max_iter=10000)
        qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, st)
        qp.set_problem(LIMITS, space, ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf), ctx.tensor(prob.vf))
        qp.reset(ctx.tensor(x0))
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
        if mode == "fault":
            assert qp.debug_set("persist_fault", 1) == 1 and qp.debug_set("persist_off", -1) == 0
        info = qp.solve()
        if mode == "fault":
            assert qp.debug_set("persist_off", -1) == 1 and qp.debug_set("persist_fault", -1) == 0
            # the fallback is visible in the result, not only in the time (scp_qp_info)
            assert info["persist_gave_up"] == 1 and info["persist_launches"] == 0 and info["pipeline"] == "three-launch"
            assert qp.debug_set("persist_gave_up_total", -1) == 1
        else:
            assert info["persist_gave_up"] == 0 and info["pipeline"] == "three-launch"
        out[mode] = (info, qp.solution().cpu().numpy())
        if mode == "fault":
            # a give-up belongs to the moment, not to the object: the next QP of the same object is back on the persistent
            # kernel (scp_qp_reset re-arms it) and says so
            qp.reset(ctx.tensor(x0))
            qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
            assert qp.debug_set("persist_off", -1) == 0
            again = qp.solve()
            assert again["pipeline"] == {4: "persistent", 2: "persistent16", 3: "persistent8-lean"}[persistent]
            assert again["persist_launches"] >= 1 and again["persist_gave_up"] == 0
            assert again["status_val"] == 1 and again["rho_switches_in_kernel"] <= again["rho_updates"]
            assert qp.debug_set("persist_gave_up_total", -1) == 1
        qp.close()
    assert out["fault"][0]["status_val"] == out["three_launch"][0]["status_val"] == 1
    assert out["fault"][0]["iter"] == out["three_launch"][0]["iter"]
    if persistent == 4:
        np.testing.assert_array_equal(out["fault"][1], out["three_launch"][1])
    else:
        # at a give-up the host rebuilds the carried F x / S0 x slabs exactly from x (it cannot know whether a workgroup wrote
        # anything back); rounding-level room for that
        np.testing.assert_allclose(out["fault"][1], out["three_launch"][1], rtol=0, atol=1e-12)
