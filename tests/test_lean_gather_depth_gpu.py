"""The lean persistent ADMM kernels on working sets whose cells hold 0, 1, U, U + 1 and >= 2 U + 1 rows for U = 2, 3, 4 (the
table and what it claims: tests/test_lean_gather_depth_cpu.py): the state after m = 1, 2 and 7 steps against the oracle's
snapshots, under pc.tolerances as tests/test_persist_iterates_gpu.py applies them."""
import numpy as np
import pytest

import persist_cases as pc
import test_lean_gather_depth_cpu as table

pytestmark = pytest.mark.gpu
PEEK = ("x", "zf", "yf", "zc", "yc", "fx", "qx")


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", table.CASES, ids=lambda c: c.id)
def test_state_after_m_steps(ctx, case):
    import torch
    from path_planning import _hip

    sc = case.scen
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    snaps, _ = pc.oracle_snapshots(sc, case.steps)
    name = pc.kernel_name(case.kernel, sc.dim)
    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**pc.gpu_step_settings(case.kernel, 1)))
    try:
        qp.set_problem(pc.LIMITS, np.concatenate([prob.pos_min, prob.pos_max]), ctx.tensor(prob.p0), ctx.tensor(prob.v0),
                       ctx.tensor(prob.pf), ctx.tensor(prob.vf))
        for m in case.steps:
            qp.update_settings(max_iter=m)
            qp.reset(ctx.tensor(x0))
            qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
            info = qp.solve()
            what = f"{name} ({case.id}) m={m}"
            assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
            assert info["iter"] == m and info["status_val"] == -2 and info["persist_gave_up"] == 0, (what, info)
            snap = snaps[m]
            order = np.searchsorted(snap["rows"], W)
            assert np.array_equal(snap["rows"][order], W), what
            ref = pc.reference_arrays(prob, snap, order)
            tols = pc.tolerances(prob, ref, snap["rho"])
            for arr in PEEK:
                got = qp.peek(arr).cpu().numpy()
                assert got.shape == ref[arr].shape, (what, arr, got.shape, ref[arr].shape)
                q = np.abs(got - ref[arr]) / tols[arr]
                i = int(np.argmax(q))
                print(f"lean-gather-margin {what} {arr}: max err/tol = {q[i]:.3g}")
                assert q[i] <= 1.0, (f"{what}: array {arr}: |gpu - oracle| = {abs(got[i] - ref[arr][i]):.3e} > {tols[arr][i]:.3e} "
                                     f"at {pc.where(prob, arr, i, W)} (gpu {got[i]!r}, oracle {ref[arr][i]!r})")
    finally:
        qp.close()
