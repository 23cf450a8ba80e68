"""Every ADMM pipeline beyond the persistent kernels, step by step, against the QP oracle (cases: tests/pipeline_cases.py),
and the per-rho KKT blocks behind all of them.

For every case and every m of its steps, a solve with max_iter = m (fixed rho, check_termination = 6, eps = 1e-12) must report
exactly the case's pipeline in info["pipeline"], info["iter"] == m (generic cases: cg_iters_total == cg_iters * m) and leave x
and z / y of the fixed and the working collision rows within tolerance of the oracle's state after m steps, entry by entry.

The carried F x and S0 x ("fx", "qx") are compared on the single-step pipelines only (three-launch and three-launch-bigK:
groups A and B up to K = 1024).  scp_qp_cg1_iteration updates d.fx and the other half of HQ in every step (qp_on_cg1_step
swaps qx_half, scp_qp_qx names the half that holds S0 x); the generic check at the end of a bigK solve leaves both alone or
exact (it forms F x in tf and S0 x in rows [K, 2K) of HQ).  The generic pipeline never writes d.fx and uses HQ as scratch
(qp_on_scratch_used), and QP#0 keeps neither between launches: there the two names hold nothing that is part of the state.

Tolerance: pc.tolerances (1e-11 * max(1, |oracle|_max) per array, the rho-scaled allowance for the duals) with the floor
100 d_m, d_m = the largest difference in x between the numpy and the C oracle after the same m steps with the same settings
(the reference's own sensitivity to the order of summation; pipeline_cases.d_m).  Nothing is fitted to the GPU's result.

KKT blocks (peek "Hf", "Minv", "T"): H_f against FixedOps.kkt_matrix at 1e-13 |H_f|_max; the Gauss-Jordan inverse by its
residual || H_f Minv - I ||_max (product in np.longdouble), at most 16 x the residual of np.linalg.inv(H_f); T against
S0 Minv at 1e-12 max(1, |T|_max); and the per-rho cache across an eviction and a hit, bit for bit against a fresh object.
"""
import numpy as np
import pytest

import persist_cases as pc
import pipeline_cases as qc
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
STATE = ("x", "zf", "yf", "zc", "yc")
CARRIED = ("fx", "qx")
RATIOS = {}      # (pipeline, K, m) -> largest error / tolerance seen
INV_RATIOS = {}  # (K, rho) -> residual of the GPU's inverse / residual of numpy's


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
    """reset(x0) (None: zeros) and the working rows"""
    import torch

    qp.reset(None if x0 is None else ctx.tensor(x0))
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size:
        qp.add_rows(torch.as_tensor(rows, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[rows]), ctx.tensor(l_col[rows]))


def peek_state(qp, names=STATE):
    return {n: qp.peek(n).cpu().numpy() for n in names}


def compare_state(qp, prob, snap, gpu_rows, names, floor, what):
    """every peeked array against the oracle snapshot, entry by entry within pc.tolerances (floor: 100 d_m); the message names
    the case, m, the array and the worst index; returns the largest error / tolerance"""
    order = np.searchsorted(snap["rows"], gpu_rows)
    assert np.array_equal(snap["rows"][order], gpu_rows), what
    ref = pc.reference_arrays(prob, snap, order)
    tols = pc.tolerances(prob, ref, snap["rho"], floor=floor)
    worst = 0.0
    for name in names:
        got = qp.peek(name).cpu().numpy()
        r, tol = ref[name], tols[name]
        assert got.shape == r.shape, (what, name, got.shape, r.shape)
        if not got.size:
            continue
        q = np.abs(got - r) / tol
        i = int(np.argmax(q))
        worst = max(worst, float(q[i]))
        assert q[i] <= 1.0, (f"{what}: array {name}: |gpu - oracle| = {abs(got[i] - r[i]):.3e} > {tol[i]:.3e} at "
                             f"{pc.where(prob, name, i, gpu_rows)} (gpu {got[i]!r}, oracle {r[i]!r})")
    return worst


# ---- the state after m steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c.id)
def test_state_after_m_steps(ctx, case):
    prob, x0, eta, l_col, dist, W = qc.problem(case)
    snaps, _ = qc.snapshots(case)
    names = STATE + (CARRIED if case.carries else ())
    qp = new_qp(ctx, prob, **case.gpu_settings(1))
    try:
        for m in case.steps:
            qp.update_settings(max_iter=m)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            what = f"{case.pipeline} ({case.id}: {case.edge}) m={m}"
            assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
            assert info["iter"] == m and info["status_val"] == -2 and info["working_rows"] == W.size, (what, info)
            if case.group == "C":
                assert info["cg_iters_total"] == case.cg_iters * m, (what, info)
            d = qc.d_m(case, m)
            worst = compare_state(qp, prob, snaps[m], W, names, 100.0 * d, what)
            key = (case.pipeline, case.scen.K, m)
            RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
            print(f"pipeline-step {case.id} m={m} d_m={d:.2e} max err/tol = {worst:.3g}")
    finally:
        qp.close()


# ---- the KKT blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", qc.KKT_K)
def test_kkt_blocks(ctx, K):
    """H_f, its inverse and T = S0 H_f^-1 at every rho of KKT_RHO, each set with set_rho after reset (K <= 96: the inverse in
    LDS; beyond: two launches per pivot).  The inverse may leave up to 16 x the residual of np.linalg.inv on the same H_f;
    numpy's own residual is below 1e-8 at every (K, rho) of the table (at most 1.7e-11, K = 250, rho = 16), so none is
    dropped.  Measured on an MI355X: ratio GPU / numpy between 0.48 and 1.68 over the 28 pairs, the largest at K = 3, rho = 16
    (residuals of 1e-16 there); 1.62 at K = 96, 1.39 at K = 97, 1.58 at K = 250."""
    prob = pc.make_problem(pc.Scenario("near", 1, 2, K, 2))
    qp = new_qp(ctx, prob)
    try:
        qp.reset(None)
        for rho in qc.KKT_RHO:
            qp.set_rho(rho)
            Hf, Minv, T = (qp.peek(n).cpu().numpy().reshape(K, K) for n in ("Hf", "Minv", "T"))
            Href, S0 = qc.kkt_reference(K, rho)
            what = f"K={K} rho={rho}"
            err = float(np.abs(Hf - Href).max())
            assert err <= 1e-13 * np.abs(Href).max(), (what, "Hf", err, float(np.abs(Href).max()))
            ref_res = qc.inverse_residual(Hf, np.linalg.inv(Hf))
            assert ref_res < 1e-8, (what, "numpy's own inverse", ref_res)
            res = qc.inverse_residual(Hf, Minv)
            INV_RATIOS[K, rho] = res / ref_res
            print(f"kkt-inverse K={K} rho={rho:g} residual gpu {res:.3e} numpy {ref_res:.3e} ratio {res / ref_res:.3g}")
            assert res <= qc.INV_RATIO_MAX * ref_res, (what, "Minv", res, ref_res)
            Tref = np.asarray(S0.astype(np.longdouble) @ Minv.astype(np.longdouble), dtype=np.float64)
            terr = float(np.abs(T - Tref).max())
            assert terr <= 1e-12 * max(1.0, np.abs(Tref).max()), (what, "T", terr, float(np.abs(Tref).max()))
    finally:
        qp.close()


def lru(sequence, slots=32):
    """hit (True) / miss (False) of every request of the per-rho cache (scp_qp_build_kkt: least recently used is evicted)"""
    held, out = [], []
    for v in sequence:
        out.append(v in held)
        if v in held:
            held.remove(v)
        elif len(held) == slots:
            held.pop(0)
        held.append(v)
    return out


@pytest.mark.parametrize("back_to,hit", [(0, False), (32, True)], ids=["evicted-first", "hit-last-but-one"])
@pytest.mark.parametrize("K", sorted(qc.EVICT_SCEN))
def test_kkt_cache_eviction_and_hit(ctx, K, back_to, hit):
    """set_rho through 34 distinct grid values (more than SCP_KKT_SLOTS_MAX = 32; K = 50 and 97 both get 32 slots), then back to
    the first one (evicted, rebuilt) or the last but one (still cached), and two steps: x, z, y bit-identical to a fresh object
    taken straight to that rho, and within tolerance of the oracle at that rho."""
    sc = qc.EVICT_SCEN[K]
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    rho, m = qc.EVICT_RHOS[back_to], 2
    # reset builds settings.rho = 0.1 = EVICT_RHOS[0]; then the 34 values, then the return
    assert lru((0.1,) + qc.EVICT_RHOS + (rho,))[-1] == hit and lru((0.1, rho)) == [False, rho == 0.1]
    states = []
    for tour in (qc.EVICT_RHOS, ()):
        qp = new_qp(ctx, prob, **pc.gpu_step_settings(0, m))
        try:
            load(ctx, qp, x0, W, eta, l_col)
            for r in tour:
                qp.set_rho(r)
            qp.set_rho(rho)
            info = qp.solve()
            assert info["pipeline"] == "three-launch" and info["iter"] == m and info["rho"] == rho, info
            states.append(peek_state(qp))
            if tour:
                snaps, _ = pc.oracle_snapshots(sc, (m,), rho=rho, margin=sc.margin)
                xc, _ = co.admm(prob, eta, l_col, dist, x0=x0, st=pc.step_settings(m, rho=rho, margin=sc.margin))
                d = float(np.abs(xc - snaps[m]["x"]).max())
                assert snaps[m]["rho"] == rho
                worst = compare_state(qp, prob, snaps[m], W, STATE, 100.0 * d, f"K={K} after the tour, rho={rho}")
                key = ("kkt-cache " + ("hit" if hit else "rebuilt"), K, m)
                RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
        finally:
            qp.close()
    for name in STATE:
        assert np.array_equal(states[0][name], states[1][name]), (K, rho, name)


def test_report_margins(record_property):
    """largest error / tolerance per (pipeline, K, m) and the inverse's residual ratio per (K, rho) over the tests above
    (pytest -rA or --junitxml shows them)"""
    for (pipe, K, m), r in sorted(RATIOS.items()):
        record_property(f"{pipe} K={K} m={m}", f"{r:.3g}")
        print(f"pipeline-margin {pipe:20s} K={K:5d} m={m:3d} max err/tol = {r:.3g}")
    for (K, rho), r in sorted(INV_RATIOS.items()):
        record_property(f"inverse K={K} rho={rho:g}", f"{r:.3g}")
        print(f"inverse-ratio   K={K:5d} rho={rho:<9g} gpu residual / numpy residual = {r:.3g}")
