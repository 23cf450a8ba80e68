"""Joint QPs with per-state position boxes, step by step, against the boxed QP oracle (cases: tests/box_cases.py), on every
pipeline a boxed QP can take: the round-2 persistent kernel (whatever settings.persistent in 1 .. 4 asks for), the three-launch
pipeline, its K > 120 form, the generic pipeline and QP#0.

For every case and every m of its steps, a solve with max_iter = m (fixed rho, check_termination = 6, eps = 1e-12) after
set_problem + set_position_boxes must report exactly the case's pipeline in info["pipeline"], info["iter"] == m and leave x and
z / y of the fixed and the working collision rows (on the pipelines that carry them also F x and S0 x) within tolerance of the
oracle's state after m steps, entry by entry.  After the solves "lf" / "uf" are still the oracle's bounds bit for bit.  At
m = 1 the boxed x equals the box-free one (z starts as A x unclamped, y = 0): there the boxes show in z and y only.

Tolerance: pc.tolerances with the floor 100 d_box(m) (box_cases.d_box: the boxed numpy oracle against its own rerun from a
start perturbed by one ulp; calibrated against pipeline_cases.d_m in tests/test_box_cases_cpu.py).  Nothing is fitted to the
GPU's result.

Sensitivity, one control per group: the same solve with the last agent's box left out ON THE GPU SIDE ONLY, pushed through the
comparison with the assert turned into a return value (box_cases.worst_ratio), comes out above 1.0 at every m.

Measured on an MI355X, largest error / tolerance: persistent 0.35 (K = 50, m = 12), three-launch 0.35 (K = 50, m = 12), bigK 0.48
(K = 250, m = 12), qp0 0.21 (K = 120, m = 1), generic 0.96 (QP#0 at K = 121 from the random start, m = 12: an error of 7e-11
against d_box = 7.6e-13; 0.49 at its other steps, at most 0.05 with rows); the controls 1.5e9 .. 5.8e10 (test_report_margins
lists all of them).
"""
import numpy as np
import pytest

import box_cases as bc
from test_pipeline_iterates_gpu import compare_state, load, new_qp

pytestmark = pytest.mark.gpu
RATIOS = {}   # (pipeline, K, m) -> largest error / tolerance seen
CONTROLS = {}  # (group, m) -> error / tolerance of the solve without the last agent's box


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def boxed_qp(ctx, prob, lo, hi, **st):
    """set_problem, then the boxes"""
    qp = new_qp(ctx, prob, **st)
    qp.set_position_boxes(ctx.tensor(lo), ctx.tensor(hi))
    return qp


def assert_bounds_undisturbed(qp, case, what):
    for name, want in zip(("lf", "uf"), bc.oracle_bounds(case)):
        got = qp.peek(name).cpu().numpy()
        assert got.shape == want.shape, (what, name)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_state_after_m_steps(ctx, case):
    prob, x0, eta, l_col, dist, W = bc.problem(case)
    snaps, _ = bc.snapshots(case)
    lo, hi = bc.case_boxes(case)
    for per in case.persistents:
        qp = boxed_qp(ctx, prob, lo, hi, **case.gpu_settings(1, per))
        try:
            for m in case.steps:
                qp.update_settings(max_iter=m)
                load(ctx, qp, x0, W, eta, l_col)
                info = qp.solve()
                what = f"{case.pipeline} ({case.id}, persistent={per}) m={m}"
                assert info["pipeline"] == case.pipeline, (what, info["pipeline"])
                assert info["iter"] == m and info["status_val"] == -2 and info["working_rows"] == W.size, (what, info)
                if case.group == "C":
                    assert info["cg_iters_total"] == case.cg_iters * m, (what, info)
                d = bc.d_box(case, m)
                worst = compare_state(qp, prob, snaps[m], W, case.names, 100.0 * d, what)
                key = (case.pipeline, case.scen.K, m)
                RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
                print(f"box-step {case.id} persistent={per} m={m} d_box={d:.2e} max err/tol = {worst:.3g}")
            assert_bounds_undisturbed(qp, case, f"{case.id}, persistent={per}")
        finally:
            qp.close()


CONTROL = [next(c for c in bc.CASES if c.group == g) for g in bc.GROUPS]


@pytest.mark.parametrize("case", CONTROL, ids=lambda c: c.id)
def test_a_dropped_box_shows(ctx, case):
    """the GPU never hears of the last agent's box; the oracle keeps it"""
    prob, x0, eta, l_col, dist, W = bc.problem(case)
    snaps, _ = bc.snapshots(case)
    lo, hi = bc.drop_agent(*bc.case_boxes(case), prob.N - 1)
    qp = boxed_qp(ctx, prob, lo, hi, **case.gpu_settings(1))
    try:
        for m in case.steps:
            qp.update_settings(max_iter=m)
            load(ctx, qp, x0, W, eta, l_col)
            info = qp.solve()
            assert info["pipeline"] == case.pipeline and info["iter"] == m, (case.id, m, info)
            got = {n: qp.peek(n).cpu().numpy() for n in case.names}
            r = bc.worst_ratio(prob, snaps[m], got, W, case.names, 100.0 * bc.d_box(case, m))
            CONTROLS[case.group, m] = r
            print(f"box-control {case.id} m={m}: max err/tol without the last agent's box = {r:.3g}")
            assert r > 1.0, (case.id, m, r)
    finally:
        qp.close()


def test_report_margins(record_property):
    """largest error / tolerance per (pipeline, K, m) over the tests above, and what the controls came out at (pytest -rA or
    --junitxml shows them)"""
    for (pipe, K, m), r in sorted(RATIOS.items()):
        record_property(f"{pipe} K={K} m={m}", f"{r:.3g}")
        print(f"box-margin {pipe:20s} K={K:5d} m={m:3d} max err/tol = {r:.3g}")
    for (group, m), r in sorted(CONTROLS.items()):
        record_property(f"control group {group} m={m}", f"{r:.3g}")
        print(f"box-control-margin group {group} m={m:3d} err/tol = {r:.3g}")
