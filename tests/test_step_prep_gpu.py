"""The large-problem SCP step with "fused_step_prep" on (the default: the prep launch of a multi-launch pairwise pass derives
the positions it stages itself -- from the accelerations at the start of a step, from the QP's time-major solution in every
round -- and the relative-step kernel hands the result out) against the same step with the option off (layout change,
kinematics and prep as separate launches, a copy at the end).  "single_launch_passes" is 0 throughout, so that small shapes
take the large-problem path.  The two are the same arithmetic on the same operands: accelerations, records and rel_step are
compared exactly.

The K = 33 case uses T = 6.7 (int(6.7 / 0.2) = 33; 6.6 / 0.2 rounds below 33 and gives K = 32)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, dim, seed, T)
GRID_CASES = [(2, 2, 1, 10.0), (10, 2, 3, 10.0), (27, 3, 17, 10.0), (64, 2, 64000, 10.0), (10, 2, 3, 6.7)]
_ACC0 = {}


def same_records(a, b):
    keys = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "rounds", "added", "unresolved_rows",
            "status")
    for k in keys:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("r_prim", "r_dual", "rho", "max_violation"):
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


def make(p0, pf, space, T, dim, fused, near=None, row_free=True):
    from path_planning.solvers.scp import SCP

    s = SCP(len(p0), T, 0.2, 0.8, space, dim=dim, verbose=False, row_free=row_free)
    s._ctx.set_option("single_launch_passes", 0)
    s._ctx.set_option("fused_step_prep", fused)
    if near is not None:
        s._ctx.set_near_pass(near)
    s.set_initial_states(np.asarray(p0, dtype=float))
    s.set_final_states(np.asarray(pf, dtype=float))
    return s


def grid(case):
    from path_planning.scenarios.position_generator import generate_grid_swap

    n, dim, seed, T = case
    p0, pf, space = generate_grid_swap(n, seed=seed, dim=dim)
    return p0, pf, space, T, dim


def initial_acc(key, scenario):
    """QP#0's solution for a scenario, computed once and fed to every step that is compared (numpy, (N, K, D))"""
    if key not in _ACC0:
        s = make(*scenario, fused=0)
        s._precompute_constraint_matrices()
        _ACC0[key] = s._solve_initial_trajectory().cpu().numpy().copy()
        s.close()
    return _ACC0[key]


def step(scenario, acc0, fused, near=None, row_free=True, repeats=1):
    s = make(*scenario, fused=fused, near=near, row_free=row_free)
    out = []
    before = s._ctx.near_pass_counts()  # (a context from the pool has a past)
    for _ in range(repeats):
        new, info = s.scp_iteration(acc0)
        out.append((new.cpu().numpy().copy(), info))
    counts = tuple(a - b for a, b in zip(s._ctx.near_pass_counts(), before))
    s.close()
    return out, counts


def assert_same_step(a, b):
    np.testing.assert_array_equal(a[0].view(np.int64), b[0].view(np.int64))
    same_records(a[1], b[1])
    assert a[1]["rel_step"] == b[1]["rel_step"] and a[1]["pipeline"] == b[1]["pipeline"]


@pytest.mark.parametrize("near", [0, 1, 2])
@pytest.mark.parametrize("row_free", [True, False], ids=["row_free", "rows"])
@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: "n%d_d%d_T%g" % (c[0], c[1], c[3]))
def test_single_step(case, row_free, near):
    scenario = grid(case)
    acc0 = initial_acc(case, scenario)
    if case[3] == 6.7:
        assert acc0.shape[1] == 33
    (ref,), ref_counts = step(scenario, acc0, 0, near, row_free)
    (got,), counts = step(scenario, acc0, 1, near, row_free)
    assert_same_step(got, ref)
    assert counts == ref_counts and (counts[0] > 0) == (near != 0)
    assert np.isfinite(got[0]).all() and got[1]["rounds"] >= 1


@pytest.mark.parametrize("case", [(10, 2, 3, 10.0), (27, 3, 17, 10.0)], ids=lambda c: "n%d_d%d" % (c[0], c[1]))
def test_complete_solve(case):
    scenario = grid(case)
    out = []
    for fused in (0, 1):
        s = make(*scenario, fused=fused)
        out.append((s.generate_trajectories(15), s.last_info))
        s.close()
    (ta, ia), (tb, ib) = out
    for key in ("positions", "velocities", "accelerations"):
        np.testing.assert_array_equal(ta[key], tb[key])
    assert (ia["n_iterations"], ia["converged"]) == (ib["n_iterations"], ib["converged"]) and ia["n_iterations"] >= 1
    assert len(ia["iterations"]) == len(ib["iterations"])
    for ra, rb in zip(ia["iterations"], ib["iterations"]):
        same_records(ra, rb)
        assert ra["rel_step"] == rb["rel_step"]


def test_near_pass_falls_back():
    """three agents on parallel lanes 8 m apart: every row lies far below -tau, the near form reports that and the exhaustive
    pass follows -- from the positions the first prep launch left"""
    p0 = [[2.0, 2.0], [2.0, 10.0], [2.0, 18.0]]
    pf = [[6.0, 2.5], [6.0, 10.5], [6.0, 17.5]]
    scenario = (p0, pf, [0, 0, 20, 20], 4.0, 2)
    acc0 = initial_acc("lanes", scenario)
    (ref,), ref_counts = step(scenario, acc0, 0)
    (got,), counts = step(scenario, acc0, 1)
    assert counts == ref_counts and counts[0] >= 1 and counts[1] == counts[0]
    assert_same_step(got, ref)


def test_no_pairs():
    scenario = ([[3.0, 3.0]], [[3.05, 2.95]], [0, 0, 20, 20], 2.0, 2)
    acc0 = initial_acc("single", scenario)
    (ref,), _ = step(scenario, acc0, 0)
    (got,), _ = step(scenario, acc0, 1)
    assert_same_step(got, ref)


@pytest.mark.parametrize("row_free", [True, False], ids=["row_free", "rows"])
def test_no_state_leaks_between_steps(row_free):
    case = (27, 3, 17, 10.0)
    scenario = grid(case)
    acc0 = initial_acc(case, scenario)
    (first, second), _ = step(scenario, acc0, 1, row_free=row_free, repeats=2)
    assert_same_step(second, first)
    assert not np.array_equal(first[0], acc0)  # (the step moved, and the input array was left alone)
    np.testing.assert_array_equal(acc0, initial_acc(case, scenario))
