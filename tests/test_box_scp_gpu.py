"""SCP solves with per-state position boxes (SCP.set_position_boxes): whole solves against the boxed oracle loop
(qo.scp_solve(pos_boxes=...)) in the form of tests/test_scp_gpu.py::test_scp_matches_oracle, the unique minimiser at
eps = 1e-8, and the solver's other modes (polish, refresh_feasibility, repair_conflicts) with boxes set.

Boxes: box_cases.waypoint_boxes around the BOX-FREE oracle plan (two PCG steps, default tolerances) -- a waypoint some
vehicles must pass at state K / 2, displaced from where they would fly, widening over the neighbouring states."""
import functools

import numpy as np
import pytest

import box_cases as bc
import holds_ref as hr
from oracle import qp_oracle as qo
from test_scp_gpu import CG_CASES, check_solution_properties

pytestmark = pytest.mark.gpu
LEAN = {"persistent16", "persistent8-lean"}
R, SHAPES, scenario = bc.SCP_R, bc.SCP_SHAPES, bc.scp_scenario


@functools.lru_cache(maxsize=None)
def oracle_solve(name, cg):
    prob, lo, hi = scenario(name)[3:6]
    return qo.scp_solve(prob, 15, qo.Settings(max_iter=10000, cg_iters=cg), pos_boxes=(lo, hi))


def boxed_solver(name, max_iterations=15, **kw):
    from path_planning.solvers.scp import SCP

    n, dim, T, h = SHAPES[name][:4]
    p0, pf, space, prob, lo, hi = scenario(name)[:6]
    s = SCP(n_vehicles=n, time_horizon=T, time_step=h, min_distance=R, space_dims=space, dim=dim, verbose=False, **kw)
    assert s.K == prob.K
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s.set_position_boxes(lo, hi)
    return s, s.generate_trajectories(max_iterations=max_iterations)


def box_excess(name, positions):
    """how far the worst boxed state lies outside its box (negative: inside)"""
    lo, hi = scenario(name)[4:6]
    return float(np.maximum(lo - positions, positions - hi)[np.isfinite(lo)].max())


def pipelines(s):
    return {p for it in s.last_info["iterations"] for p in it["pipeline"].split("+")}


@pytest.mark.parametrize("cg,tol", CG_CASES)
@pytest.mark.parametrize("name", ["n4", "n10", "grid3d"])
def test_boxed_scp_matches_oracle(name, cg, tol):
    n, dim = SHAPES[name][:2]
    prob, free = scenario(name)[3], scenario(name)[6]
    out = oracle_solve(name, cg)
    assert [i["status_val"] for i in out["infos"]] == [1] * len(out["infos"]) and out["iterations"] >= 1
    assert np.abs(out["positions"] - free).max() > 0.15  # the boxes move the plan
    got = {}
    for native in (True, False):
        s, traj = boxed_solver(name, native=native, qp_settings={"cg_iters": cg})
        assert s.last_info["n_iterations"] == out["iterations"]
        assert s.last_info["converged"] == out["converged"]
        assert s.last_info["qp0"]["iter"] == out["infos"][0]["iter"]
        for a, b in zip(s.last_info["iterations"], out["infos"][1:]):
            if cg > 1:
                assert a["iter"] == b["iter"] and a["working_rows"] == b["working_rows"] and a["rounds"] == b["rounds"]
            else:
                assert abs(a["iter"] - b["iter"]) <= 50 and a["rounds"] == b["rounds"]
        np.testing.assert_allclose([i["rel_step"] for i in s.last_info["iterations"]], out["rel_steps"],
                                   rtol=1e-6 if cg > 1 else 0.05, atol=0 if cg > 1 else 2e-3)
        for key in ("positions", "velocities", "accelerations"):
            assert traj[key].shape == (n, prob.K, dim) and traj[key].dtype == np.float64
            np.testing.assert_allclose(traj[key], out[key], rtol=0, atol=tol if key == "positions" or cg > 1 else 10 * tol)
        pipes = pipelines(s)
        assert not pipes & LEAN and (cg > 1 or "persistent" in pipes), pipes
        print(f"boxed SCP {name} cg={cg} native={native}: {s.last_info['n_iterations']} iterations, pipelines {sorted(pipes)}, "
              f"max |positions - oracle| = {np.abs(traj['positions'] - out['positions']).max():.3e}, "
              f"box excess {box_excess(name, traj['positions']):.2e}")
        got[native] = traj["accelerations"].copy()
        s.close()
    np.testing.assert_array_equal(got[True], got[False])


@pytest.mark.parametrize("name", ["n4", "n6"])
def test_boxed_default_path_reaches_the_oracle_minimiser(name):
    """eps = 1e-8, the default single PCG step, two SCP iterations: every QP has one minimiser, boxes or not, so the boxed
    waypoints match the numpy oracle at 1e-6 (test_scp_gpu.py::test_default_path_reaches_the_oracle_minimiser, whose C
    oracle takes no boxes)."""
    prob, lo, hi = scenario(name)[3:6]
    tight = {"eps_abs": 1e-8, "eps_rel": 1e-8, "max_iter": 40000, "max_iter0": 4000}  # (qo.scp_solve caps QP#0 at 4000)
    s, traj = boxed_solver(name, max_iterations=2, qp_settings=tight)
    assert s._native.settings.cg_iters == 1 and s._native.settings.persistent == 1  # the defaults
    ref = qo.scp_solve(prob, 2, qo.Settings(max_iter=40000, eps_abs=1e-8, eps_rel=1e-8), pos_boxes=(lo, hi))
    assert s.last_info["n_iterations"] == ref["iterations"] >= 1
    for a, b in zip(s.last_info["iterations"], ref["infos"][1:]):
        assert a["status_val"] == b["status_val"] == 1 and a["working_rows"] == b["working_rows"], (a, b)
    assert not pipelines(s) & LEAN
    np.testing.assert_allclose(traj["positions"], ref["positions"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(traj["accelerations"], ref["accelerations"], rtol=0, atol=1e-5)
    assert box_excess(name, traj["positions"]) < 1e-6 and box_excess(name, traj["positions"]) > -1e-6  # a box is active
    s.close()


@pytest.mark.parametrize("name", ["n10", "grid3d"])
def test_polish_holds_the_boxes(name):
    """polish=True: every boxed state inside its box to 1e-6, the bound of test_polish_meets_every_constraint for every other
    constraint; without it to 3e-2, the bound of check_solution_properties"""
    s, traj = boxed_solver(name, polish=True)
    assert s.last_info["polish"]["status_val"] in (1, 2) and s.last_info["polish"]["unresolved_rows"] == 0
    assert not set(s.last_info["polish"]["pipeline"].split("+")) & LEAN
    check_solution_properties(s, traj, tol=1e-6)
    assert box_excess(name, traj["positions"]) <= 1e-6
    s0, t0 = boxed_solver(name)
    check_solution_properties(s0, t0)
    print(f"boxed polish {name}: box excess {box_excess(name, traj['positions']):.2e} polished, "
          f"{box_excess(name, t0['positions']):.2e} without")
    assert "polish" not in s0.last_info and box_excess(name, t0["positions"]) <= 3e-2
    s.close()
    s0.close()


@pytest.mark.parametrize("native", [True, False])
def test_refresh_feasibility_with_boxes(native):
    s, traj = boxed_solver("n10", refresh_feasibility=True, native=native)
    assert s.last_info["n_iterations"] >= 1 and not pipelines(s) & LEAN, pipelines(s)
    assert {it["status_val"] for it in s.last_info["iterations"]} <= {1, 2}
    check_solution_properties(s, traj)
    assert box_excess("n10", traj["positions"]) <= 3e-2
    s.close()


def test_repair_conflicts_with_a_box():
    """A ring scenario of tests/test_holds_gpu.py with one waypoint box (vehicle 0, 0.4 m off its box-free plan): every QP of
    every repair pass runs without a lean kernel, and an accepted pass keeps the boxed states inside to 3e-2."""
    from test_holds_gpu import make_solver

    N, rad, T, h, seed = 12, 6.0, 7.5, 0.3, 12
    p0, pf = hr.ring_scenario(N, rad, seed)
    s = make_solver(N, T, h, p0, pf, 0.5)
    free = s.generate_trajectories(max_iterations=15)["positions"]
    lo, hi = bc.waypoint_boxes(free[:1], 0.2, 0.4, 3)
    lo = np.concatenate([lo, np.full((N - 1,) + lo.shape[1:], -np.inf)])
    hi = np.concatenate([hi, np.full((N - 1,) + hi.shape[1:], np.inf)])
    s.set_position_boxes(lo, hi)
    traj = s.generate_trajectories(max_iterations=15)
    before = s.validate_solution(continuous=True, conflicts=True)
    pipes = []
    solve = s._solve_with_avoidance_constraints

    def spy(*a, **kw):
        out = solve(*a, **kw)
        pipes.append(s._last_qp_info["pipeline"])
        return out

    s._solve_with_avoidance_constraints = spy
    rep = s.repair_conflicts()
    excess = float(np.maximum(lo - s.trajectories["positions"], s.trajectories["positions"] - hi)[np.isfinite(lo)].max())
    print(f"boxed ring N={N}: {before['n_conflicts']} conflicts before, repair {rep['stopped_by']} after {rep['passes']} passes "
          f"({rep['conflicts_per_pass']}), {len(pipes)} QPs on {sorted(set(pipes))}, box excess {excess:.2e}")
    assert np.abs(traj["positions"] - free).max() > 0.2  # the box moves the plan
    assert before["n_conflicts"] >= 1 and rep["passes"] >= 1  # (6 conflicts; clean after 3 passes, 5 QPs, on an MI355X)
    assert len(pipes) == sum(rep["iterations_per_pass"])
    assert not {p for q in pipes for p in q.split("+")} & LEAN, pipes
    if rep["stopped_by"] != "qp_status":
        assert excess <= 3e-2
    s.close()
