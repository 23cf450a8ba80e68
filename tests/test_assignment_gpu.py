"""Goal assignment on the GPU: scp_assign_goals and scp_straight_line_check against the numpy restatement
(tests/assignment_ref.py) bit for bit, batch independence, the round guard, bad arguments, and the feature through SCP and the
two CLIs."""
import csv
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assignment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KEYS = ("cost_q", "cost_q_identity", "quantum", "phases", "rounds", "bids", "status")
LINE_KEYS = ("min_approach", "arg_i", "arg_j", "n_close", "n_opposed")
MIN_SEP = 0.8


def _ctx():
    from path_planning.scenarios.grid_swap_device import _context

    return _context(0)


def _assign(start, goal, **kw):
    goal_of, st, prices = _ctx().assign_goals(start, goal, want_prices=True, **kw)
    return goal_of.cpu().numpy(), st, prices.cpu().numpy()


def _same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _compare_assign(name, goal_of, st, prices, ref, b=0):
    np.testing.assert_array_equal(goal_of[b], ref["goal_of"], err_msg=f"{name}: goal_of")
    np.testing.assert_array_equal(prices[b], ref["prices"], err_msg=f"{name}: prices")
    for k in STAT_KEYS:
        got = st[k][b]
        if k == "quantum":
            assert _same_bits(got, ref[k]), (name, k, got, ref[k])
        else:
            assert int(got) == int(ref[k]), (name, k, got, ref[k])


def _compare_line(name, got, ref, b=0):
    for k in LINE_KEYS:
        if k == "min_approach":
            assert _same_bits(got[k][b], ref[k]), (name, k, got[k][b], ref[k])
        else:
            assert int(got[k][b]) == int(ref[k]), (name, k, got[k][b], ref[k])


@pytest.mark.parametrize("name", sorted(R.gpu_cases()))
def test_bitwise_against_the_reference(name):
    start, goal = R.gpu_cases()[name]
    ref = R.reference(name)
    goal_of, st, prices = _assign(start, goal)
    _compare_assign(name, goal_of, st, prices, ref)
    # the straight-line check with the given pairing and with the assignment
    ctx = _ctx()
    _compare_line(name, ctx.straight_line_check(start, goal, None, MIN_SEP), R.line_check(start, goal, None, MIN_SEP))
    after = ctx.straight_line_check(start, goal, goal_of[0], MIN_SEP)
    _compare_line(name, after, R.line_check(start, goal, ref["goal_of"], MIN_SEP))
    # (N + 1) c < 2^53 on every case of the list (c < 2^31, N <= 4096): no motion is opposed after the assignment
    assert int(after["n_opposed"][0]) == 0, (name, after)


def test_known_assignments():
    start, goal = R.reversed_lines(32)
    goal_of, st, _ = _assign(start, goal)
    assert goal_of[0].tolist() == list(range(31, -1, -1)) and st["cost_q"][0] < st["cost_q_identity"][0]
    start, goal = R.optimal_identity()
    goal_of, st, _ = _assign(start, goal)
    assert goal_of[0].tolist() == list(range(len(start))) and st["cost_q"][0] == st["cost_q_identity"][0]
    start, goal = R.identical_points()
    goal_of, st, _ = _assign(start, goal)
    assert sorted(goal_of[0].tolist()) == list(range(len(start)))
    assert (st["cost_q"][0], st["quantum"][0], st["phases"][0]) == (0, 1.0, 1)
    goal_of, st, _ = _assign(*R.uniform(1, 3, 3001))
    assert goal_of.tolist() == [[0]] and (st["phases"][0], st["rounds"][0], st["status"][0]) == (0, 0, 0)


@pytest.mark.parametrize("D", [2, 3])
def test_batch_independence(D):
    names = [f"uniform-{D}d-130"] * 5
    scen = [R.uniform(130, D, 1000 * D + 130)] + [R.uniform(130, D, 40 + b) for b in range(1, 5)]
    scen[3] = (scen[3][0], np.tile(scen[3][1][:1], (130, 1)))  # one price war among them
    start, goal = np.stack([s for s, _ in scen]), np.stack([g for _, g in scen])
    goal_of, st, prices = _assign(start, goal)
    _compare_assign(names[0], goal_of, st, prices, R.reference(names[0]), b=0)
    line = _ctx().straight_line_check(start, goal, goal_of, MIN_SEP)
    for b in range(5):
        g1, st1, p1 = _assign(start[b], goal[b])
        np.testing.assert_array_equal(goal_of[b], g1[0])
        np.testing.assert_array_equal(prices[b], p1[0])
        assert st[b].tobytes() == st1[0].tobytes(), (b, st[b], st1[0])
        l1 = _ctx().straight_line_check(start[b], goal[b], g1[0], MIN_SEP)
        assert line[b].tobytes() == l1[0].tobytes(), (b, line[b], l1[0])


def test_round_guard_gives_the_identity():
    start, goal = R.identical_goals(64)
    ref = R.auction(start, goal, max_rounds_per_phase=1)
    goal_of, st, prices = _assign(start, goal, max_rounds_per_phase=1)  # (returns: the call is SCP_OK)
    assert st["status"][0] == 1 and goal_of[0].tolist() == list(range(64))
    _compare_assign("guard", goal_of, st, prices, ref)
    # the default guard leaves the same case alone
    goal_of, st, prices = _assign(start, goal)
    _compare_assign("identical-goals-64", goal_of, st, prices, R.reference("identical-goals-64"))


def test_bad_arguments_leave_the_context_usable():
    import torch

    from path_planning import _hip

    ctx = _ctx()
    for N, D in ((4097, 2), (8, 4), (8, 1)):
        pts = torch.zeros((1, N, D), dtype=torch.float64, device=ctx.tdev)
        with pytest.raises(_hip.HipError) as e:
            ctx.assign_goals(pts, pts)
        assert e.value.code == -1, e.value
        with pytest.raises(_hip.HipError) as e:
            ctx.straight_line_check(pts, pts) if D != 2 else ctx.straight_line_check(pts[:, :8], pts[:, :8], min_sep=-1.0)
        assert e.value.code == -1, e.value
    lib, pts = ctx.lib, torch.zeros((1, 8, 2), dtype=torch.float64, device=ctx.tdev)
    out = torch.zeros(64, dtype=torch.int64, device=ctx.tdev)
    for B, N in ((0, 8), (1, 0)):
        assert lib.scp_assign_goals(ctx.h, B, N, 2, pts.data_ptr(), pts.data_ptr(), out.data_ptr(), None, 0,
                                    out.data_ptr()) == -1
        assert lib.scp_straight_line_check(ctx.h, B, N, 2, pts.data_ptr(), pts.data_ptr(), None, 0.0, out.data_ptr()) == -1
    assert lib.scp_assign_goals(ctx.h, 1, 8, 2, pts.data_ptr(), pts.data_ptr(), None, None, 0, out.data_ptr()) == -1
    start, goal = R.reversed_lines(8)
    bad = start.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_hip.HipError) as e:
        ctx.assign_goals(bad, goal)
    assert e.value.code == -1, e.value
    with pytest.raises(_hip.HipError) as e:  # an entry of goal_of that is no index: refused, nothing read out of bounds
        ctx.straight_line_check(start, goal, np.array([0, 1, 2, 3, 4, 5, 6, 8], dtype=np.int32))
    assert e.value.code == -1, e.value
    goal_of, _, _ = ctx.assign_goals(start, goal)
    assert goal_of.cpu().numpy()[0].tolist() == list(range(7, -1, -1))


@pytest.mark.parametrize("D", [2, 3])
def test_line_check_equals_the_generators_min_approach(D):
    from path_planning.scenarios import generate_grid_swap_batch

    init, goal, _, st = generate_grid_swap_batch(128, [21, 22, 23], dim=D)
    line = _ctx().straight_line_check(init, goal, None, 0.3)
    for b in range(3):
        assert _same_bits(line["min_approach"][b], st["min_approach"][b]), (b, line["min_approach"][b], st["min_approach"][b])
        assert (line["n_close"][b] == 0) == bool(st["ok"][b])
    _compare_line("grid-swap", line, R.line_check(init[0].cpu().numpy(), goal[0].cpu().numpy(), None, 0.3))


def test_python_surface():
    from path_planning.scenarios import assign_goals, assign_goals_batch

    start, goal = R.uniform(65, 2, 2065)
    ref = R.reference("uniform-2d-65")
    goal_of, info = assign_goals(start, goal, min_sep=MIN_SEP)
    assert goal_of.tolist() == ref["goal_of"].tolist()
    assert (info["cost_q"], info["cost_q_identity"], info["status"]) == (ref["cost_q"], ref["cost_q_identity"], 0)
    assert info["line_after"]["n_opposed"] == 0 and info["line_before"] == R.line_check(start, goal, None, MIN_SEP)
    gb, ib = assign_goals_batch(np.stack([start, start]), np.stack([goal, goal[::-1]]), min_sep=MIN_SEP)
    assert gb.shape == (2, 65) and gb[0].cpu().numpy().tolist() == goal_of.tolist()
    assert ib["cost_q"].tolist() == [ref["cost_q"]] * 2 and ib["line_after"]["n_opposed"].tolist() == [0, 0]


def _crossing_solver():
    from path_planning.solvers.scp import SCP

    solver = SCP(n_vehicles=8, time_horizon=10.0, time_step=0.5, min_distance=0.5, space_dims=[-5, -5, 25, 20], device=0,
                 verbose=False)
    start = np.array([[2.0 * i, 0.0] for i in range(8)])
    goal = np.array([[2.0 * (7 - i), 10.0] for i in range(8)])
    return solver, start, goal


def test_end_to_end_crossing_lines():
    solver, start, goal = _crossing_solver()
    with pytest.raises(ValueError):
        solver.assign_goals()
    solver.set_initial_states(start)
    solver.set_final_states(goal)
    solver.generate_trajectories(max_iterations=1)
    assert solver.last_info["initially_feasible"] is False  # all eight straight lines meet at (7, 5)
    vf = np.arange(16, dtype=float).reshape(8, 2) * 0.01
    solver.set_final_states(goal, vf)
    perm = solver.assign_goals()
    assert perm.tolist() == list(range(7, -1, -1)) and solver.goal_assignment.tolist() == perm.tolist()
    np.testing.assert_array_equal(solver.final_positions.reshape(8, 2), goal[perm])
    np.testing.assert_array_equal(solver.final_velocities.reshape(8, 2), vf[perm])
    info = solver.assignment_info
    assert info["line_before"]["n_opposed"] == 28 and info["line_after"]["n_opposed"] == 0
    assert info["line_before"]["min_approach"] < 1e-9 and info["line_after"]["min_approach"] == 2.0
    assert info["cost_q"] < info["cost_q_identity"] and info["status"] == 0
    # a second call starts from the order given to set_final_states: it does not compose
    assert solver.assign_goals().tolist() == perm.tolist()
    np.testing.assert_array_equal(solver.final_positions.reshape(8, 2), goal[perm])
    solver.set_final_states(goal)  # (zero final velocities: the straight flight is QP#0's answer)
    solver.assign_goals()
    solver.generate_trajectories(max_iterations=15)
    assert solver.last_info["n_iterations"] == 0 and solver.last_info["initially_feasible"]
    assert solver.validate_solution()["collision_free"]
    np.testing.assert_allclose(solver.trajectories["positions"][:, 0, :], start, atol=1e-9)


def test_cli_single_solve_prints_the_assignment(capsys):
    from path_planning.cli import compute_trajectories as cli

    solver = cli.main(["--n-agents", "16", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20",
                       "--seed", "4", "--no-plots", "--assign-goals"])
    out = capsys.readouterr().out
    line = [ln for ln in out.split("\n") if ln.startswith("Goal assignment:")]
    assert solver is not None and len(line) == 1, out
    assert "m^2" in line[0] and "minimum approach" in line[0] and "opposed pairs" in line[0]
    assert sorted(solver.goal_assignment.tolist()) == list(range(16)) and solver.assignment_info["line_after"]["n_opposed"] == 0


RECORD_KEYS = ["N", "status", "time_sec", "error", "K", "T", "h", "seed", "scp_iterations", "converged", "iteration_time_sec",
               "rel_steps", "qp_iterations", "qp_status", "qp_residuals", "working_rows", "qp_pipeline", "persist_gave_up",
               "rho_switches_in_kernel", "trial_index"]


def test_batch_cli_flag_adds_keys_only_when_given(tmp_path, monkeypatch, capsys):
    from path_planning.cli import compute_trajectories_batch as cli

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    plain_dir, flag_dir = tmp_path / "plain", tmp_path / "flag"
    plain = cli.main(["--Ns", "16", "--trials", "2", "--seed", "3", "--results-dir", str(plain_dir)])
    capsys.readouterr()
    flagged = cli.main(["--Ns", "16", "--trials", "2", "--seed", "3", "--results-dir", str(flag_dir), "--assign-goals"])
    out = capsys.readouterr().out
    assert sum("Goal assignment:" in ln for ln in out.split("\n")) == 2, out
    for r in plain["runs"]:
        assert r["status"] == "success" and list(r) == RECORD_KEYS, list(r)
    assert "assign_goals" not in plain["meta"]["config"] and flagged["meta"]["config"]["assign_goals"] is True
    for r in flagged["runs"]:
        assert r["status"] == "success", r
        assert list(r) == RECORD_KEYS[:9] + ["goal_assignment", "assign_ms"] + RECORD_KEYS[9:], list(r)
        assert sorted(r["goal_assignment"]) == list(range(16)) and r["assign_ms"] > 0
    saved = json.load(open(next(p for p in plain_dir.iterdir() if p.suffix == ".json")))
    assert [list(r) for r in saved["runs"]] == [RECORD_KEYS] * 2
    for d in (plain_dir, flag_dir):
        header = next(csv.reader(open(next(p for p in d.iterdir() if p.suffix == ".csv"))))
        assert header == cli.CSV_FIELDS
