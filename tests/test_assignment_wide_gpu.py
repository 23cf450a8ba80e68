"""scp_assign_goals_wide on the GPU: bit for bit against the numpy restatement (tests/assignment_ref.py) and against
scp_assign_goals under every setting of its two forks, above the one-workgroup limit and at its own, the round guard in both
kinds of round, batch independence, bad arguments, and the feature through assign_goals, SCP and the CLI."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assignment_ref as R  # noqa: E402
import assignment_wide_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KEYS = ("cost_q", "cost_q_identity", "quantum", "phases", "rounds", "bids", "status")
# "assign_wide_min_bidders": chosen by the call, every round wide, a handful of bidders narrow, every round narrow
THRESHOLDS = (0, 1, 8, 10 ** 9)
SWITCHES = [(m, lds) for m in THRESHOLDS for lds in (1, 0)]
# "assign_wide_control_threads": both sizes of the control workgroup on every case, whatever the call would choose
THREADS = [(0, -1, 256), (0, -1, 1024), (8, 0, 256), (8, 1, 1024)]


def _shared_ctx():
    from path_planning.scenarios.grid_swap_device import _context

    return _context(0)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the tests move its developer switches"""
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _switch(ctx, min_bidders, lds, threads=0):
    ctx.set_option("assign_wide_min_bidders", min_bidders)
    ctx.set_option("assign_wide_prices_in_lds", lds)
    ctx.set_option("assign_wide_control_threads", threads)


def _call(fn, start, goal, **kw):
    goal_of, st, prices = fn(start, goal, want_prices=True, **kw)
    return goal_of.cpu().numpy(), st, prices.cpu().numpy()


def _compare(name, goal_of, st, prices, ref, b=0):
    np.testing.assert_array_equal(goal_of[b], ref["goal_of"], err_msg=f"{name}: goal_of")
    np.testing.assert_array_equal(prices[b], ref["prices"], err_msg=f"{name}: prices")
    for k in STAT_KEYS:
        if k == "quantum":
            assert np.float64(st[k][b]).view(np.uint64) == np.float64(ref[k]).view(np.uint64), (name, k, st[k][b], ref[k])
        else:
            assert int(st[k][b]) == int(ref[k]), (name, k, st[k][b], ref[k])


def _same_bytes(name, got, want):
    for a, b, what in zip(got, want, ("goal_of", "stats", "prices")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, what, a, b)


# ---- 1. every form against the reference and against scp_assign_goals ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.gpu_cases()))
def test_bitwise_against_the_reference_every_form(ctx, name):
    start, goal = R.gpu_cases()[name]
    ref = R.reference(name)
    single = _call(ctx.assign_goals, start, goal)
    _compare(name, single[0], single[1], single[2], ref)
    for m, lds, threads in [(m, lds, 0) for m, lds in SWITCHES] + THREADS:
        _switch(ctx, m, lds, threads)
        wide = _call(ctx.assign_goals_wide, start, goal)
        _compare(f"{name} min_bidders={m} lds={lds} threads={threads}", wide[0], wide[1], wide[2], ref)
        _same_bytes(f"{name} min_bidders={m} lds={lds} threads={threads}", wide, single)
    _switch(ctx, 0, -1)


def test_unknown_option_keys_and_values_are_refused(ctx):
    from path_planning import _hip

    for key, value in (("assign_wide", 1), ("assign_wide_min_bidders", -1), ("assign_wide_prices_in_lds", 2),
                       ("assign_wide_prices_in_lds", -2), ("assign_wide_control_threads", 512),
                       ("assign_wide_control_threads", -1)):
        with pytest.raises(_hip.HipError) as e:
            ctx.set_option(key, value)
        assert e.value.code == -1, e.value
    _switch(ctx, 0, -1)


# ---- 2. above the old limit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(W.wide_cases()))
def test_above_the_one_workgroup_limit(name):
    start, goal = W.wide_case(name)
    ref = W.wide_reference(name)
    goal_of, st, prices = _call(_shared_ctx().assign_goals_wide, start, goal)
    _compare(name, goal_of, st, prices, ref)
    assert W.certify(start, goal, goal_of[0], prices[0])
    assert 0 <= prices.min() and prices.max() < W.price_bound(len(start))


# ---- 3. at the limit --------------------------------------------------------------------------------------------------------------
def test_at_the_limit_of_65536():
    import torch

    c = _shared_ctx()
    N = 65536
    start, goal = W.jittered_grid(N, 11, swaps=4096)
    s, g = torch.as_tensor(start, device=c.tdev), torch.as_tensor(goal, device=c.tdev)
    goal_of, st, prices = c.assign_goals_wide(s, g, want_prices=True)
    print(f"N = {N}: {int(st['phases'][0])} phases, {int(st['rounds'][0])} rounds, {int(st['bids'][0])} bids")
    assert int(st["status"][0]) == 0
    assert W.certify(s, g, goal_of[0], prices[0])
    assert int(prices.min()) >= 0 and int(prices.max()) < W.price_bound(N)
    perm = goal_of[0].cpu().numpy()
    assert W.displaced(start, goal[perm]) == 0 and int((perm != np.arange(N)).sum()) == W.displaced(start, goal)
    again = c.assign_goals_wide(s, g, want_prices=True)
    assert again[0].cpu().numpy().tobytes() == perm.tobytes() and again[1].tobytes() == st.tobytes()
    assert torch.equal(again[2], prices)


def test_beyond_the_limit_is_refused():
    import torch

    from path_planning import _hip

    c = _shared_ctx()
    pts = torch.zeros((1, 65537, 2), dtype=torch.float64, device=c.tdev)
    with pytest.raises(_hip.HipError) as e:
        c.assign_goals_wide(pts, pts)
    assert e.value.code == -1, e.value
    with pytest.raises(_hip.HipError) as e:  # the one-workgroup form keeps its own limit
        c.assign_goals(pts[:, :4097], pts[:, :4097])
    assert e.value.code == -1, e.value


# ---- 4. the guard -----------------------------------------------------------------------------------------------------------------
# identical_goals(64): every round one person wins, so round r has 65 - r bidders.  (guard, "assign_wide_min_bidders"):
# the guard strikes after a wide round | with the threshold at 8: rounds 1 .. 7 and the round it strikes at have 57 or more
# bidders, all wide | with the threshold at 60: rounds 6 and 7 (59, 58 bidders) run inside a narrow run and the guard strikes
# there | everything narrow | the call's own threshold
@pytest.mark.parametrize("guard,min_bidders", [(1, 1), (1, 8), (7, 8), (7, 60), (7, 10 ** 9), (7, 0), (70, 8)])
def test_round_guard_in_both_kinds_of_round(ctx, guard, min_bidders):
    start, goal = R.identical_goals(64)
    ref = R.auction(start, goal, max_rounds_per_phase=guard)
    single = _call(ctx.assign_goals, start, goal, max_rounds_per_phase=guard)
    for lds in (1, 0):
        _switch(ctx, min_bidders, lds)
        wide = _call(ctx.assign_goals_wide, start, goal, max_rounds_per_phase=guard)
        assert wide[1]["status"][0] == ref["status"]
        if guard <= 7:  # (the first phase needs 64 rounds)
            assert ref["status"] == 1 and wide[0][0].tolist() == list(range(64))
        _compare(f"guard {guard}", wide[0], wide[1], wide[2], ref)
        _same_bytes(f"guard {guard}", wide, single)
        # the next call on the same ctx, with the default guard, is right
        wide = _call(ctx.assign_goals_wide, start, goal)
        _compare("identical-goals-64", wide[0], wide[1], wide[2], R.reference("identical-goals-64"))
    _switch(ctx, 0, -1)


# ---- 5. batch independence --------------------------------------------------------------------------------------------------------
def test_batch_independence(ctx):
    N = 130
    rng = np.random.default_rng(77)
    side = 12
    far = np.array([(k // side, k % side) for k in range(N)], dtype=np.float64) * 10.0
    scen = [R.uniform(N, 2, 2130),                                           # ~ hundreds of rounds
            (far, far + rng.uniform(-1.0, 1.0, (N, 2))),                     # the identity is optimal: one round per phase
            (rng.uniform(0.0, 20.0, (N, 2)), np.tile([[7.0, 5.0]], (N, 1)))]  # identical goals: N rounds per phase
    start, goal = np.stack([s for s, _ in scen]), np.stack([g for _, g in scen])
    rounds = None
    for m, lds in SWITCHES:
        _switch(ctx, m, lds)
        batch = _call(ctx.assign_goals_wide, start, goal)
        for b in range(3):
            one = _call(ctx.assign_goals_wide, start[b], goal[b])
            _same_bytes(f"scenario {b} min_bidders={m} lds={lds}", [a[b:b + 1] for a in batch], one)
        if rounds is None:
            rounds = batch[1]["rounds"].tolist()
            _compare("uniform-2d-130", batch[0], batch[1], batch[2], R.reference("uniform-2d-130"), b=0)
            assert batch[1]["status"].tolist() == [0, 0, 0]
            assert rounds[2] >= 10 * rounds[1], rounds  # (identical goals: at least N rounds per phase)
        assert batch[1]["rounds"].tolist() == rounds
    _same_bytes("batch, single", batch, _call(ctx.assign_goals, start, goal))
    _switch(ctx, 0, -1)


# ---- 6. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_context_usable(ctx):
    import torch

    from path_planning import _hip

    for N, D in ((8, 4), (8, 1)):
        pts = torch.zeros((1, N, D), dtype=torch.float64, device=ctx.tdev)
        with pytest.raises(_hip.HipError) as e:
            ctx.assign_goals_wide(pts, pts)
        assert e.value.code == -1, e.value
    lib, pts = ctx.lib, torch.zeros((1, 8, 2), dtype=torch.float64, device=ctx.tdev)
    out = torch.zeros(64, dtype=torch.int64, device=ctx.tdev)
    for B, N in ((0, 8), (1, 0)):
        assert lib.scp_assign_goals_wide(ctx.h, B, N, 2, pts.data_ptr(), pts.data_ptr(), out.data_ptr(), None, 0,
                                         out.data_ptr()) == -1
    assert lib.scp_assign_goals_wide(ctx.h, 1, 8, 2, pts.data_ptr(), pts.data_ptr(), None, None, 0, out.data_ptr()) == -1
    start, goal = R.reversed_lines(8)
    bad = start.copy()
    bad[3, 1] = np.nan
    huge = start.copy()
    huge[0, 0], huge[1, 0] = 1.5e308, -1.5e308  # finite coordinates, a range that overflows
    for m in (0, 1, 10 ** 9):
        _switch(ctx, m, -1)
        for s in (bad, huge):
            with pytest.raises(_hip.HipError) as e:  # (after the launch)
                ctx.assign_goals_wide(s, goal)
            assert e.value.code == -1, e.value
            goal_of, st, _ = ctx.assign_goals_wide(start, goal)
            assert goal_of.cpu().numpy()[0].tolist() == list(range(7, -1, -1)) and st["status"][0] == 0
    _switch(ctx, 0, -1)


# ---- 7. the Python surface --------------------------------------------------------------------------------------------------------
def test_scp_object_beyond_4096_vehicles():
    from path_planning import _hip
    from path_planning.solvers.scp import SCP

    name = "jittered-grid-4100"
    start, goal = W.wide_case(name)
    solver = SCP(n_vehicles=4100, time_horizon=10.0, time_step=0.5, min_distance=0.5, space_dims=[-5, -5, 140, 140], device=0,
                 verbose=False)
    solver.set_initial_states(start)
    solver.set_final_states(goal)
    perm = solver.assign_goals()
    ref = W.wide_reference(name)
    assert perm.tolist() == ref["goal_of"].tolist()
    info = solver.assignment_info
    assert (info["cost_q"], info["cost_q_identity"], info["rounds"], info["status"]) == (
        ref["cost_q"], ref["cost_q_identity"], ref["rounds"], 0)
    assert info["line_after"]["n_opposed"] == 0
    np.testing.assert_array_equal(solver.final_positions.reshape(4100, 2), goal[perm])
    with pytest.raises(_hip.HipError):  # the one-workgroup form still refuses the size
        solver.assign_goals(method="single")


def test_methods_agree_and_bad_methods_are_refused():
    from path_planning.scenarios import assign_goals, assign_goals_batch
    from path_planning.solvers.scp import SCP

    start, goal = R.uniform(300, 2, 2300)
    ref = R.reference("uniform-2d-300")
    results = {m: assign_goals(start, goal, min_sep=0.8, method=m) for m in ("auto", "single", "wide")}
    for m, (goal_of, info) in results.items():
        assert goal_of.tolist() == ref["goal_of"].tolist(), m
        assert info == results["single"][1], m
    gb, ib = assign_goals_batch(np.stack([start, start]), np.stack([goal, goal[::-1]]), method="wide")
    gs, is_ = assign_goals_batch(np.stack([start, start]), np.stack([goal, goal[::-1]]), method="single")
    assert gb.cpu().numpy().tobytes() == gs.cpu().numpy().tobytes() and ib["rounds"].tolist() == is_["rounds"].tolist()
    with pytest.raises(ValueError):
        assign_goals(start, goal, method="widest")
    with pytest.raises(ValueError):
        assign_goals_batch(start[None], goal[None], method=None)

    solver = SCP(n_vehicles=300, time_horizon=10.0, time_step=0.5, min_distance=0.5, space_dims=[-5, -5, 60, 60], device=0,
                 verbose=False)
    solver.set_initial_states(start)
    solver.set_final_states(goal)
    perms = {m: (solver.assign_goals(method=m).tolist(), dict(solver.assignment_info)) for m in ("single", "wide", "auto")}
    assert perms["wide"] == perms["single"] == perms["auto"] and perms["wide"][0] == ref["goal_of"].tolist()
    with pytest.raises(ValueError):
        solver.assign_goals(method="both")


def test_cli_assign_method_prints_the_same_line(capsys, monkeypatch):
    from path_planning.cli import compute_trajectories as cli

    # the eight crossing lines of tests/test_assignment_gpu.py (moved off the arena's edge)
    start = np.array([[2.0 * i + 2.0, 2.0] for i in range(8)])
    goal = np.array([[2.0 * (7 - i) + 2.0, 12.0] for i in range(8)])
    monkeypatch.setattr(cli, "generate_positions", lambda n, r, seed=None: (start.copy(), goal.copy()))
    argv = ["--n-agents", "8", "--time-horizon", "10", "--time-step", "0.5", "--min-distance", "0.5", "--space", "0", "0", "30",
            "20", "--no-plots", "--assign-goals"]
    lines = {}
    for method in (None, "wide", "single"):
        solver = cli.main(argv + (["--assign-method", method] if method else []))
        out = capsys.readouterr().out
        line = [ln for ln in out.split("\n") if ln.startswith("Goal assignment:")]
        assert solver is not None and len(line) == 1, out
        assert solver.goal_assignment.tolist() == list(range(7, -1, -1))
        lines[method] = line[0]
    assert lines["wide"] == lines[None] == lines["single"] and "opposed pairs 28 -> 0" in lines[None]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--assign-method", "both"])
