"""grid-swap-device on the GPU: scp_generate_grid_swap against the numpy restatement (tests/scenario_device_ref.py) bit for
bit, batch invariance, unmeetable and bad parameters, and the scenarios through the solver and the batch CLI."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scenario_device_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INT_STATS = ("sweeps", "unmet_blocks", "conflicts", "ok")


def _gen(N, seeds, dim, **kw):
    from path_planning.scenarios import generate_grid_swap_batch

    init, goal, space, st = generate_grid_swap_batch(N, seeds, dim=dim, **kw)
    return init.cpu().numpy(), goal.cpu().numpy(), space.cpu().numpy(), st


def _compare(N, dim, seeds, **kw):
    init, goal, space, st = _gen(N, seeds, dim, **kw)
    assert init.shape == goal.shape == (len(seeds), N, dim) and space.shape == (len(seeds), 2 * dim)
    ref_stats = []
    for b, s in enumerate(seeds):
        ri, rg, rs, rst = R.generate(N, s, dim, **kw)
        np.testing.assert_array_equal(init[b], ri, err_msg=f"init b={b}")
        np.testing.assert_array_equal(goal[b], rg, err_msg=f"goal b={b}")
        np.testing.assert_array_equal(space[b], rs, err_msg=f"space b={b}")
        for k in INT_STATS:
            assert int(st[k][b]) == int(rst[k]), (k, b, st[k][b], rst[k])
        ma, rma = float(st["min_approach"][b]), rst["min_approach"]
        assert ma == rma or abs(ma - rma) <= np.spacing(rma), (ma, rma)
        ref_stats.append(rst)
    return ref_stats


@pytest.mark.parametrize("N,dim,B", [(16, 2, 1), (128, 2, 8), (128, 3, 8), (1000, 2, 2), (4096, 2, 1)])
def test_bitwise_default_params(N, dim, B):
    _compare(N, dim, list(range(11, 11 + B)))


def test_bitwise_other_block():
    _compare(200, 2, [5, 6, 7], block=3, min_sep=0.5)


def test_bitwise_with_sweeps():
    stats = _compare(64, 2, [3, 4, 5, 6], block=2, min_sep=1.7)
    assert any(s["sweeps"] > 0 for s in stats)
    stats = _compare(64, 2, [3], block=2, min_sep=1.75)  # sweeps run out: conflicts are left and reported
    assert stats[0]["sweeps"] == 20 and stats[0]["conflicts"] > 0


def test_batch_invariance_and_seeds():
    seeds = [9, 1, 77, 1234567890123, 5]
    init, goal, space, st = _gen(128, seeds, 2)
    for b, s in enumerate(seeds):
        i1, g1, s1, st1 = _gen(128, [s], 2)
        np.testing.assert_array_equal(init[b], i1[0])
        np.testing.assert_array_equal(goal[b], g1[0])
        np.testing.assert_array_equal(space[b], s1[0])
        assert st["min_approach"][b] == st1["min_approach"][0]
    assert not np.array_equal(goal[0], goal[1]) and not np.array_equal(init[0], init[2])


def test_unmeetable_min_sep():
    init, goal, space, st = _gen(128, [1, 2, 3], 2, min_sep=10.0)
    assert not st["ok"].any() and (st["unmet_blocks"] > 0).all() and (st["sweeps"] == 20).all()
    assert np.isfinite(init).all() and np.isfinite(goal).all() and np.isfinite(space).all()


def test_bad_arguments_leave_the_context_usable():
    from path_planning import _hip
    from path_planning.scenarios.grid_swap_device import _context

    ctx = _context(0)
    for N, D, seeds, kw in ((64, 2, [1], dict(block=1)), (64, 2, [1], dict(block=9)), (64, 4, [1], {}),
                            (0, 2, [1], {}), (64, 2, [], {})):
        with pytest.raises(_hip.HipError) as e:
            ctx.generate_grid_swap(N, D, seeds, _hip.gen_params(**kw))
        assert e.value.code == -1, e.value
    init, goal, space, st = ctx.generate_grid_swap(64, 2, [1], _hip.gen_params())
    ri, rg, _, _ = R.generate(64, 1, 2)
    np.testing.assert_array_equal(goal.cpu().numpy()[0], rg)


def test_scenario_solves_and_validates():
    from path_planning.scenarios import generate_grid_swap_device
    from path_planning.solvers.scp import SCP

    init, goal, space = generate_grid_swap_device(128, seed=2)
    solver = SCP(n_vehicles=128, time_horizon=10.0, time_step=0.2, min_distance=0.8, space_dims=space, device=0,
                 verbose=False)
    solver.set_initial_states(init)
    solver.set_final_states(goal)
    solver.generate_trajectories(max_iterations=15)
    v = solver.validate_solution()
    assert v["collision_free"] and v["min_pair_distance"] >= 0.8 - 0.011, v


def test_batch_cli_device_scenarios(tmp_path, monkeypatch):
    from path_planning.cli import compute_trajectories_batch as cli

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = cli.main(["--Ns", "64", "--trials", "8", "--scenario", "grid-swap-device", "--seed", "3",
                    "--results-dir", str(tmp_path)])
    runs = res["runs"]
    assert len(runs) == 8 and all(r["status"] == "success" and r["error"] is None for r in runs), runs
    assert all("scenario_ok" in r for r in runs)
    saved = json.load(open(next(p for p in tmp_path.iterdir() if p.suffix == ".json")))
    assert all("scenario_ok" in r for r in saved["runs"])
