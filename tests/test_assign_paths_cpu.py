"""Goal assignment by path length, the parts that need no GPU: the matrix auction of tests/assign_paths_ref.py is the auction
of tests/assignment_ref.py and exactly optimal, path_costs keeps its promises, and the two new entry points are declared."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_paths_ref as P  # noqa: E402
import assignment_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUCTION_KEYS = ("goal_of", "prices", "cost_q", "cost_q_identity", "rounds", "bids", "phases", "status", "longest_phase", "eps_last")


@pytest.mark.parametrize("name", sorted(R.gpu_cases()))
def test_matrix_auction_is_the_coordinate_auction(name):
    """on the quantised costs and the top of the quantisation, every number of the old auction comes out again"""
    start, goal = R.gpu_cases()[name]
    c, _, top = R.quantise(start, goal)
    want = R.reference(name)
    got = P.auction_costs(c, top=top)
    for k in AUCTION_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")
    if name == "identical-goals-64":  # the round guard, on the case the old tests use for it
        got, want = P.auction_costs(c, max_rounds_per_phase=1, top=top), R.auction(start, goal, max_rounds_per_phase=1)
        assert got["status"] == 1 and got["goal_of"].tolist() == list(range(64))
        for k in AUCTION_KEYS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"guard: {k}")


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7])
def test_optimal_against_brute_force(N):
    for seed in range(4):
        for c in (P.random_matrix(N, 10 * N + seed, high=50), P.random_matrix(N, 10 * N + seed, high=6),  # (many ties)
                  P.random_matrix(N, 10 * N + seed, high=2 ** 31)):
            out = P.auction_costs(c)
            assert sorted(out["goal_of"].tolist()) == list(range(N)) and out["status"] == 0 and out["eps_last"] == 1
            assert out["cost_q"] == R.brute_force(c), (N, seed)


def test_optimal_against_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(77)
    for trial in range(24):
        N = int(rng.integers(2, 65))
        rows = N // 3 if trial % 3 else 0  # (sentinel entries: N * 999 + 1 at the most)
        c = P.random_matrix(N, 900 + trial, high=int(rng.choice([4, 1000] if rows else [4, 1000, 2 ** 31])), sentinel_rows=rows)
        out = P.auction_costs(c)
        r, j = lsa(c)
        assert sorted(out["goal_of"].tolist()) == list(range(N))
        assert out["cost_q"] == int(c[r, j].sum()), (trial, N)
        # eps-complementary slackness with the returned prices (eps = 1 on costs scaled by N + 1)
        v = -(N + 1) * c - out["prices"][None, :]
        assert (v[np.arange(N), out["goal_of"]] >= v.max(1) - 1).all()
    for name, c in P.gpu_matrices().items():
        r, j = lsa(c)
        assert P.reference(name)["cost_q"] == int(c[r, j].sum()), name


def _hops(N, seed, unreachable=0.0, high=40):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, high, (N, N), dtype=np.int64)
    h[rng.random((N, N)) < unreachable] = 0xFFFF
    return h, rng.uniform(0.0, 90.0, (N, N))


def test_path_costs_promises():
    from path_planning.scenarios.assignment import MAX_TIE_BITS, path_costs

    for N, seed, unreachable, high, power in ((6, 1, 0.2, 40, 2), (64, 2, 0.05, 300, 2), (64, 3, 0.05, 300, 1), (300, 4, 0.3, 2000, 1),
                                              (5, 5, 0.0, 3, 2), (4096, 6, 0.001, 700, 2)):
        hops, d2 = _hops(N, seed, unreachable, high)
        c, how = path_costs(hops, d2, power)
        b, U, Hmax = how["tie_bits"], how["unreachable_cost"], how["max_hops"]
        finite = hops != 0xFFFF
        assert c.dtype == np.int64 and c.min() >= 0 and c.max() <= 2 ** 31 - 1
        assert Hmax == hops[finite].max()
        # the bit budget: b is the largest value of 0 .. 12 that fits
        assert 0 <= b <= MAX_TIE_BITS and N * (Hmax ** power + 1) * 2 ** b <= 2 ** 31 - 1
        assert b == MAX_TIE_BITS or N * (Hmax ** power + 1) * 2 ** (b + 1) > 2 ** 31 - 1
        # hops decide, the straight-line distance only breaks ties
        assert ((c >> b) == hops ** power)[finite].all()
        tie = c & (2 ** b - 1)
        order = np.argsort(d2[finite], kind="stable")
        assert (np.diff(tie[finite][order]) >= 0).all()  # monotone in d2
        if b > 0:
            assert tie[finite].max() == 2 ** b - 1 or not finite.flat[np.argmax(d2)]
        # dominance: one unreachable pair costs more than any assignment without one
        assert (c[~finite] == U).all() and U == N * int(c[finite].max()) + 1 and U > N * int(c[finite].max())
    # the int16 view of the device's uint16 words, and a torch tensor, are the same matrix
    hops, d2 = _hops(7, 9, 0.3)
    want, how = path_costs(hops, d2)
    got, how16 = path_costs(hops.astype(np.uint16).view(np.int16), d2)
    np.testing.assert_array_equal(got, want)
    import torch

    got, howt = path_costs(torch.as_tensor(hops.astype(np.uint16).view(np.int16)), torch.as_tensor(d2))
    np.testing.assert_array_equal(got, want)
    assert how == how16 == howt


def test_path_costs_edge_cases():
    from path_planning.scenarios.assignment import path_costs

    # max d2 == 0: the tie-break term is 0
    hops = np.array([[0, 3], [2, 0xFFFF]])
    c, how = path_costs(hops, np.zeros((2, 2)), 2)
    assert how == {"tie_bits": 12, "unreachable_cost": 2 * (9 << 12) + 1, "max_hops": 3}
    assert c.tolist() == [[0, 9 << 12], [4 << 12, 2 * (9 << 12) + 1]]
    # nothing reachable: every pair costs U = 1
    c, how = path_costs(np.full((3, 3), 0xFFFF), np.ones((3, 3)))
    assert (c == 1).all() and how == {"tie_bits": 12, "unreachable_cost": 1, "max_hops": 0}
    # nothing fits: 4096 (32767^2 + 1) > 2^31 - 1; power = 1 does
    hops, d2 = _hops(4096, 11, 0.0, 100)
    hops[5, 7] = 32767
    with pytest.raises(ValueError, match=r"power=1 or a larger stride"):
        path_costs(hops, d2, 2)
    c, how = path_costs(hops, d2, 1)
    assert how["tie_bits"] == 3 and c.max() <= 2 ** 31 - 1  # 4096 * 32768 * 2^b = 2^(27 + b): b = 4 gives 2^31, one too many
    for bad in (dict(power=3), dict(power=True), dict(power=1.5)):
        with pytest.raises(ValueError):
            path_costs(hops[:4, :4], d2[:4, :4], **bad)
    with pytest.raises(ValueError):
        path_costs(hops[:4, :3], d2[:4, :3])
    with pytest.raises(ValueError):
        path_costs(hops[:4, :4].astype(np.float64), d2[:4, :4])
    with pytest.raises(ValueError):
        path_costs(hops[:4, :4], -d2[:4, :4] - 1.0)


def test_the_abi_is_additive():
    from path_planning import _hip

    header = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert _hip.ABI_VERSION == 7 == int(re.search(r"#define SCP_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define SCP_ASSIGN_MAX_COST (\d+)", header).group(1)) == _hip.ASSIGN_MAX_COST == P.MAX_COST
    for name in ("scp_lattice_distances", "scp_assign_costs"):
        assert name in _hip.EXPORTS and name in _hip.PROTOTYPES
        assert re.search(rf"^int {name}\(scp_ctx\* ctx,", header, flags=re.M), name
    assert len(_hip.PROTOTYPES["scp_lattice_distances"][1]) == 13 and len(_hip.PROTOTYPES["scp_assign_costs"][1]) == 8
    lib = _hip.load_library()
    assert hasattr(lib, "scp_lattice_distances") and hasattr(lib, "scp_assign_costs") and lib.scp_abi_version() == 7
    import inspect

    from path_planning.scenarios import assignment
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.assign_goals)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("min_sep", None), ("method", "auto"), ("cost", "line"), ("stride", None), ("clearance", 0), ("power", 2),
        ("allow_unreachable", False)]
    sig = inspect.signature(assignment.assign_goals_costs)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [("cost", inspect.Parameter.empty), ("device", 0),
                                                                    ("max_rounds_per_phase", 0)]


def test_cli_flags_and_the_report_line():
    from path_planning.cli import compute_trajectories as ct
    from path_planning.cli import compute_trajectories_batch as cb
    from path_planning.scenarios.assignment import describe, hop_totals

    parser = ct.build_parser()
    assert parser.parse_args([]).assign_cost == "line" and cb.build_parser().parse_args([]).assign_cost == "line"
    args = parser.parse_args(["--assign-goals", "--assign-cost", "path", "--obstacle-discs", "5,5,1", "--corridor-stride", "2",
                              "--corridor-clearance", "1"])
    assert args.assign_cost == "path" and ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]  # (no --corridor-search needed)
    for argv in (["--assign-cost", "path", "--obstacle-discs", "5,5,1"], ["--assign-goals", "--assign-cost", "path"],
                 ["--assign-goals", "--assign-cost", "path", "--obstacle-discs", "5,5,1", "--corridor-shorten"],
                 ["--assign-goals", "--assign-cost", "line", "--obstacle-discs", "5,5,1", "--corridor-stride", "2"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    with pytest.raises(SystemExit):
        parser.parse_args(["--assign-cost", "hops"])
    with pytest.raises(SystemExit):  # the batch scenarios have no map
        cb.main(["--assign-goals", "--assign-cost", "path"])

    hops = np.array([[3, 0xFFFF, 9], [4, 2, 0xFFFF], [1, 7, 5]])
    assert hop_totals(hops) == {"sum": 10, "max": 5, "n_unreachable": 0}
    assert hop_totals(hops, [2, 0, 1]) == {"sum": 20, "max": 9, "n_unreachable": 0}
    assert hop_totals(hops, [1, 2, 0]) == {"sum": 1, "max": 1, "n_unreachable": 2}
    line = {"min_approach": 0.5, "arg_i": 0, "arg_j": 1, "n_close": 0, "n_opposed": 2}
    info = {"quantum": 1.0, "status": 0, "phases": 3, "rounds": 11, "line_before": line, "line_after": dict(line, n_opposed=0),
            "hops_identity": {"sum": 80, "max": 17}, "hops_assigned": {"sum": 78, "max": 13}, "n_unreachable_identity": 1,
            "n_unreachable_assigned": 0, "distances_ms": 0.25, "assign_ms": 0.5}
    text = describe(info)
    assert text.startswith("Goal assignment by path length: 80 -> 78 lattice moves in all (longest 17 -> 13), pairs without a "
                           "path 1 -> 0,") and "opposed pairs 2 -> 0 (3 phases, 11 rounds, 0.750 ms)" in text
