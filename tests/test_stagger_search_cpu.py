"""CPU tests of the order search of the staggered starts: the declaration of scp_schedule_starts_batch, the two numpy functions
that make candidate orders, and the reference of tests/stagger_search_ref.py on the inputs the GPU tests rely on."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stagger_ref as st  # noqa: E402
import stagger_search_ref as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_batch_call():
    from path_planning import _hip

    header = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert re.search(r"\bint scp_schedule_starts_batch\(scp_ctx\* ctx, int N, int max_lag, const uint64_t\* mask", header)
    assert re.search(r"#define SCP_ABI_VERSION 7\b", header)
    assert "scp_schedule_starts_batch" in _hip.EXPORTS and _hip.ABI_VERSION == 7
    assert _hip.SCHEDULE_OBJECTIVES == {"makespan": 0, "total": 1} and _hip.SCHEDULE_MAX_BATCH == 65535
    assert _hip.START_SCHEDULE_STATS_DTYPE.itemsize == 48 == __import__("ctypes").sizeof(_hip.StartScheduleStats)


@pytest.mark.parametrize("N,B", [(1, 1), (1, 3), (2, 2), (7, 1), (33, 36), (130, 5)])
def test_candidate_orders(N, B):
    from path_planning.solvers.stagger import candidate_orders

    got = candidate_orders(N, B, np.random.default_rng(3))
    assert got.shape == (B, N) and got.dtype == np.int32
    assert all(sorted(row.tolist()) == list(range(N)) for row in got)
    assert got[0].tolist() == list(range(N))
    if B >= 2:
        assert got[1].tolist() == list(range(N))[::-1]
    rng = np.random.default_rng(3)  # rows 2 ... are the generator's permutations, drawn in sequence
    assert all(got[b].tolist() == rng.permutation(N).tolist() for b in range(2, B))
    assert candidate_orders(N, B, np.random.default_rng(3)).tobytes() == got.tobytes()
    base = np.random.default_rng(N).permutation(N)
    based = candidate_orders(N, B, np.random.default_rng(3), base=base)
    assert based[0].tolist() == base.tolist() and based[2:].tobytes() == got[2:].tobytes()
    if B >= 2:
        assert based[1].tolist() == base[::-1].tolist()


def test_refined_orders_by_hand():
    from path_planning.solvers.stagger import refined_orders

    #          vehicle  0  1   2  3  4   5
    delays = np.array([2, -1, 0, 2, 0, -1])
    best = [3, 5, 0, 2, 1, 4]  # positions: 3 -> 0, 5 -> 1, 0 -> 2, 2 -> 3, 1 -> 4, 4 -> 5
    got = refined_orders(best, delays, 9, np.random.default_rng(5))
    assert got.shape == (9, 6) and got.dtype == np.int32
    assert got[0].tolist() == best
    assert got[1].tolist() == [5, 1, 3, 0, 2, 4]  # the unplaced by position, then the placed by position
    assert got[2].tolist() == [5, 1, 2, 4, 3, 0]  # ... then the placed by ascending delay, ties by position
    assert got[3].tolist() == [3, 0, 2, 4, 5, 1]  # the placed by descending delay, ties by position, then the unplaced
    rng = np.random.default_rng(5)
    for b in range(4, 9):  # max(1, 6 // 16) = 1 transposition each
        i, j = rng.integers(0, 6, 2)
        want = list(best)
        want[i], want[j] = want[j], want[i]
        assert got[b].tolist() == want
    assert refined_orders(best, delays, 9, np.random.default_rng(5)).tobytes() == got.tobytes()
    for B in (1, 2, 3):
        assert refined_orders(best, delays, B, np.random.default_rng(5)).tolist() == got[:B].tolist()


@pytest.mark.parametrize("N,B", [(1, 6), (33, 12), (130, 7)])
def test_refined_orders_are_permutations(N, B):
    from path_planning.solvers.stagger import refined_orders

    rng = np.random.default_rng(N)
    best = rng.permutation(N)
    delays = rng.integers(-1, 4, N)
    got = refined_orders(best, delays, B, np.random.default_rng(1))
    assert got.shape == (B, N) and all(sorted(row.tolist()) == list(range(N)) for row in got)
    assert got[0].tolist() == best.tolist()
    swaps = max(1, N // 16)
    assert all((got[b] != best).sum() <= 2 * swaps for b in range(4, B))


def test_best_of_is_the_lexicographic_minimum():
    mk = lambda u, m, t: {"n_unplaced": u, "max_delay": m, "total_delay": t}  # noqa: E731
    stats = [mk(2, 1, 1), mk(1, 5, 9), mk(1, 4, 12), mk(1, 4, 12), mk(1, 6, 8)]
    assert ss.best_of(stats, "makespan") == 2 and ss.best_of(stats, "total") == 4
    assert ss.best_of([mk(0, 0, 0)] * 3, "makespan") == 0  # ties go to the lowest index
    with pytest.raises(ValueError):
        ss.key(stats[0], "shortest", 0)


def test_reference_search_beats_the_index_order():
    """the condition on the inputs of the GPU test: the search has something to find"""
    from path_planning.solvers.stagger import candidate_orders

    m = st.random_masks(33, 5, 0.10, 1)
    orders = candidate_orders(33, 36, np.random.default_rng(101))
    _, stats = ss.schedule_all(m, 5, orders)
    for objective in ss.OBJECTIVES:
        b = ss.best_of(stats, objective)
        assert b != 0 and ss.key(stats[b], objective, 0) < ss.key(stats[0], objective, 0)
    assert ss.key(stats[0], "makespan", 0)[:3] == (11, 5, 26)
    assert ss.key(stats[ss.best_of(stats, "makespan")], "makespan", 0)[:3] <= (5, 5, 41)


def test_reference_objectives_can_disagree():
    from path_planning.solvers.stagger import candidate_orders

    m = st.random_masks(12, 6, 0.2, 8)
    orders = candidate_orders(12, 8, np.random.default_rng(8))
    _, stats = ss.schedule_all(m, 6, orders)
    a, b = ss.best_of(stats, "makespan"), ss.best_of(stats, "total")
    assert a != b and stats[a]["n_unplaced"] == stats[b]["n_unplaced"]
    assert stats[a]["max_delay"] < stats[b]["max_delay"] and stats[a]["total_delay"] > stats[b]["total_delay"]


def test_schedule_key():
    from path_planning.solvers.stagger import schedule_key

    assert schedule_key(np.int32(3), np.int32(2), np.int64(7), "makespan") == (3, 2, 7)
    assert schedule_key(3, 2, 7, "total") == (3, 7, 2)


def test_cli_search_flags_need_stagger_starts():
    from path_planning.cli import compute_trajectories as ct
    from path_planning.cli import compute_trajectories_batch as ctb

    for flag in (["--stagger-search", "4"], ["--stagger-rounds", "2"], ["--stagger-seed", "1"], ["--stagger-objective", "total"]):
        for cli in (ct, ctb):
            with pytest.raises(SystemExit) as err:
                cli.main(flag)
            assert err.value.code == 2
