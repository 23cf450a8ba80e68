"""The checks behind the GPU tests of scp_assign_goals_wide, without a GPU: ``certify`` accepts the reference's output and
rejects a damaged one, the price bound the header states holds on the reference's prices, the jittered grid is what the
tests say it is, and the function is declared and bound."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assignment_ref as R  # noqa: E402
import assignment_wide_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CERTIFY_CASES = ("uniform-2d-65", "uniform-3d-300", "lattice-1100")


@pytest.mark.parametrize("name", CERTIFY_CASES)
def test_certify_accepts_the_auction_and_rejects_damage(name):
    start, goal = R.gpu_cases()[name]
    ref = R.reference(name)
    N = len(start)
    assert W.certify(start, goal, ref["goal_of"], ref["prices"])
    assert W.certify(start, goal, ref["goal_of"], ref["prices"], block_elems=7 * N)  # (several row blocks, a ragged last one)
    # two goals swapped: still a permutation, no longer optimal -- unless the swap costs nothing, so take a pair it costs
    c, g = ref["c"], ref["goal_of"]
    i, j = next((i, j) for i in range(N) for j in range(i + 1, N) if c[i, g[j]] + c[j, g[i]] > c[i, g[i]] + c[j, g[j]])
    swapped = g.copy()
    swapped[[i, j]] = g[[j, i]]
    assert not W.certify(start, goal, swapped, ref["prices"])
    twice = g.copy()
    twice[1] = twice[0]
    assert not W.certify(start, goal, twice, ref["prices"])  # not a permutation
    # One price lowered.  Which one: the second choice of the person whose own goal beats it by the least (`slack`).  A
    # discount of more than slack + 1 on that goal must be noticed, a smaller one on any goal must not: 2 (N + 1) is noticed
    # on the uniform cases, whose last bidders are left 1 below their second choice, and not on the lattice, where a phase is
    # a single round that raises everybody's second choice too (the costs are scaled by N + 1, the slack is of that order).
    v = -(N + 1) * c - ref["prices"][None, :]
    mine = v[np.arange(N), g].copy()
    v[np.arange(N), g] = np.iinfo(np.int64).min
    slack = mine - v.max(1)
    i = int(np.argmin(slack))
    k = int(v[i].argmax())
    assert slack[i] >= -1
    if name.startswith("uniform"):
        assert slack[i] == -1
    for discount in (2 * (N + 1), int(slack[i]) + 2, int(slack[i]) + 1):
        lowered = ref["prices"].copy()
        lowered[k] -= discount
        assert W.certify(start, goal, g, lowered) == (discount <= slack[i] + 1), (discount, slack[i])


def test_price_bound_of_the_header():
    names = sorted(R.gpu_cases())
    for name in names:
        ref = R.reference(name)
        N = len(ref["prices"])
        assert 0 <= int(ref["prices"].min()) and int(ref["prices"].max()) < W.price_bound(N), (name, ref["prices"].max())
        assert ref["phases"] <= 25, (name, ref["phases"])
    assert W.price_bound(65536) < 2 ** 53 and W.price_bound(4096) < 2 ** 49
    text = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert "prices <= 50 C + (4/3) C + 50 < 52 (N + 1) 2^31" in text and "1 <= N <= 65536" in text


@pytest.mark.parametrize("name", sorted(W.wide_cases()))
def test_price_bound_above_the_old_limit(name):
    ref = W.wide_reference(name)
    N = len(ref["prices"])
    assert N > 4096 and ref["status"] == 0
    assert 0 <= int(ref["prices"].min()) and int(ref["prices"].max()) < W.price_bound(N), (name, ref["prices"].max())
    assert ref["phases"] <= 25, (name, ref["phases"])
    start, goal = W.wide_case(name)
    assert W.certify(start, goal, ref["goal_of"], ref["prices"])


def test_jittered_grid_is_deterministic_and_swaps_what_it_says():
    a, b = W.jittered_grid(4100, 7, swaps=1024), W.jittered_grid(4100, 7, swaps=1024)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert W.jittered_grid(4100, 8, swaps=1024)[0].tobytes() != a[0].tobytes()
    assert W.displaced(*a) == W.JITTERED_4100_DISPLACED
    assert W.displaced(*W.jittered_grid(300, 1, swaps=0)) == 0
    # the reference re-pairs exactly those vehicles: everybody ends at the goal of its own grid point
    ref = W.wide_reference("jittered-grid-4100")
    start, goal = W.wide_case("jittered-grid-4100")
    assert int((ref["goal_of"] != np.arange(4100)).sum()) == W.JITTERED_4100_DISPLACED
    assert W.displaced(start, goal[ref["goal_of"]]) == 0


def test_the_function_is_declared_and_bound():
    from path_planning import _hip

    text = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert re.search(r"\bint scp_assign_goals_wide\(scp_ctx\* ctx, int B, int N, int D,", text)
    assert "scp_assign_goals_wide" in _hip.EXPORTS and "scp_assign_goals" in _hip.EXPORTS
    assert "#define SCP_ABI_VERSION 7" in text and _hip.ABI_VERSION == 7
    assert hasattr(_hip.Context, "assign_goals_wide")
