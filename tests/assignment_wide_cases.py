"""Cases of the goal assignment beyond 4096 vehicles (scp_assign_goals_wide), the once-per-process cache of their reference
(tests/assignment_ref.py: minutes of CPU time would be paid per test otherwise), and ``certify``: the optimality check for
sizes the reference cannot reach, because it holds N^2 int64."""
import math

import numpy as np

import assignment_ref as R

PRICE_BOUND_FACTOR = 52  # include/scp_hip.h: prices < 52 (N + 1) 2^31
JITTERED_4100_DISPLACED = 1024  # of jittered_grid(4100, 7, swaps=1024): the permutation of the 1024 goals has no fixed point


def price_bound(N):
    return PRICE_BOUND_FACTOR * (N + 1) * 2 ** 31


def jittered_grid(N, seed, swaps):
    """grid points 2 m apart; starts and goals are the points jittered by +-0.2 m, and ``swaps`` of the goals are permuted
    among themselves: the optimum sends every vehicle to the goal at its own grid point, whoever holds it"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    k = np.arange(N)
    pts = np.stack([k // side, k % side], 1).astype(np.float64) * 2.0
    start = pts + rng.uniform(-0.2, 0.2, (N, 2))
    goal = pts + rng.uniform(-0.2, 0.2, (N, 2))
    idx = rng.choice(N, swaps, replace=False)
    goal[idx] = goal[idx[rng.permutation(swaps)]]
    return start, goal


def displaced(start, goal):
    """vehicles of a jittered grid whose given goal is not the one at their own grid point"""
    return int((np.abs(goal - start).max(1) > 1.0).sum())


def wide_cases():
    """name -> (start, goal), all above the one-workgroup limit of 4096"""
    return {
        "jittered-grid-4100": jittered_grid(4100, 7, swaps=1024),  # 22 rounds, every one with thousands of bidders
        "uniform-3d-4100": R.uniform(4100, 3, 5),                  # ~27 000 rounds of both kinds, many switches
        "lattice-4225": R.lattice_permutation(4225),               # exact ties at scale
    }


_CASES = {}
_RESULTS = {}


def wide_case(name):
    if name not in _CASES:
        _CASES[name] = wide_cases()[name]
    return _CASES[name]


def wide_reference(name):
    """the auction of a case of wide_cases(), computed once per process and never modified"""
    if name not in _RESULTS:
        _RESULTS[name] = R.auction(*wide_case(name))
    return _RESULTS[name]


def certify(start, goal, goal_of, prices, block_elems=1 << 23):
    """True iff goal_of is a permutation and a[i, goal_of[i]] - p[goal_of[i]] >= max_j (a_ij - p_j) - 1 for every i, with
    a = -(N + 1) c and c recomputed by the rule's arithmetic (every product and sum rounded on its own, ldexp, floor), row
    block by row block on torch tensors (of the device start is on).  The costs are integers scaled by N + 1, so this
    1-complementary slackness proves that goal_of is exactly optimal for c."""
    import torch

    start = torch.as_tensor(start, dtype=torch.float64)
    dev = start.device
    goal = torch.as_tensor(goal, dtype=torch.float64).to(dev)
    goal_of = torch.as_tensor(goal_of).to(device=dev, dtype=torch.int64).reshape(-1)
    prices = torch.as_tensor(prices).to(device=dev, dtype=torch.int64).reshape(-1)
    N, D = start.shape
    if sorted(goal_of.cpu().tolist()) != list(range(N)):
        return False
    pts = torch.cat([start, goal])
    span = (pts.max(0).values - pts.min(0).values).cpu().tolist()
    Bd = span[0] * span[0]
    for d in range(1, D):
        Bd = Bd + span[d] * span[d]
    s = 31 - math.frexp(Bd)[1] if Bd > 0 else 0
    s1 = torch.tensor(s // 2, device=dev)
    s2 = torch.tensor(s - s // 2, device=dev)
    rows = max(1, block_elems // N)
    for r0 in range(0, N, rows):
        a_pts = start[r0:r0 + rows]
        diff = a_pts[:, None, 0] - goal[None, :, 0]
        d2 = diff * diff
        for d in range(1, D):
            diff = a_pts[:, None, d] - goal[None, :, d]
            d2 = d2 + diff * diff
        c = torch.floor(torch.ldexp(torch.ldexp(d2, s1), s2)).to(torch.int64)  # (two exact steps: 2^s alone may overflow)
        v = -(N + 1) * c - prices[None, :]
        mine = v.gather(1, goal_of[r0:r0 + rows, None])[:, 0]
        if not bool((mine >= v.max(1).values - 1).all()):
            return False
    return True
