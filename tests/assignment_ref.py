"""numpy / int64 restatement of the goal-assignment rule and of the straight-line check (include/scp_hip.h), the cases
the CPU and GPU tests share, and a brute-force optimum for small N.  The GPU tests compare the kernels against this bit for
bit; the CPU tests check its promises (exact optimality on the quantised costs, eps-complementary slackness)."""
import itertools

import numpy as np


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def quantise(start, goal):
    """-> (c (N, N) int64, s, top = floor(Bd 2^s)): costs of the rule for one scenario; every product rounded, d ascending"""
    start, goal = np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    pts = np.concatenate([start, goal])
    span = pts.max(0) - pts.min(0)
    Bd = span[0] * span[0]
    for d in range(1, start.shape[1]):
        Bd = Bd + span[d] * span[d]
    s, top = 0, 0
    if Bd > 0:
        _, e = np.frexp(Bd)
        s = 31 - int(e)
        top = int(np.floor(np.ldexp(Bd, s)))
    diff = start[:, None, :] - goal[None, :, :]
    d2 = diff[..., 0] * diff[..., 0]
    for d in range(1, start.shape[1]):
        d2 = d2 + diff[..., d] * diff[..., d]
    c = np.floor(np.ldexp(d2, s)).astype(np.int64)
    assert c.max() < 2 ** 31
    return c, s, top


def auction(start, goal, max_rounds_per_phase=0):
    """The Jacobi forward auction with eps-scaling of the rule.  Returns a dict: goal_of, prices (int64), cost_q,
    cost_q_identity, quantum, rounds, bids, phases, status, and longest_phase / eps_last for the tests."""
    c, s, top = quantise(start, goal)
    N = c.shape[0]
    guard = int(max_rounds_per_phase) if max_rounds_per_phase > 0 else 256 * N + 4096
    a = -(N + 1) * c
    p = np.zeros(N, dtype=np.int64)
    goal_of = np.arange(N, dtype=np.int64)
    rounds = bids = phases = status = longest = 0
    eps = max(1, ((N + 1) * top) // 2)
    while N >= 2:
        owner = np.full(N, -1, dtype=np.int64)
        goal_of = np.full(N, -1, dtype=np.int64)
        phases += 1
        r = 0
        while True:
            U = np.flatnonzero(goal_of < 0)
            if U.size == 0:
                break
            if r == guard:
                status = 1
                break
            r += 1
            bids += int(U.size)
            v = a[U] - p[None, :]
            j1 = v.argmax(1)  # the first maximum: lowest j on ties
            rows = np.arange(U.size)
            w1 = v[rows, j1]
            v[rows, j1] = np.iinfo(np.int64).min
            w2 = v.max(1)
            bid = p[j1] + (w1 - w2) + eps
            order = np.lexsort((U, -bid, j1))  # by goal, then highest bid, then lowest person
            first = np.ones(order.size, dtype=bool)
            first[1:] = j1[order][1:] != j1[order][:-1]
            win = order[first]
            for k in win:
                j, i = int(j1[k]), int(U[k])
                if owner[j] >= 0:
                    goal_of[owner[j]] = -1
                owner[j] = i
                goal_of[i] = j
                p[j] = bid[k]
        rounds += r
        longest = max(longest, r)
        if status or eps == 1:
            break
        eps = max(1, eps // 4)
    if status:
        goal_of = np.arange(N, dtype=np.int64)
    idx = np.arange(N)
    return dict(goal_of=goal_of, prices=p, cost_q=int(c[idx, goal_of].sum()), cost_q_identity=int(c[idx, idx].sum()),
                quantum=float(np.ldexp(1.0, -s)), rounds=rounds, bids=bids, phases=phases, status=status,
                longest_phase=longest, eps_last=eps, c=c)


def brute_force(c):
    """smallest sum_i c[i][perm[i]] over all permutations (N <= 7)"""
    N = c.shape[0]
    idx = np.arange(N)
    return min(int(c[idx, list(perm)].sum()) for perm in itertools.permutations(range(N)))


def line_check(start, goal, goal_of=None, min_sep=0.0):
    """The straight-line check: min_approach, arg_i, arg_j, n_close, n_opposed (z terms last, every product rounded)"""
    start, goal = np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    N, D = start.shape
    if N == 1:
        return dict(min_approach=np.inf, arg_i=-1, arg_j=-1, n_close=0, n_opposed=0)
    g = goal if goal_of is None else goal[np.asarray(goal_of)]
    i, j = np.triu_indices(N, 1)  # lexicographic: the first minimum is the lowest (i, j)
    r0 = start[i] - start[j]
    dg = g[i] - g[j]
    dr = dg - r0
    den = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]
    num = r0[:, 0] * dr[:, 0] + r0[:, 1] * dr[:, 1]
    dot = r0[:, 0] * dg[:, 0] + r0[:, 1] * dg[:, 1]
    if D == 3:
        den = den + dr[:, 2] * dr[:, 2]
        num = num + r0[:, 2] * dr[:, 2]
        dot = dot + r0[:, 2] * dg[:, 2]
    s = np.clip(-num / np.where(den > 0, den, 1.0), 0.0, 1.0)
    cc = r0 + s[:, None] * dr
    d2 = cc[:, 0] * cc[:, 0] + cc[:, 1] * cc[:, 1]
    if D == 3:
        d2 = d2 + cc[:, 2] * cc[:, 2]
    k = int(np.argmin(d2))
    return dict(min_approach=float(np.sqrt(d2[k])), arg_i=int(i[k]), arg_j=int(j[k]),
                n_close=int((d2 < min_sep * min_sep).sum()), n_opposed=int((dot < 0).sum()))


# ---- the cases of the GPU test list (the CPU tests check the guard on the same ones) ------------------------------------------
def uniform(N, D, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 50.0, (N, D)), rng.uniform(0.0, 50.0, (N, D))


def lattice_permutation(N, seed=3):
    """integer lattice points, the goals a permutation of the starts: many exact ties"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    pts = np.array([(k // side, k % side) for k in range(N)], dtype=np.float64) * 2.0
    return pts, pts[rng.permutation(N)]


def reversed_lines(N=32):
    x = 2.0 * np.arange(N, dtype=np.float64)
    return np.stack([x, np.zeros(N)], 1), np.stack([x[::-1], np.full(N, 10.0)], 1)


def identical_goals(N=64, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 20.0, (N, 2)), np.tile(np.array([[7.0, 5.0]]), (N, 1))


def identical_points(N=9, D=2):
    return np.full((N, D), 1.25), np.full((N, D), 1.25)


def optimal_identity(N=40):
    """every start next to its own goal and far from all others: the identity is the optimum"""
    rng = np.random.default_rng(11)
    side = int(np.ceil(np.sqrt(N)))
    pts = np.array([(k // side, k % side) for k in range(N)], dtype=np.float64) * 10.0
    return pts, pts + rng.uniform(-1.0, 1.0, (N, 2))


def gpu_cases():
    """name -> (start, goal)"""
    cases = {}
    for D in (2, 3):
        for N in (1, 2, 3, 63, 64, 65, 130, 300):
            cases[f"uniform-{D}d-{N}"] = uniform(N, D, 1000 * D + N)
    cases["lattice-1100"] = lattice_permutation(1100)
    cases["reversed-lines-32"] = reversed_lines(32)
    cases["identical-goals-64"] = identical_goals(64)
    cases["identical-points"] = identical_points()
    cases["optimal-identity-40"] = optimal_identity()
    return cases


_RESULTS = {}


def reference(name):
    """the auction of a case of gpu_cases(), computed once"""
    if name not in _RESULTS:
        _RESULTS[name] = auction(*gpu_cases()[name])
    return _RESULTS[name]
