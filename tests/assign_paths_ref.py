"""numpy / int64 restatement of the two rules behind goal assignment by path length (include/scp_hip.h): the hop counts of
scp_lattice_distances, built on the lattice helpers of tests/reference_path_ref.py, and the auction of scp_assign_costs -- the
rule of tests/assignment_ref.py with its costs read from a matrix.  Integers only: the GPU tests compare byte for byte."""
import numpy as np

import corridor_ref as cr
import reference_path_ref as rr

UNREACHED = rr.UNREACHED
MAX_COST = 2 ** 31 - 1


# ---- scp_lattice_distances -----------------------------------------------------------------------------------------------------
def passable_node(D, origin, cell, dims, L, stride, edges, p):
    """the node of a point, or -1: off the grid, beyond the lattice, or on a block that is not passable"""
    node = rr.point_node(D, origin, cell, dims, L, stride, p)
    return node if node >= 0 and int(edges[node]) >> rr.SELF & 1 else -1


def hop_matrix(D, origin, cell, occ, stride, clearance, src, dst):
    """-> (hops (n_src, n_dst) uint16, src_node (n_src,) int32, dst_node (n_dst,) int32, dist (n_src, nodes) uint16: the
    COMPLETE breadth-first field of every source, all 0xFFFF for a source without a node, edges uint32 (nodes,))"""
    nz, ny, nx = occ.shape
    dims = (nx, ny, nz)
    L = rr.lattice(D, dims, stride)
    edges = rr.lattice_edges(D, cr.summed_table(occ), stride, clearance)
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    src_node = np.array([passable_node(D, origin, cell, dims, L, stride, edges, p) for p in src], dtype=np.int32)
    dst_node = np.array([passable_node(D, origin, cell, dims, L, stride, edges, p) for p in dst], dtype=np.int32)
    dist = np.full((len(src), edges.size), UNREACHED, dtype=np.uint16)
    hops = np.full((len(src), len(dst)), UNREACHED, dtype=np.uint16)
    fields = {}  # (sources often share a node: one search each)
    for a, node in enumerate(src_node):
        if node < 0:
            continue
        if int(node) not in fields:
            fields[int(node)] = rr.distances(L, edges, int(node))
        dist[a] = fields[int(node)]
        ok = dst_node >= 0
        hops[a, ok] = dist[a, dst_node[ok]]
    return hops, src_node, dst_node, dist, edges


# ---- scp_assign_costs ----------------------------------------------------------------------------------------------------------
def auction_costs(c, max_rounds_per_phase=0, top=None):
    """The Jacobi forward auction with eps-scaling on the matrix c (N, N), c[i][j] the cost of person i for goal j, whole
    numbers in [0, 2^31 - 1].  top None: max c, the rule of scp_assign_costs; given: the value eps_0 is made from (the
    quantisation of scp_assign_goals uses floor(Bd 2^s), which its largest cost need not attain).  Returns a dict: goal_of,
    prices (int64), cost_q, cost_q_identity, quantum = 1.0, rounds, bids, phases, status, and longest_phase / eps_last."""
    c = np.asarray(c)
    assert c.ndim == 2 and c.shape[0] == c.shape[1] and c.dtype.kind in "iu"
    c = c.astype(np.int64)
    assert c.min() >= 0 and c.max() <= MAX_COST
    N = c.shape[0]
    top = int(c.max()) if top is None else int(top)
    guard = int(max_rounds_per_phase) if max_rounds_per_phase > 0 else 256 * N + 4096
    a = -(N + 1) * c
    p = np.zeros(N, dtype=np.int64)
    goal_of = np.arange(N, dtype=np.int64)
    rounds = bids = phases = status = longest = 0
    eps = max(1, ((N + 1) * top) // 2)
    while N >= 2:  # phases: eps falls by 4 until it is 1
        owner = np.full(N, -1, dtype=np.int64)
        goal_of = np.full(N, -1, dtype=np.int64)
        phases += 1
        r = 0
        while True:  # rounds: every unassigned person bids
            U = np.flatnonzero(goal_of < 0)
            if U.size == 0:
                break
            if r == guard:
                status = 1
                break
            r += 1
            bids += int(U.size)
            v = a[U] - p[None, :]
            j1 = v.argmax(1)  # the first maximum: the lowest j on ties
            rows = np.arange(U.size)
            w1 = v[rows, j1]
            v[rows, j1] = np.iinfo(np.int64).min
            w2 = v.max(1)
            bid = p[j1] + (w1 - w2) + eps
            for j in np.unique(j1):  # the highest bid per goal, the lowest person on ties
                k = np.flatnonzero(j1 == j)
                k = k[bid[k] == bid[k].max()][0]  # (U ascends: the first is the lowest person)
                if owner[j] >= 0:
                    goal_of[owner[j]] = -1
                owner[j] = U[k]
                goal_of[U[k]] = j
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
                quantum=1.0, rounds=rounds, bids=bids, phases=phases, status=status, longest_phase=longest, eps_last=eps)


# ---- the matrices the CPU and the GPU tests share -------------------------------------------------------------------------------
def random_matrix(N, seed, high=1000, sentinel_rows=0):
    """whole numbers below `high`; the first `sentinel_rows` rows reach only goals 0 .. N/2 and pay the sentinel
    N * (largest other entry) + 1 elsewhere, as path_costs writes unreachable pairs"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, high, (N, N), dtype=np.int64)
    if sentinel_rows:
        c[:sentinel_rows, N // 2 + 1:] = N * int(c.max()) + 1
    return c


def gpu_matrices():
    """name -> (N, N) int64"""
    out = {f"random-{N}": random_matrix(N, 500 + N) for N in (1, 2, 3, 63, 64, 65, 130)}
    out["all-equal-17"] = np.full((17, 17), 7, dtype=np.int64)
    out["all-zero-5"] = np.zeros((5, 5), dtype=np.int64)
    out["sentinel-rows-40"] = random_matrix(40, 41, sentinel_rows=6)
    c = random_matrix(9, 9, high=2 ** 20)
    c[2, 5] = c[7, 7] = MAX_COST
    out["max-cost-9"] = c
    return out


_RESULTS = {}


def reference(name):
    """the auction of a matrix of gpu_matrices(), computed once"""
    if name not in _RESULTS:
        _RESULTS[name] = auction_costs(gpu_matrices()[name])
    return _RESULTS[name]
