"""numpy / plain-Python restatement of the rules of include/scp_hip.h, "static obstacles: weighted search": node penalties
from the gap-1 distance field (with the exact integer square root), the cost field by Dijkstra's algorithm (heapq), the path
walk, the statuses and the cost matrix.  Integers exactly; the reference points are those of tests/reference_path_ref.py (bit
for bit).  Lattice, edge masks and the node of a point come from that file too."""
import heapq
import math

import numpy as np

import assign_paths_ref as ar
import reference_path_ref as rr

UNREACHED = 0xFFFFFFFF
W = (0, 70, 99, 121)           # move weights by |dx| + |dy| + |dz|
MAX_PRODUCT = 32768            # SCP_PENALTY_MAX_PRODUCT
PATH_INFO_DTYPE = rr.PATH_INFO_DTYPE


def move_len(n):
    return sum(abs(v) for v in rr.direction(n))


def block_minimum(D, field, stride):
    """field [nz][ny][nx] uint32 -> m uint32 [nodes]: the minimum over the cells of every node's block"""
    nz, ny, nx = field.shape
    L = rr.lattice(D, (nx, ny, nz), stride)
    sz = stride if D == 3 else 1
    f = np.asarray(field, dtype=np.uint32)[:L[2] * sz, :L[1] * stride, :L[0] * stride]
    return f.reshape(L[2], sz, L[1], stride, L[0], stride).min(axis=(1, 3, 5)).reshape(-1)


def penalties(D, field, stride, prefer, weight):
    """-> (pen uint32 [nodes], rho [nodes] as Python-int array); ValueError where the call is not supported"""
    if prefer < 0 or weight < 0 or prefer * weight > MAX_PRODUCT:
        raise ValueError(f"weight * prefer = {weight * prefer} is not supported")
    m = block_minimum(D, field, stride)
    rho = np.array([math.isqrt(int(v)) for v in m], dtype=np.int64)
    return (weight * (prefer - np.minimum(rho, prefer))).astype(np.uint32), rho


def edge_cost(pen, u, v, n):
    return 2 * W[move_len(n)] + (0 if pen is None else int(pen[u]) + int(pen[v]))


def _neighbours(L, edges, node):
    """(direction code, neighbour) over the set edge bits of a node, in direction order"""
    mask = int(edges[node])
    return [(n, rr.neighbour(L, node, n)) for n in rr.DIRECTION_ORDER if mask >> n & 1]


def cost_field(L, edges, pen, origin):
    """the complete cost field of `origin` (a passable node): uint32 [nodes], UNREACHED where no walk leads"""
    best = {origin: 0}
    done = set()
    heap = [(0, origin)]
    while heap:
        c, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u)
        for n, v in _neighbours(L, edges, u):
            via = c + edge_cost(pen, u, v, n)
            if via < best.get(v, UNREACHED):
                best[v] = via
                heapq.heappush(heap, (via, v))
    out = np.full(edges.size, UNREACHED, dtype=np.uint32)
    assert max(best.values()) < UNREACHED
    out[list(best)] = list(best.values())
    return out


def walk(L, edges, pen, cost, start, goal, max_path):
    """the path from `start`: the first neighbour in direction order over a set edge bit with cost[nb] + w == cost[node]; None
    if the goal has not been reached after max_path nodes"""
    path, node = [], start
    while True:
        if len(path) == max_path:
            return None
        path.append(node)
        if node == goal:
            return path
        for n, nb in _neighbours(L, edges, node):
            if cost[nb] != UNREACHED and int(cost[nb]) + edge_cost(pen, node, nb, n) == int(cost[node]):
                node = nb
                break
        else:
            raise AssertionError("a reached node without a neighbour that explains its cost")


def reference_paths_weighted(D, origin, cell, sat, stride, edges, pen, p0, pf, K, max_path, ref):
    """-> (ref (N, K + 1, D) with the rows of the found vehicles replaced, path (N, max_path) int32, info PATH_INFO_DTYPE (N,),
    path_cost (N,) uint32, cost (N, nodes) uint32, n_failed)"""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    L = rr.lattice(D, dims, stride)
    nodes = L[0] * L[1] * L[2]
    assert edges.shape == (nodes,) and 1 <= max_path <= nodes and (pen is None or pen.shape == (nodes,))
    p0, pf = np.asarray(p0, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    N = p0.shape[0]
    ref = np.array(ref, dtype=np.float64, copy=True)
    path = np.full((N, max_path), -1, dtype=np.int32)
    info = np.zeros(N, dtype=PATH_INFO_DTYPE)
    cost = np.full((N, nodes), UNREACHED, dtype=np.uint32)
    path_cost = np.full(N, UNREACHED, dtype=np.uint32)
    n_failed = 0
    by_goal = {}
    for i in range(N):
        status, goal, m = 0, -1, 0
        start = rr.point_node(D, origin, cell, dims, L, stride, p0[i])
        if start < 0 or not int(edges[start]) >> rr.SELF & 1:
            status = 1
        if status == 0:
            goal = rr.point_node(D, origin, cell, dims, L, stride, pf[i])
            if goal < 0 or not int(edges[goal]) >> rr.SELF & 1:
                status = 2
        if status == 0:
            if goal not in by_goal:
                by_goal[goal] = cost_field(L, edges, pen, goal)
            cost[i] = by_goal[goal]
            if cost[i, start] == UNREACHED:
                status = 3
            else:
                nodes_i = walk(L, edges, pen, cost[i], start, goal, max_path)
                if nodes_i is None:
                    status = 4
                else:
                    m = len(nodes_i)
                    path[i, :m] = nodes_i
                    path_cost[i] = cost[i, start]
                    ref[i] = rr.reference_points(D, origin, cell, L, stride, p0[i], pf[i], nodes_i, K)
        info[i] = (status, m, start, goal)
        n_failed += status != 0
    return ref, path, info, path_cost, cost, n_failed


def cost_matrix(D, origin, cell, dims, stride, edges, pen, src, dst):
    """scp_lattice_costs -> (costs (n_src, n_dst) uint32, src_node, dst_node int32, cost (n_src, nodes) uint32)"""
    L = rr.lattice(D, dims, stride)
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    src_node = np.array([ar.passable_node(D, origin, cell, dims, L, stride, edges, p) for p in src], dtype=np.int32)
    dst_node = np.array([ar.passable_node(D, origin, cell, dims, L, stride, edges, p) for p in dst], dtype=np.int32)
    cost = np.full((len(src), edges.size), UNREACHED, dtype=np.uint32)
    costs = np.full((len(src), len(dst)), UNREACHED, dtype=np.uint32)
    fields = {}
    ok = dst_node >= 0
    for a, node in enumerate(src_node):
        if node < 0:
            continue
        if int(node) not in fields:
            fields[int(node)] = cost_field(L, edges, pen, int(node))
        cost[a] = fields[int(node)]
        costs[a, ok] = cost[a, dst_node[ok]]
    return costs, src_node, dst_node, cost


def bellman_ford(L, edges, pen, origin):
    """the same field by dense synchronous Bellman-Ford rounds in numpy (independent of cost_field): int64 rounds over all
    nodes and all directions at once until nothing changes"""
    nodes = edges.size
    INF = np.int64(1) << np.int64(50)
    cost = np.full(nodes, INF, dtype=np.int64)
    cost[origin] = 0
    p = np.zeros(nodes, dtype=np.int64) if pen is None else pen.astype(np.int64)
    idx = np.arange(nodes, dtype=np.int64)
    for _ in range(nodes):
        new = cost.copy()
        for n in range(27):
            if n == rr.SELF:
                continue
            has = (edges >> np.uint32(n) & np.uint32(1)) != 0
            if not has.any():
                continue
            u = idx[has]
            v = rr.neighbour(L, u, n)
            new[u] = np.minimum(new[u], cost[v] + 2 * W[move_len(n)] + p[u] + p[v])
        if (new == cost).all():
            break
        cost = new
    return np.where(cost >= INF, UNREACHED, cost).astype(np.uint32)
