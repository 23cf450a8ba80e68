"""numpy / plain-Python restatement of the lattice-search rules of include/scp_hip.h ("reference paths by a lattice search"):
edge masks, breadth-first distances from the goal, the path, the reference points and the statuses.  Integers exactly; the
points bit for bit (numpy rounds every product, quotient, sum and difference on its own).  Cell lookup and summed table are
those of tests/corridor_ref.py."""
import numpy as np

import corridor_ref as cr

MAX_NODES = 32768
UNREACHED = 0xFFFF
SELF = 13

PATH_INFO_DTYPE = np.dtype([("status", np.int32), ("n_nodes", np.int32), ("start_node", np.int32), ("goal_node", np.int32)])


def direction(n):
    """(dx, dy, dz) of a direction code"""
    return n % 3 - 1, (n // 3) % 3 - 1, n // 9 - 1


DIRECTION_ORDER = sorted((n for n in range(27) if n != SELF), key=lambda n: (sum(abs(v) for v in direction(n)), n))


def lattice(D, dims, stride):
    """(L_x, L_y, L_z) of a grid dims = (nx, ny, nz); ValueError where the lattice is not supported"""
    if stride < 1:
        raise ValueError("stride >= 1")
    L = tuple(int(dims[d]) // stride if d < D else 1 for d in range(3))
    if min(L) < 1 or L[0] * L[1] * L[2] > MAX_NODES:
        raise ValueError(f"lattice {L} is not supported")
    return L


def node_id(L, X):
    return (X[2] * L[1] + X[1]) * L[0] + X[0]


def node_coords(L, node):
    return node % L[0], (node // L[0]) % L[1], node // (L[0] * L[1])


def _sat_at(sat, x, y, z):
    """sat at arrays of indices; a term with an index -1 is 0"""
    ok = (x >= 0) & (y >= 0) & (z >= 0)
    return np.where(ok, sat[np.maximum(z, 0), np.maximum(y, 0), np.maximum(x, 0)].astype(np.int64), 0)


def occupied_in(sat, a, b):
    """cr.occupied_in for arrays of ranges: a, b = three index arrays each"""
    n = (_sat_at(sat, b[0], b[1], b[2]) - _sat_at(sat, a[0] - 1, b[1], b[2]) - _sat_at(sat, b[0], a[1] - 1, b[2])
         + _sat_at(sat, a[0] - 1, a[1] - 1, b[2]))
    n -= (_sat_at(sat, b[0], b[1], a[2] - 1) - _sat_at(sat, a[0] - 1, b[1], a[2] - 1) - _sat_at(sat, b[0], a[1] - 1, a[2] - 1)
          + _sat_at(sat, a[0] - 1, a[1] - 1, a[2] - 1))
    return n


def lattice_edges(D, sat, stride, clearance):
    """sat [nz][ny][nx] -> edges uint32 [nodes] (all nodes at once, direction by direction)"""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    L = lattice(D, dims, stride)
    node = np.arange(L[0] * L[1] * L[2], dtype=np.int64)
    X = node_coords(L, node)
    edges = np.zeros(node.size, dtype=np.uint32)
    for n in range(27):
        dirn = direction(n)
        if D == 2 and dirn[2] != 0:
            continue
        Y = [X[d] + dirn[d] for d in range(3)]
        inside = np.ones(node.size, dtype=bool)
        a, b = [np.zeros_like(node)] * 3, [np.zeros_like(node)] * 3
        for d in range(D):
            inside &= (Y[d] >= 0) & (Y[d] < L[d])
            a[d] = np.maximum(np.minimum(X[d], Y[d]) * stride - clearance, 0)
            b[d] = np.minimum(np.maximum(X[d], Y[d]) * stride + stride - 1 + clearance, dims[d] - 1)
        free = occupied_in(sat, a, b) == 0
        edges |= np.where(inside & free, np.uint32(1 << n), np.uint32(0))
    return edges


def point_node(D, origin, cell, dims, L, stride, p):
    """the node of a point, or -1: a coordinate is not inside the grid or lies beyond the lattice"""
    X = [0, 0, 0]
    for d in range(D):
        inside, c = cr.cell_of(p[d], origin[d], cell, dims[d])
        if not inside or c // stride >= L[d]:
            return -1
        X[d] = c // stride
    return node_id(L, X)


def neighbour(L, node, n):
    dx, dy, dz = direction(n)
    return node + (dz * L[1] + dy) * L[0] + dx


def distances(L, edges, goal):
    """breadth-first distance of every node from `goal` over the set edge bits: uint16, 0xFFFF = unreached (level by level,
    every node of a level at once)"""
    dist = np.full(edges.size, UNREACHED, dtype=np.uint16)
    dist[goal] = 0
    used = int(np.bitwise_or.reduce(edges)) & ~(1 << SELF)
    frontier = np.array([goal], dtype=np.int64)
    level = 0
    while frontier.size:
        found = []
        for n in range(27):
            if used >> n & 1:
                nb = neighbour(L, frontier[(edges[frontier] >> np.uint32(n) & np.uint32(1)) != 0], n)
                nb = nb[dist[nb] == UNREACHED]
                dist[nb] = level + 1
                found.append(nb)
        frontier = np.unique(np.concatenate(found)) if found else frontier[:0]
        level += 1
    return dist


def distances_until(L, edges, goal, start, full=None):
    """the distances as the level-by-level search leaves them: it stops after the level that reaches `start` (or changes
    nothing), so nodes farther from the goal than the start stay unreached.  full: distances(L, edges, goal) if at hand"""
    dist = distances(L, edges, goal) if full is None else full.copy()
    if dist[start] != UNREACHED:
        dist[dist > dist[start]] = UNREACHED
    return dist


def walk(L, edges, dist, start):
    """the path from `start`: the first neighbour in direction order over a set edge bit with dist one less"""
    path = [start]
    node = start
    while dist[node] != 0:
        mask = int(edges[node])
        for n in DIRECTION_ORDER:
            if mask >> n & 1 and dist[neighbour(L, node, n)] == dist[node] - 1:
                node = neighbour(L, node, n)
                break
        else:
            raise AssertionError("a reached node without a neighbour one step nearer")
        path.append(node)
    return path


def reference_points(D, origin, cell, L, stride, p0, pf, path, K):
    """(K + 1, D) points along p0, the centres of the path's nodes, pf"""
    m = len(path)
    E = m + 1
    cell = np.float64(cell)
    V = np.empty((E + 1, D))
    V[0] = np.asarray(p0, dtype=np.float64)[:D]
    V[E] = np.asarray(pf, dtype=np.float64)[:D]
    for t, node in enumerate(path):
        X = node_coords(L, node)
        for d in range(D):
            V[t + 1, d] = np.float64(origin[d]) + cell * (np.float64(X[d] * stride) + np.float64(0.5) * np.float64(stride))
    out = np.empty((K + 1, D))
    for j in range(K + 1):
        q, r = divmod(j * E, K)
        if q == E:
            out[j] = V[E]
        else:
            out[j] = V[q] + (np.float64(r) / np.float64(K)) * (V[q + 1] - V[q])
    return out


def reference_paths(D, origin, cell, sat, stride, edges, p0, pf, K, max_path, ref):
    """-> (ref (N, K + 1, D) with the rows of the found vehicles replaced, path (N, max_path) int32, info PATH_INFO_DTYPE (N,),
    dist (N, nodes) uint16 as the search leaves it, n_failed)"""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    L = lattice(D, dims, stride)
    nodes = L[0] * L[1] * L[2]
    assert edges.shape == (nodes,) and 1 <= max_path <= nodes
    p0, pf = np.asarray(p0, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    N = p0.shape[0]
    ref = np.array(ref, dtype=np.float64, copy=True)
    path = np.full((N, max_path), -1, dtype=np.int32)
    info = np.zeros(N, dtype=PATH_INFO_DTYPE)
    dist = np.full((N, nodes), UNREACHED, dtype=np.uint16)
    n_failed = 0
    by_goal = {}  # (vehicles often share a goal node: one breadth-first search each)
    for i in range(N):
        status, start, goal, m = 0, -1, -1, 0
        start = point_node(D, origin, cell, dims, L, stride, p0[i])
        if start < 0 or not int(edges[start]) >> SELF & 1:
            status = 1
        if status == 0:
            goal = point_node(D, origin, cell, dims, L, stride, pf[i])
            if goal < 0 or not int(edges[goal]) >> SELF & 1:
                status = 2
        if status == 0:
            if goal not in by_goal:
                by_goal[goal] = distances(L, edges, goal)
            dist[i] = distances_until(L, edges, goal, start, by_goal[goal])
            if dist[i, start] == UNREACHED:
                status = 3
            elif int(dist[i, start]) + 1 > max_path:
                status = 4
            else:
                nodes_i = walk(L, edges, dist[i], start)
                m = len(nodes_i)
                assert m == int(dist[i, start]) + 1
                path[i, :m] = nodes_i
                ref[i] = reference_points(D, origin, cell, L, stride, p0[i], pf[i], nodes_i, K)
        info[i] = (status, m, start, goal)
        n_failed += status != 0
    return ref, path, info, dist, n_failed
