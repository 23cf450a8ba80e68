"""numpy / plain-Python restatement of the rules of include/scp_hip.h, "static obstacles: shared paths": the load and the
overuse of a path set, one vehicle's shared penalty, the re-routing of one group and the negotiation over the rounds.  The
cost fields come from weighted_path_ref.cost_field with pen_i as the penalty array, the walk from weighted_path_ref.walk, the
reference points from reference_path_ref: integers exactly, the points bit for bit."""
import numpy as np

import reference_path_ref as rr
import weighted_path_ref as wr

UNREACHED = wr.UNREACHED
MAX_PRODUCT = wr.MAX_PRODUCT      # SCP_PENALTY_MAX_PRODUCT: the clamp of pen_i
MAX_ROUNDS = 64                   # SCP_NEGOTIATE_MAX_ROUNDS
PATH_INFO_DTYPE = rr.PATH_INFO_DTYPE


def nodes_of(path, info, i):
    """nodes_i: the first n_nodes entries of row i if status == 0, otherwise empty"""
    return [int(u) for u in path[i, :int(info["n_nodes"][i])]] if info["status"][i] == 0 else []


def path_load(path, info, nodes, capacity):
    """scp_path_load -> (load uint32 [nodes], overuse as a Python int)"""
    assert capacity >= 1
    load = [0] * nodes
    for i in range(path.shape[0]):
        for u in nodes_of(path, info, i):
            load[u] += 1
    return np.array(load, dtype=np.uint32), sum(max(0, v - capacity) for v in load)


def shared_penalty(pen, load, own, share_weight, capacity):
    """pen_i uint32 [nodes] of a vehicle whose path holds the nodes `own`: Python integers, clamped at MAX_PRODUCT"""
    assert 0 <= share_weight <= MAX_PRODUCT and capacity >= 1
    own = set(own)
    out = np.empty(len(load), dtype=np.uint32)
    for u in range(len(load)):
        others = int(load[u]) - (u in own)
        out[u] = min((0 if pen is None else int(pen[u])) + share_weight * max(0, others + 1 - capacity), MAX_PRODUCT)
    return out


def reroute(D, origin, cell, dims, stride, edges, pen, p0, pf, K, max_path, ref, path, info, path_cost, load, share_weight,
            capacity, groups, group, cost=None):
    """scp_reference_paths_shared -> (ref, path, info, path_cost, cost, n_kept): copies of the four in/out arrays (and of `cost`,
    the caller's pre-filled cost_out, where given) with the rows of the active vehicles replaced"""
    L = rr.lattice(D, dims, stride)
    N = path.shape[0]
    assert 1 <= groups <= N and 0 <= group < groups
    ref, path, info, path_cost = (np.array(a, copy=True) for a in (ref, path, info, path_cost))
    cost = None if cost is None else np.array(cost, copy=True)
    before = (path.copy(), info.copy())  # every active vehicle reads the set on entry
    n_kept = 0
    for i in range(group, N, groups):
        if before[1]["status"][i] != 0:
            continue  # skipped: nothing of it is written
        start, goal = int(before[1]["start_node"][i]), int(before[1]["goal_node"][i])
        pen_i = shared_penalty(pen, load, nodes_of(*before, i), share_weight, capacity)
        field = wr.cost_field(L, edges, pen_i, goal)
        if cost is not None:
            cost[i] = field
        assert field[start] != UNREACHED, "penalties cannot change what can be reached"
        nodes_i = wr.walk(L, edges, pen_i, field, start, goal, max_path)
        if nodes_i is None:
            n_kept += 1  # keeps its path row, info, ref rows and path_cost entirely
            continue
        assert len(set(nodes_i)) == len(nodes_i)
        path[i] = -1
        path[i, :len(nodes_i)] = nodes_i
        info[i] = (0, len(nodes_i), start, goal)
        path_cost[i] = field[start]
        ref[i] = rr.reference_points(D, origin, cell, L, stride, p0[i], pf[i], nodes_i, K)
    return ref, path, info, path_cost, cost, n_kept


def negotiate(D, origin, cell, sat, stride, edges, pen, p0, pf, K, max_path, ref, share_weight, capacity, groups, rounds):
    """scp_negotiate_paths -> {"ref", "path", "info", "path_cost", "n_failed", "overuse" (list of rounds + 1 ints), "best_round",
    "n_kept", "sets": the (ref, path, info, path_cost) of every round, "loads": the load every round r >= 1 read}"""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    nodes = edges.size
    p0, pf = np.asarray(p0, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    assert 0 <= rounds <= MAX_ROUNDS and 1 <= groups <= p0.shape[0]
    r0, path, info, path_cost, _, n_failed = wr.reference_paths_weighted(D, origin, cell, sat, stride, edges, pen, p0, pf, K, max_path,
                                                                        ref)
    sets, loads, overuse, n_kept = [(r0, path, info, path_cost)], [], [], 0
    for r in range(rounds + 1):
        load, over = path_load(sets[-1][1], sets[-1][2], nodes, capacity)
        overuse.append(over)
        if r == rounds:
            break
        loads.append(load)
        *new, _, kept = reroute(D, origin, cell, dims, stride, edges, pen, p0, pf, K, max_path, *sets[-1], load, share_weight,
                                capacity, groups, r % groups)
        sets.append(tuple(new))
        n_kept += kept
    best = min(range(rounds + 1), key=lambda r: (overuse[r], r))
    ref, path, info, path_cost = sets[best]
    return {"ref": ref, "path": path, "info": info, "path_cost": path_cost, "n_failed": n_failed, "overuse": overuse,
            "best_round": best, "n_kept": n_kept, "sets": sets, "loads": loads}
