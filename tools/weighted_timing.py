"""Device time of the weighted lattice search beside the hop search it stands next to.

    python tools/weighted_timing.py [--reps 30] [--warmup 5] [--threads 256 512 1024] [--only hops | weighted]

Part 1: scp_reference_paths (hops) and scp_reference_paths_weighted (length alone, and length with keep_clear = 2 at weight 70)
on the two lattices of tools/reference_timing.py -- the same maps, 1024 vehicles x 50 steps, the same starts and goals -- per
workgroup width.  Part 2: scp_lattice_distances and scp_lattice_costs on the 181 x 181 map of tools/assign_paths_times.py, 256
sources and destinations.  --only hops with SCP_HIP_LIB naming another build of the library (the parent commit's) measures
the hop kernels there, so that the comparison point is not this tree's own code; --only weighted measures the rest.  Times are HIP events around each call's launches
(scp_ctx_last_pair_ms), median of the repetitions after the warm-up.  For 8 vehicles / 4 sources the tool also counts on the host
the levels of the breadth-first search and the synchronous Bellman-Ford rounds the weighted field needs (tests/
weighted_path_ref.py) -- an upper bound on the device's sweeps, which read values stored earlier in the same sweep."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from corridor_timing import scene  # noqa: E402
from reference_timing import block_points  # noqa: E402

import assign_paths_times as apt  # noqa: E402


def median(ms):
    return float(np.median(ms))


def rounds_to_fixed_point(L, edges, pen, origin):
    """synchronous Bellman-Ford rounds until nothing changes (the last, idle one included)"""
    import reference_path_ref as rr
    import weighted_path_ref as wr

    nodes = edges.size
    INF = np.int64(1) << np.int64(50)
    cost = np.full(nodes, INF, dtype=np.int64)
    cost[origin] = 0
    p = np.zeros(nodes, dtype=np.int64) if pen is None else pen.astype(np.int64)
    idx = np.arange(nodes, dtype=np.int64)
    moves = [(n, idx[(edges >> np.uint32(n) & np.uint32(1)) != 0]) for n in range(27) if n != rr.SELF]
    moves = [(n, u, rr.neighbour(L, u, n)) for n, u in moves if u.size]
    for r in range(1, nodes + 1):
        new = cost.copy()
        for n, u, v in moves:
            new[u] = np.minimum(new[u], cost[v] + 2 * wr.W[wr.move_len(n)] + p[u] + p[v])
        if (new == cost).all():
            return r
        cost = new
    return nodes


def reference_scene(D, n_cells, stride, N, K):
    from path_planning import _hip
    from path_planning.scenarios.obstacles import default_search_stride

    rng = np.random.default_rng(D * 1000 + n_cells)
    occ, origin, cell = scene(D, n_cells, rng)
    if stride is None:
        stride = default_search_stride(occ.shape[::-1][:D], K, D)
    grid = _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])
    return rng, occ, origin, cell, stride, grid


def part1(ctx, D, n_cells, stride, N, K, reps, warmup, thread_counts, which):
    """which: "hops", "weighted" or "both" -> {label: {threads: median ms}}"""
    import torch

    from path_planning import _hip

    rng, occ, origin, cell, stride, grid = reference_scene(D, n_cells, stride, N, K)
    L = _hip.lattice_shape(D, grid, stride)
    nodes = L[0] * L[1] * L[2]
    max_path = min(nodes, 8 * K)
    d_occ, sat = ctx.occupancy_prepare(D, grid, torch.as_tensor(occ).to(ctx.tdev))
    edges = ctx.lattice_edges(D, grid, sat, stride, 0)
    h_edges = edges.cpu().numpy().view(np.uint32)
    passable = np.nonzero(h_edges >> np.uint32(13) & np.uint32(1))[0]
    starts, goals = rng.choice(passable, N), rng.choice(passable, N)
    p0 = block_points(rng, D, origin, cell, stride, L, starts)
    pf = block_points(rng, D, origin, cell, stride, L, goals)
    straight = p0[:, None, :] + (np.arange(K + 1) / K)[None, :, None] * (pf - p0)[:, None, :]
    d_p0, d_pf = ctx.tensor(p0), ctx.tensor(pf)
    out = {"lattice": list(L[:D]), "nodes": nodes, "stride": stride}

    def timed(call):
        res = {}
        for threads in thread_counts + [0]:
            ctx.set_option("ref_path_threads", threads)
            ms = []
            for r in range(warmup + reps):
                ref = ctx.tensor(straight)
                call(ref)
                if r >= warmup:
                    ms.append(ctx.last_pair_ms())
            res[str(threads)] = median(ms)
        ctx.set_option("ref_path_threads", 0)
        return res

    if which in ("hops", "both"):
        out["hops"] = timed(lambda ref: ctx.reference_paths(N, K, D, grid, stride, edges, d_p0, d_pf, max_path, ref, want_path=False))
    if which in ("weighted", "both"):
        pen = ctx.lattice_penalties(D, grid, ctx.obstacle_distance(D, grid, d_occ, 1), stride, 2, 70)
        out["penalties_ms"] = ctx.last_pair_ms()
        out["length"] = timed(lambda ref: ctx.reference_paths_weighted(N, K, D, grid, stride, edges, d_p0, d_pf, max_path, ref,
                                                                       want_path=False))
        out["length_keep_clear_2"] = timed(lambda ref: ctx.reference_paths_weighted(N, K, D, grid, stride, edges, d_p0, d_pf,
                                                                                    max_path, ref, pen=pen, want_path=False))
        import reference_path_ref as rr

        h_pen = pen.cpu().numpy().view(np.uint32)
        levels, rounds, rounds_pen = [], [], []
        for i in range(8):
            dist = rr.distances(L, h_edges, int(goals[i]))
            if dist[starts[i]] != rr.UNREACHED:
                levels.append(int(dist[starts[i]]))
            rounds.append(rounds_to_fixed_point(L, h_edges, None, int(goals[i])))
            rounds_pen.append(rounds_to_fixed_point(L, h_edges, h_pen, int(goals[i])))
        out["host_counts_8_vehicles"] = {"bfs_levels_to_the_start": levels, "rounds_length": rounds, "rounds_keep_clear_2": rounds_pen}
    return out


def part2(ctx, N, reps, warmup, which):
    import torch

    from path_planning import _hip

    occ = apt.the_map()
    grid = _hip.occupancy_grid(2, [0.0, 0.0], apt.CELL, (apt.SIDE, apt.SIDE))
    d_occ, sat = ctx.occupancy_prepare(2, grid, torch.as_tensor(occ).to(ctx.tdev))
    edges = ctx.lattice_edges(2, grid, sat, 1, 0)
    src, dst = apt.points(occ, N, 11)
    d_src, d_dst = ctx.tensor(src), ctx.tensor(dst)
    out = {"N": N, "nodes": apt.SIDE * apt.SIDE}

    def timed(call):
        ms = []
        for r in range(warmup + reps):
            call()
            if r >= warmup:
                ms.append(ctx.last_pair_ms())
        return median(ms)

    if which in ("hops", "both"):
        out["lattice_distances_ms"] = timed(lambda: ctx.lattice_distances(2, grid, 1, edges, d_src, d_dst))
    if which in ("weighted", "both"):
        pen = ctx.lattice_penalties(2, grid, ctx.obstacle_distance(2, grid, d_occ, 1), 1, 2, 70)
        out["lattice_costs_ms"] = timed(lambda: ctx.lattice_costs(2, grid, 1, edges, d_src, d_dst))
        out["lattice_costs_keep_clear_2_ms"] = timed(lambda: ctx.lattice_costs(2, grid, 1, edges, d_src, d_dst, pen=pen))
        import reference_path_ref as rr

        h_edges, h_pen = edges.cpu().numpy().view(np.uint32), pen.cpu().numpy().view(np.uint32)
        L = (apt.SIDE, apt.SIDE, 1)
        nodes = [int(n) for n in ctx.lattice_costs(2, grid, 1, edges, d_src, d_dst)[1].cpu().numpy()[:4]]
        out["host_counts_4_sources"] = {
            "bfs_levels": [int(d[d != rr.UNREACHED].max()) for d in (rr.distances(L, h_edges, n) for n in nodes)],
            "rounds_length": [rounds_to_fixed_point(L, h_edges, None, n) for n in nodes],
            "rounds_keep_clear_2": [rounds_to_fixed_point(L, h_edges, h_pen, n) for n in nodes]}
    return out


def run(args, which):
    import ctypes

    import torch  # noqa: F401  (before the library: it brings the HIP runtime both then share)

    from path_planning import _hip

    if which == "hops":  # (a build from before the weighted search lacks its three entry points: they are not called here)
        lib = ctypes.CDLL(_hip.library_path())
        for name in ("scp_lattice_penalties", "scp_reference_paths_weighted", "scp_lattice_costs"):
            if not hasattr(lib, name):
                _hip.PROTOTYPES.pop(name, None)
    ctx = _hip.Context(0)
    out = {"library": _hip.library_path(), "reference_paths": [], "all_pairs": None}
    for D, n_cells, stride in ((2, 1024, None), (3, 256, 8)):
        out["reference_paths"].append(part1(ctx, D, n_cells, stride, 1024, 50, args.reps, args.warmup, args.threads, which))
    out["all_pairs"] = part2(ctx, 256, max(args.reps // 4, 3), 1, which)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--only", choices=("hops", "weighted", "both"), default="both")
    args = ap.parse_args()
    print(json.dumps(run(args, args.only)), flush=True)


if __name__ == "__main__":
    main()
