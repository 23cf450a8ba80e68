"""Device time of the shared path search beside the plain weighted search.

    python tools/shared_timing.py [--reps 9] [--vehicles 256] [--groups 4] [--rounds 8] [--only weighted | shared]

The 181 x 181 map of tools/assign_paths_times.py (two long walls) at stride 1 (32761 nodes: the 128 KiB field) and at stride 2
(90 x 90 = 8100 nodes: the 32 KiB field), 256 vehicles x 50 steps, share 1 (weight 70), capacity 1.  Per lattice: one
scp_reference_paths_weighted of all vehicles, one scp_path_load, one scp_reference_paths_shared of group 0 (N / groups vehicles,
from the plain set and its load) and the whole scp_negotiate_paths; times are HIP events around each call's launches
(scp_ctx_last_pair_ms), median of the repetitions after one warm-up.  --only weighted measures the plain search alone and
calls none of the shared-path entry points, so it also runs on a library (SCP_HIP_LIB) that lacks them."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import assign_paths_times as apt  # noqa: E402

NEW = ("scp_path_load", "scp_reference_paths_shared", "scp_negotiate_paths")


def median(call, ctx, reps):
    ms = []
    for r in range(reps + 1):
        call()
        if r:
            ms.append(ctx.last_pair_ms())
    return float(np.median(ms))


def lattice(ctx, stride, N, K, groups, rounds, reps, which):
    import torch

    from path_planning import _hip

    occ = apt.the_map()
    grid = _hip.occupancy_grid(2, [0.0, 0.0], apt.CELL, (apt.SIDE, apt.SIDE))
    _, sat = ctx.occupancy_prepare(2, grid, torch.as_tensor(occ).to(ctx.tdev))
    edges = ctx.lattice_edges(2, grid, sat, stride, 0)
    L = _hip.lattice_shape(2, grid, stride)
    nodes = L[0] * L[1]
    max_path = min(nodes, 8 * K)
    p0, pf = apt.points(occ, N, 11)
    straight = p0[:, None, :] + (np.arange(K + 1) / K)[None, :, None] * (pf - p0)[:, None, :]
    d_p0, d_pf = ctx.tensor(p0), ctx.tensor(pf)
    out = {"stride": stride, "nodes": nodes, "N": N, "K": K, "max_path": max_path}

    def weighted():
        return ctx.reference_paths_weighted(N, K, 2, grid, stride, edges, d_p0, d_pf, max_path, ctx.tensor(straight))

    out["weighted_ms"] = median(weighted, ctx, reps)
    out["weighted_us_per_vehicle"] = 1e3 * out["weighted_ms"] / N
    if which == "weighted":
        return out
    ref = ctx.tensor(straight)
    path, info, path_cost, _, n_failed = ctx.reference_paths_weighted(N, K, 2, grid, stride, edges, d_p0, d_pf, max_path, ref)
    out["n_failed"] = int(n_failed.item())
    load, _ = ctx.path_load(N, max_path, nodes, path, info, 1)
    out["path_load_ms"] = median(lambda: ctx.path_load(N, max_path, nodes, path, info, 1, load=load), ctx, reps)

    def one_round():
        return ctx.reference_paths_shared(N, K, 2, grid, stride, edges, d_p0, d_pf, max_path, ref.clone(), path.clone(), info.clone(),
                                          path_cost.clone(), load, 70, 1, groups, 0)

    active = -(-N // groups)
    out["shared_round_ms"] = median(one_round, ctx, reps)
    out["shared_round_vehicles"] = active
    out["shared_us_per_vehicle"] = 1e3 * out["shared_round_ms"] / active
    out["per_vehicle_ratio"] = out["shared_us_per_vehicle"] / out["weighted_us_per_vehicle"]
    res = {}

    def negotiate():
        res["out"] = ctx.negotiate_paths(N, K, 2, grid, stride, edges, d_p0, d_pf, max_path, ctx.tensor(straight), 70, 1, groups, rounds)

    out["negotiate_ms"] = median(negotiate, ctx, reps)
    out["groups"], out["rounds"] = groups, rounds
    _, _, _, _, overuse, best_round, n_kept = res["out"]
    out["overuse"] = [int(v) for v in overuse.cpu().numpy().view(np.uint64)]
    out["best_round"], out["n_kept"] = int(best_round.item()), int(n_kept.item())
    out["launches_per_round"] = "search + load clear + load + overuse + keep = 4 kernels and 1 memset"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--vehicles", type=int, default=256)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", choices=("weighted", "shared"), default="shared")
    a = ap.parse_args()

    import torch  # noqa: F401  (before the library: it brings the HIP runtime both then share)

    from path_planning import _hip

    if a.only == "weighted":  # (a build from before the shared paths lacks their entry points)
        lib = ctypes.CDLL(_hip.library_path())
        for name in NEW:
            if not hasattr(lib, name):
                _hip.PROTOTYPES.pop(name, None)
    ctx = _hip.Context(0)
    out = {"library": _hip.library_path(), "lattices": [lattice(ctx, s, a.vehicles, 50, a.groups, a.rounds, a.reps, a.only) for s in (1, 2)]}
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
