"""Device time of the reference-path search -- scp_lattice_edges and scp_reference_paths -- per workgroup size, and for
comparison the wall clock of the Python restatement (tests/reference_path_ref.py) on 8 of the vehicles.

    python tools/reference_timing.py [--reps 30] [--warmup 5] [--threads 256 512 1024]

Shape: 1024 vehicles x 50 steps.  Grids: 1024^2 cells (2-D) at the default stride and 256^3 cells (3-D) at stride 8 (32768
nodes: the supported maximum), workspace 100 m wide, 40 random discs / spheres of radius 2 .. 6 m rasterised with a margin of
0.4 m (the scene of tools/corridor_timing.py).  Starts and goals: random points inside passable lattice blocks.  Times are HIP
events around each call's launches (scp_ctx_last_pair_ms): median, min, quartiles and max over the repetitions after the
warm-up.  The line of every grid also says how many levels the searches ran (path nodes - 1) and how many corridor segments
the found references block (scp_corridor_boxes)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from corridor_timing import fmt, q, scene  # noqa: E402


def block_points(rng, D, origin, cell, stride, L, nodes):
    X = np.stack([nodes % L[0], (nodes // L[0]) % L[1], nodes // (L[0] * L[1])], axis=1)[:, :D]
    return origin + cell * stride * (X + rng.uniform(0.05, 0.95, X.shape))


def measure(ctx, D, n_cells, stride, N, K, reps, warmup, thread_counts, n_python):
    import torch

    from path_planning import _hip
    from path_planning.scenarios.obstacles import default_search_stride

    rng = np.random.default_rng(D * 1000 + n_cells)
    occ, origin, cell = scene(D, n_cells, rng)
    grid = _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])
    if stride is None:
        stride = default_search_stride(occ.shape[::-1][:D], K, D)
    L = _hip.lattice_shape(D, grid, stride)
    nodes = L[0] * L[1] * L[2]
    max_path = min(nodes, 8 * K)
    _, sat = ctx.occupancy_prepare(D, grid, torch.as_tensor(occ).to(ctx.tdev))
    t_edges = []
    for r in range(warmup + reps):
        edges = ctx.lattice_edges(D, grid, sat, stride, 0)
        if r >= warmup:
            t_edges.append(ctx.last_pair_ms())
    h_edges = edges.cpu().numpy().view(np.uint32)
    passable = np.nonzero(h_edges >> np.uint32(13) & np.uint32(1))[0]
    p0 = block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
    pf = block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
    straight = p0[:, None, :] + (np.arange(K + 1) / K)[None, :, None] * (pf - p0)[:, None, :]
    d_p0, d_pf = ctx.tensor(p0), ctx.tensor(pf)
    dims = " x ".join(str(n) for n in occ.shape[::-1][:D])
    print(f"grid {dims} ({100.0 * occ.mean():.1f} % occupied, cell {cell:.3f} m), stride {stride}: lattice "
          f"{' x '.join(str(n) for n in L[:D])} = {nodes} nodes, {passable.size} passable; {N} x {K} x {D}, max_path {max_path}",
          flush=True)
    print(f"    lattice_edges            {fmt(q(t_edges))}", flush=True)
    for threads in thread_counts + [0]:
        ctx.set_option("ref_path_threads", threads)
        t_search = []
        for r in range(warmup + reps):
            ref = ctx.tensor(straight)
            _, info, _, n_failed = ctx.reference_paths(N, K, D, grid, stride, edges, d_p0, d_pf, max_path, ref, want_path=False)
            if r >= warmup:
                t_search.append(ctx.last_pair_ms())
        print(f"    reference_paths, {str(threads) if threads else 'the call chooses the':>4s} threads per workgroup  "
              f"{fmt(q(t_search))}", flush=True)
    rec = info.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:N]
    found = rec["status"] == 0
    levels = rec["n_nodes"][found] - 1
    cells, n_blocked = ctx.corridor_boxes(N, K, D, grid, sat, ref, 8)
    hc = cells.cpu().numpy()
    short = found & (rec["n_nodes"] + 1 <= K)
    blocked_short = int((hc[short][..., 3] < hc[short][..., 0]).sum())
    _, straight_blocked = ctx.corridor_boxes(N, K, D, grid, sat, ctx.tensor(straight), 8)
    print(f"    {int(found.sum())} of {N} paths found (statuses {np.bincount(rec['status'], minlength=5).tolist()}); levels per search: "
          f"median {int(np.median(levels))}, max {int(levels.max())}; E <= K for {int((rec['n_nodes'][found] + 1 <= K).sum())}; blocked "
          f"corridor segments: {int(n_blocked.item())} with the searched reference ({blocked_short} of them on paths with E <= K), "
          f"{int(straight_blocked.item())} with the straight lines", flush=True)
    if n_python:
        import reference_path_ref as rr

        h_sat = sat.cpu().numpy()
        t0 = time.perf_counter()
        py_edges = rr.lattice_edges(D, h_sat, stride, 0)
        t1 = time.perf_counter()
        want = rr.reference_paths(D, origin, cell, h_sat, stride, py_edges, p0[:n_python], pf[:n_python], K, max_path,
                                  straight[:n_python])
        t2 = time.perf_counter()
        same = np.array_equal(py_edges, h_edges) and np.array_equal(want[0].view(np.uint64), ref.cpu().numpy()[:n_python].view(np.uint64))
        print(f"    Python restatement: edges {1e3 * (t1 - t0):.1f} ms, {n_python} vehicles {1e3 * (t2 - t1):.1f} ms "
              f"({1e3 * (t2 - t1) / n_python:.1f} ms each); same edges and reference points: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--python-vehicles", type=int, default=8)
    args = ap.parse_args()
    from path_planning import _hip

    ctx = _hip.Context(0)
    for D, n_cells, stride in ((2, 1024, None), (3, 256, 8)):
        measure(ctx, D, n_cells, stride, 1024, 50, args.reps, args.warmup, args.threads, args.python_vehicles)
    ctx.close()


if __name__ == "__main__":
    main()
