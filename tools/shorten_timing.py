"""Device time of scp_shorten_paths per workgroup size, next to scp_reference_paths on the same inputs, and what shortening
does to the paths: the length ratio, the number of vertices and the blocked corridor segments.

    python tools/shorten_timing.py [--reps 30] [--warmup 5] [--threads 64 128 256]

Shape and maps: those of tools/reference_timing.py -- 1024 vehicles x 50 steps on 1024^2 cells (2-D) at the default stride
and on 256^3 cells (3-D) at stride 8 -- with clearance = stride, the default of SCP.shorten_reference.  Times are HIP events
around each call's launch (scp_ctx_last_pair_ms): median, min, quartiles and max over the repetitions after the warm-up.
The first vehicles are also run through the Python restatement (tests/shorten_ref.py) and compared bit for bit."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from corridor_timing import fmt, q, scene  # noqa: E402
from reference_timing import block_points  # noqa: E402


def measure(ctx, D, n_cells, stride, N, K, reps, warmup, thread_counts, n_python):
    import torch

    from path_planning import _hip
    from path_planning.scenarios.obstacles import default_search_stride

    rng = np.random.default_rng(D * 1000 + n_cells)
    occ, origin, cell = scene(D, n_cells, rng)
    grid = _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])
    if stride is None:
        stride = default_search_stride(occ.shape[::-1][:D], K, D)
    clearance = stride
    L = _hip.lattice_shape(D, grid, stride)
    nodes = L[0] * L[1] * L[2]
    max_path = min(nodes, 8 * K)
    _, sat = ctx.occupancy_prepare(D, grid, torch.as_tensor(occ).to(ctx.tdev))
    edges = ctx.lattice_edges(D, grid, sat, stride, clearance)
    passable = np.nonzero(edges.cpu().numpy().view(np.uint32) >> np.uint32(13) & np.uint32(1))[0]
    p0 = block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
    pf = block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
    straight = p0[:, None, :] + (np.arange(K + 1) / K)[None, :, None] * (pf - p0)[:, None, :]
    d_p0, d_pf = ctx.tensor(p0), ctx.tensor(pf)
    dims = " x ".join(str(n) for n in occ.shape[::-1][:D])
    print(f"grid {dims} ({100.0 * occ.mean():.1f} % occupied, cell {cell:.3f} m), stride {stride}, clearance {clearance}: lattice "
          f"{' x '.join(str(n) for n in L[:D])} = {nodes} nodes, {passable.size} passable; {N} x {K} x {D}, max_path {max_path}",
          flush=True)
    t_search = []
    for r in range(warmup + reps):
        lattice_ref = ctx.tensor(straight)
        path, info, _, _ = ctx.reference_paths(N, K, D, grid, stride, edges, d_p0, d_pf, max_path, lattice_ref)
        if r >= warmup:
            t_search.append(ctx.last_pair_ms())
    print(f"    reference_paths, the call chooses the threads per workgroup  {fmt(q(t_search))}", flush=True)
    first = None
    for threads in thread_counts + [0]:
        ctx.set_option("shorten_threads", threads)
        t_shorten = []
        for r in range(warmup + reps):
            ref = lattice_ref.clone()
            kept, out = ctx.shorten_paths(N, K, D, grid, sat, stride, clearance, d_p0, d_pf, max_path, path, info, ref)
            if r >= warmup:
                t_shorten.append(ctx.last_pair_ms())
        got = (ref.cpu().numpy(), kept.cpu().numpy(), out.cpu().numpy())
        first = first or got
        same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, first))
        print(f"    shorten_paths, {str(threads) if threads else 'the call chooses the':>4s} threads per workgroup  "
              f"{fmt(q(t_shorten))}" + ("" if same else "  OUTPUTS DIFFER from the first run"), flush=True)
    rec = info.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:N]
    res = got[2].view(_hip.SHORTEN_INFO_DTYPE)[:N]
    found = rec["status"] == 0
    ratio = res["length"][found] / res["length_before"][found]
    delta = np.floor(res["length"] / (K * cell)).astype(np.int64) + 1
    sure = found & (clearance >= delta)
    blocked = {}
    for name, r in (("shortened", ref), ("lattice", lattice_ref)):
        hc = ctx.corridor_boxes(N, K, D, grid, sat, r, 8)[0].cpu().numpy()
        b = hc[..., 3] < hc[..., 0]
        blocked[name] = (int(b[found].sum()), int(b[sure].sum()))
    print(f"    {int(found.sum())} of {N} paths found; nodes per path: median {int(np.median(rec['n_nodes'][found]))}, max "
          f"{int(rec['n_nodes'][found].max())}; vertices after shortening: median {int(np.median(res['n_vertices'][found]))}, max "
          f"{int(res['n_vertices'][found].max())}; length after / before: median {np.median(ratio):.4f}, min {ratio.min():.4f}, max "
          f"{ratio.max():.4f}", flush=True)
    print(f"    blocked corridor segments of the found vehicles: {blocked['shortened'][0]} with the shortened reference, "
          f"{blocked['lattice'][0]} with the lattice reference; clearance >= delta for {int(sure.sum())} vehicles, whose shortened "
          f"references block {blocked['shortened'][1]}", flush=True)
    if n_python:
        import shorten_ref as sr

        n = n_python
        want = sr.shorten_paths(D, origin, cell, sat.cpu().numpy(), stride, clearance, p0[:n], pf[:n], K, path.cpu().numpy()[:n],
                                rec[:n], lattice_ref.cpu().numpy()[:n])
        same = (np.array_equal(want[0].view(np.uint64), got[0][:n].view(np.uint64)) and np.array_equal(want[1], got[1][:n])
                and want[2].tobytes() == res[:n].tobytes())
        print(f"    Python restatement on {n} vehicles: same kept lists, records and reference points: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--python-vehicles", type=int, default=8)
    args = ap.parse_args()
    from path_planning import _hip

    ctx = _hip.Context(0)
    for D, n_cells, stride in ((2, 1024, None), (3, 256, 8)):
        measure(ctx, D, n_cells, stride, 1024, 50, args.reps, args.warmup, args.threads, args.python_vehicles)
    ctx.close()


if __name__ == "__main__":
    main()
