"""Device time of the calls that judge a plan against the map: scp_obstacle_distance (the squared distance field of the
occupancy grid) and scp_obstacle_clearance (the per-vehicle and per-step minimum of the field over the plan's pieces).

    python tools/obstacle_distance_timing.py [--reps 30] [--warmup 5] [--fields-only]

Maps: those of tools/corridor_timing.py -- 1024^2 cells (2-D) and 256^3 cells (3-D, 2^24: the supported maximum), workspace
100 m wide, 40 random discs / spheres of radius 2 .. 6 m rasterised with a margin of 0.4 m (the same seeds, so the same maps)
-- and the empty map of each size, the worst case of the field's expansion form (every cell walks its whole line in every
envelope pass).  Beside the field: scipy.ndimage.distance_transform_edt of the dilated map on the host, a yardstick, and the
check that both give the same integers.  Plan: 1024 vehicles x 50 steps, the straight pieces of corridor_timing.py with
random velocities and accelerations, at 1, 4 and 16 pieces per segment.  Times are HIP events around each call's launches
(scp_ctx_last_pair_ms): median, min, quartiles and max over the repetitions after the warm-up.

The share of each pass of the field comes from a kernel trace, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/obstacle_distance_timing.py --fields-only
-- dist_rows_kernel is the pass along x, dist_envelope_kernel<1> the one along y, dist_envelope_kernel<2> the one along z."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from corridor_timing import fmt, free_points, q, scene  # noqa: E402


def dilate(occ):
    """a cell is occupied if a cell within one step per coordinate is"""
    out = occ != 0
    for axis in range(3):
        grown = out.copy()
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= out[tuple(hi)]
        grown[tuple(hi)] |= out[tuple(lo)]
        out = grown
    return out


def time_field(ctx, D, grid, d_occ, reps, warmup):
    t = []
    for r in range(warmup + reps):
        field = ctx.obstacle_distance(D, grid, d_occ, 1)
        ms = ctx.last_pair_ms()
        if r >= warmup:
            t.append(ms)
    return field, t


def measure_grid(ctx, D, n_cells, N, K, h, reps, warmup, fields_only):
    import torch

    from path_planning import _hip

    rng = np.random.default_rng(D * 1000 + n_cells)
    occ, origin, cell = scene(D, n_cells, rng)
    grid = _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])
    dims = " x ".join(str(n) for n in occ.shape[::-1][:D])
    d_occ = torch.as_tensor(occ).to(ctx.tdev)
    field, t_map = time_field(ctx, D, grid, d_occ, reps, warmup)
    _, t_empty = time_field(ctx, D, grid, torch.zeros_like(d_occ), reps, warmup)
    got = field.cpu().numpy().view(np.uint32)
    print(f"grid {dims} ({occ.size} cells, {100.0 * occ.mean():.1f} % occupied, cell {cell:.3f} m): largest squared distance "
          f"{int(got.max())} cells^2 ({cell * np.sqrt(float(got.max())):.2f} m)", flush=True)
    print(f"    field, gap 1        {fmt(q(t_map))}", flush=True)
    print(f"    field, empty map    {fmt(q(t_empty))}", flush=True)
    if fields_only:
        return
    try:
        from scipy import ndimage
    except ImportError:
        print("    scipy is not installed: no host yardstick", flush=True)
    else:
        grown = dilate(occ)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            edt = ndimage.distance_transform_edt(~grown)
            host.append((time.perf_counter() - t0) * 1e3)
        same = np.array_equal(np.rint(edt * edt).astype(np.uint32), got)
        print(f"    scipy.ndimage.distance_transform_edt of the dilated map, host: median {np.median(host):.1f} ms of 3 "
              f"(min {min(host):.1f}); the same integers: {same}", flush=True)
    _, sat = ctx.occupancy_prepare(D, grid, d_occ)
    a, b = free_points(rng, occ, origin, cell, D, N), free_points(rng, occ, origin, cell, D, N)
    b = a + (b - a) * (15.0 / np.maximum(np.linalg.norm(b - a, axis=1, keepdims=True), 15.0))  # at most 15 m: 0.3 m per segment
    s = (np.arange(K) / K)[None, :, None]
    pos = ctx.tensor(a[:, None, :] + s * (b - a)[:, None, :])
    vel = ctx.tensor(rng.normal(0, 1.0, (N, K, D)))
    acc = ctx.tensor(rng.uniform(-15, 15, (N, K, D)))
    for pieces in (1, 4, 16):
        t = []
        for r in range(warmup + reps):
            st, step_min = ctx.obstacle_clearance(N, K, D, h, grid, sat, field, pieces, pos, vel, acc)
            ms = ctx.last_pair_ms()
            if r >= warmup:
                t.append(ms)
        sq = st["min_sq"].astype(np.float64)
        print(f"    clearance, {N} x {K} x {D}, {pieces:2d} pieces  {fmt(q(t))}; fleet clearance {cell * np.sqrt(sq.min()):.3f} m, "
              f"median vehicle {cell * np.sqrt(np.median(sq)):.3f} m, {int(st['n_touch'].sum())} of {N * K * pieces} pieces touch, "
              f"{int(st['n_off'].sum())} off the map, {int(st['n_wide'].sum())} wide", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fields-only", action="store_true", help="only the field calls (for a kernel trace)")
    args = ap.parse_args()
    from path_planning import _hip

    ctx = _hip.Context(0)
    for D, n_cells in ((2, 1024), (3, 256)):
        measure_grid(ctx, D, n_cells, 1024, 50, 0.2, args.reps, args.warmup, args.fields_only)
    ctx.close()


if __name__ == "__main__":
    main()
