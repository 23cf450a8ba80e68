"""Device time of scp_rasterize_shapes (shapes into an occupancy grid), beside the host rasteriser and scp_occupancy_prepare.

    python tools/rasterize_timing.py [--reps 30] [--warmup 5] [--skip-host]

Maps: those of tools/corridor_timing.py -- 1024^2 cells (2-D) and 256^3 cells (3-D, 2^24: the supported maximum), workspace
100 m wide, 40 random discs / spheres of radius 2 .. 6 m, margin 0.4 m (the same seeds, so the same maps) -- and on each grid a
map of 40 oblique capsules (length 10 .. 40 m, radius 0.2 .. 1 m) and 20 polygons of 16 vertices (stars of radius 3 .. 8 m; in
3-D prisms 5 .. 30 m high).  Device times are HIP events around the call's clear, copy and launch (scp_ctx_last_pair_ms):
median, min, quartiles and max over the repetitions after the warm-up.  Beside each disc map, on the SAME machine: the host's
scenarios.obstacles.rasterize plus the upload of its grid (wall clock, median of 3), and the check that the device grid has
the same bytes; beside every map scp_occupancy_prepare on the same grid, and the item count at the default work item size
and at 64 and 16384 cells per item."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from corridor_timing import fmt, q  # noqa: E402

WIDTH, MARGIN = 100.0, 0.4


def disc_map(D, n_cells):
    rng = np.random.default_rng(D * 1000 + n_cells)  # (the map of corridor_timing.scene)
    return {"discs": [tuple(rng.uniform(10.0, 90.0, D)) + (float(rng.uniform(2.0, 6.0)),) for _ in range(40)]}


def oblique_map(D, n_cells):
    rng = np.random.default_rng(D * 1000 + n_cells + 1)
    capsules, polygons = [], []
    for _ in range(40):
        a = rng.uniform(5.0, 95.0, D)
        u = rng.normal(size=D)
        b = a + u / np.linalg.norm(u) * rng.uniform(10.0, 40.0)
        capsules.append(tuple(a) + tuple(b) + (float(rng.uniform(0.2, 1.0)),))
    for _ in range(20):
        c, rad = rng.uniform(10.0, 90.0, 2), rng.uniform(3.0, 8.0)
        ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, 16))
        verts = c + (rad * rng.uniform(0.4, 1.0, 16))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        z0 = float(rng.uniform(0.0, 60.0))
        polygons.append((verts, z0, z0 + float(rng.uniform(5.0, 30.0))) if D == 3 else (verts,))
    return {"capsules": capsules, "polygons": polygons}


def timed(ctx, call, reps, warmup):
    t, out = [], None
    for r in range(warmup + reps):
        out = call()
        ms = ctx.last_pair_ms()
        if r >= warmup:
            t.append(ms)
    return out, t


def measure(ctx, D, n_cells, name, shapes, reps, warmup, skip_host):
    import torch

    from path_planning import _hip
    from path_planning.scenarios.obstacles import grid_shape, pack_shapes, rasterize

    space = [0.0] * D + [WIDTH] * D
    cell = WIDTH / n_cells
    origin, dims = grid_shape(space, cell)
    grid = _hip.occupancy_grid(D, origin, cell, dims)
    packed = pack_shapes(D, **shapes)
    occ, t_dev = timed(ctx, lambda: ctx.rasterize_shapes(D, grid, packed, MARGIN), reps, warmup)
    got = occ.cpu().numpy()
    print(f"grid {' x '.join(str(n) for n in dims)} ({got.size} cells, cell {cell:.3f} m), {name}: {packed['shapes'].size} shapes, "
          f"{packed['vertices'].shape[0]} vertices, {100.0 * got.mean():.1f} % occupied", flush=True)
    print(f"    scp_rasterize_shapes          {fmt(q(t_dev))}", flush=True)
    for cells in (64, 16384):
        ctx.set_option("raster_item_cells", cells)
        other, t = timed(ctx, lambda: ctx.rasterize_shapes(D, grid, packed, MARGIN), reps, warmup)
        same = bool(torch.equal(other, occ))
        print(f"      at {cells:5d} cells per item    {fmt(q(t))}; the same grid: {same}", flush=True)
    ctx.set_option("raster_item_cells", 0)
    _, t_sat = timed(ctx, lambda: ctx.occupancy_prepare(D, grid, occ), reps, warmup)
    print(f"    scp_occupancy_prepare         {fmt(q(t_sat))}", flush=True)
    if "discs" in shapes and not skip_host:
        host, up = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            h_occ, _, _ = rasterize(space, cell, discs=shapes["discs"], margin=MARGIN)
            t1 = time.perf_counter()
            d = torch.as_tensor(h_occ).to(ctx.tdev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3)
            up.append((t2 - t1) * 1e3)
        print(f"    host rasterize + upload       median {np.median(host):.1f} ms + {np.median(up):.2f} ms of 3 (min {min(host):.1f} + "
              f"{min(up):.2f}); the same bytes as the device grid: {bool(np.array_equal(h_occ, got))}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="without the host rasteriser (1.8 s per 256^3 map)")
    args = ap.parse_args()
    from path_planning import _hip

    ctx = _hip.Context(0)
    for D, n_cells in ((2, 1024), (3, 256)):
        measure(ctx, D, n_cells, "40 discs" if D == 2 else "40 spheres", disc_map(D, n_cells), args.reps, args.warmup, args.skip_host)
        measure(ctx, D, n_cells, "40 capsules + 20 polygons of 16 vertices", oblique_map(D, n_cells), args.reps, args.warmup, True)
    ctx.close()


if __name__ == "__main__":
    main()
