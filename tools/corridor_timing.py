"""Device time of the static-obstacle calls -- scp_occupancy_prepare, scp_corridor_boxes, scp_corridor_state_boxes,
scp_check_corridor -- and the price of position boxes in the joint QP (the round-2 persistent kernel against the lean one).

    python tools/corridor_timing.py [--reps 30] [--warmup 5] [--skip-step]

Shape: 1024 vehicles x 50 steps.  Grids: 1024^2 cells (2-D) and 256^3 cells (3-D, 2^24: the supported maximum), workspace
100 m wide, 40 random discs / spheres of radius 2 .. 6 m rasterised with a margin of 0.4 m.  Reference paths: straight lines
between random free points (segments that cross an obstacle are blocked and cost one table query; the line says how many).
Trajectories for the check: the reference points as positions, random velocities and accelerations.  Times are HIP events
around each call's launches (scp_ctx_last_pair_ms): median, min, quartiles and max over the repetitions after the warm-up.

The step: one SCP iteration (scp_solver_step) of bench.py's grid-swap scenario at 1024 x 50 x 2 from QP#0's solution, without
boxes (lean 8-agent kernel) and with boxes wider than the workspace (the same QP on the round-2 kernel), alternating."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd")):
    sys.path.insert(0, p)


def q(v):
    a = np.sort(np.asarray(v, dtype=float))
    return float(np.median(a)), float(a[0]), float(np.percentile(a, 25)), float(np.percentile(a, 75)), float(a[-1])


def fmt(s):
    return f"median {s[0]*1e3:8.1f} us (min {s[1]*1e3:.1f}, quartiles {s[2]*1e3:.1f} .. {s[3]*1e3:.1f}, max {s[4]*1e3:.1f})"


def scene(D, n_cells, rng):
    from path_planning.scenarios.obstacles import rasterize

    width = 100.0
    space = [0.0] * D + [width] * D
    discs = [tuple(rng.uniform(10.0, 90.0, D)) + (float(rng.uniform(2.0, 6.0)),) for _ in range(40)]
    return rasterize(space, width / n_cells, discs=discs, margin=0.4)


def free_points(rng, occ, origin, cell, D, n):
    free = np.argwhere(occ == 0)
    pick = free[rng.integers(len(free), size=n)][:, ::-1][:, :D]  # (z, y, x) -> (x, y[, z])
    return origin + cell * (pick + rng.uniform(0.1, 0.9, (n, D)))


def measure_grid(ctx, D, n_cells, N, K, h, reps, warmup, max_grows):
    from path_planning import _hip

    rng = np.random.default_rng(D * 1000 + n_cells)
    occ, origin, cell = scene(D, n_cells, rng)
    grid = _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])
    a, b = free_points(rng, occ, origin, cell, D, N), free_points(rng, occ, origin, cell, D, N)
    b = a + (b - a) * (15.0 / np.maximum(np.linalg.norm(b - a, axis=1, keepdims=True), 15.0))  # at most 15 m: 0.3 m per segment
    s = (np.arange(K + 1) / K)[None, :, None]
    ref = ctx.tensor(a[:, None, :] + s * (b - a)[:, None, :])
    pos = ref[:, :K].contiguous()
    vel = ctx.tensor(rng.normal(0, 1.0, (N, K, D)))
    acc = ctx.tensor(rng.uniform(-15, 15, (N, K, D)))
    shrink = 15.0 * h * h / 8 + 0.02
    import torch

    d_occ = torch.as_tensor(occ).to(ctx.tdev)
    for max_grow in max_grows:
        measure_calls(ctx, D, N, K, h, reps, warmup, max_grow, occ, cell, grid, d_occ, ref, pos, vel, acc, shrink)


def measure_calls(ctx, D, N, K, h, reps, warmup, max_grow, occ, cell, grid, d_occ, ref, pos, vel, acc, shrink):
    t = {k: [] for k in ("prepare", "boxes", "state_boxes", "check")}
    for r in range(warmup + reps):
        _, sat = ctx.occupancy_prepare(D, grid, d_occ)
        t0 = ctx.last_pair_ms()
        cells, n_blocked = ctx.corridor_boxes(N, K, D, grid, sat, ref, max_grow)
        t1 = ctx.last_pair_ms()
        lo, hi, n_open = ctx.corridor_state_boxes(N, K, D, grid, cells, shrink)
        t2 = ctx.last_pair_ms()
        st = ctx.check_corridor(N, K, D, h, grid, cells, pos, vel, acc, 0.0)
        t3 = ctx.last_pair_ms()
        if r >= warmup:
            for k, v in zip(t, (t0, t1, t2, t3)):
                t[k].append(v)
    hc = cells.cpu().numpy()
    ok = hc[..., 3] >= hc[..., 0]
    grown = (hc[..., 3:3 + D] - hc[..., :D] + 1)[ok].mean() if ok.any() else 0.0
    dims = " x ".join(str(n) for n in occ.shape[::-1][:D])
    print(f"grid {dims} ({occ.size} cells, {100.0 * occ.mean():.1f} % occupied, cell {cell:.3f} m), {N} x {K} x {D}, max_grow "
          f"{max_grow}: {int(n_blocked.item())} blocked segments, {int(n_open.item())} open states, mean box edge {grown:.1f} cells, "
          f"{int(st['n_outside'].sum())} segments outside", flush=True)
    for k in t:
        print(f"    {k:12s} {fmt(q(t[k]))}", flush=True)


def measure_step(N, K, h, R, reps, warmup):
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP

    p0, pf, space = generate_grid_swap(N, seed=1000 * N, dim=2)
    s = SCP(N, K * h + 1e-9, h, R, space, dim=2, device=0, verbose=False)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s._precompute_constraint_matrices()
    acc0 = s._solve_initial_trajectory()
    wide = (np.full((N, K, 2), np.asarray(space[:2]) - 1.0), np.full((N, K, 2), np.asarray(space[2:]) + 1.0))
    out = {False: [], True: []}
    for r in range(warmup + reps):
        for boxes in (False, True):
            s.set_position_boxes(*(wide if boxes else (None, None)))
            _, info = s.scp_iteration(acc0)
            if r >= warmup:
                out[boxes].append((info["solve_ms"] / max(info["iter"], 1), info["solve_ms"], info["time_sec"] * 1e3, info["iter"],
                                   info["pipeline"]))
    for boxes in (False, True):
        per, solve, wall = (q([o[i] for o in out[boxes]]) for i in range(3))
        print(f"SCP step {N} x {K} x 2, {'with' if boxes else 'without'} boxes [{out[boxes][-1][4]}], {out[boxes][-1][3]} ADMM steps: "
              f"per ADMM step {fmt(per)}; QP solve median {solve[0]:.3f} ms; iteration wall median {wall[0]:.3f} ms", flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    from path_planning import _hip

    N, K, h, R = 1024, 50, 0.2, 0.8
    ctx = _hip.Context(0)
    for D, n_cells in ((2, 1024), (3, 256)):
        measure_grid(ctx, D, n_cells, N, K, h, args.reps, args.warmup, (8, 32))
    ctx.close()
    if not args.skip_step:
        measure_step(N, K, h, R, max(args.reps // 3, 5), 2)


if __name__ == "__main__":
    main()
