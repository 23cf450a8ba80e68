"""Device time of the staggered starts: the mask pass (scp_lag_conflicts) next to scp_delay_margins at the same shape and lag
range, the segments each sends to the quartic, the schedule kernel (scp_schedule_starts), and SCP.stagger_starts end to end
next to SCP.repair_conflicts on the same trajectories.

    python tools/stagger_times.py [--reps 20] [--warmup 3] [--sizes 1024 4096] [--skip-repair]

Shape: N x 50 x 2, the grid-swap scenario of bench.py after a solve (QP#0 + SCP iterations, max 15).  Lags: S = 10 and 32.
Times are HIP events around each call's kernels (scp_ctx_last_pair_ms), the two passes alternating in one process: median,
min, quartiles and max over the repetitions after the warm-up.  The end-to-end figures are host wall clock of one call each
(uploads, the two separation checks and the host-side staggered fleet included)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from separation_times import fmt, q  # noqa: E402


def measure(ctx, N, K, D, h, R, dev, S, reps, warmup, label):
    t_lag, t_dly, t_sch = [], [], []
    for r in range(warmup + reps):
        mask = ctx.lag_conflicts(N, K, D, h, R, *dev, S, device=True)
        a = ctx.last_pair_ms()
        got = ctx.delay_margins(N, K, D, h, R, *dev, S)
        b = ctx.last_pair_ms()
        delays, st = ctx.schedule_starts(mask, S)
        c = ctx.last_pair_ms()
        if r >= warmup:
            t_lag.append(a)
            t_dly.append(b)
            t_sch.append(c)
    ctx.lag_conflicts(N, K, D, h, R, *dev, S, device=True)
    solved, solved_dly = ctx.last_lag_solved(), ctx.last_delay_solved()
    seg = N * (N - 1) * sum(K + s for s in range(S + 1))
    m = mask.cpu().numpy().view(np.uint64)
    anyb = np.bitwise_or.reduce(m, axis=1)
    bits = ((anyb[:, None] >> np.arange(S + 1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert (bits == (got["n_violating"] > 0)).all()
    a, b, c = q(t_lag), q(t_dly), q(t_sch)
    print(f"{label:26s} {N:5d} x {K} x {D}  S = {S:2d}  lag conflicts {fmt(a)}   delay margins {fmt(b)}   masks / margins "
          f"{a[0]/b[0]:.2f}   quartic: masks {solved} of {seg} segments ({100.0*solved/seg:.3f} %), margins {solved_dly} "
          f"({100.0*solved_dly/seg:.3f} %)   schedule {fmt(c)}   non-zero words {int((m != 0).sum())}, delayed {st['n_delayed']}, "
          f"unplaced {st['n_unplaced']}, largest delay {st['max_delay']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--skip-repair", action="store_true")
    args = ap.parse_args()
    from path_planning import _hip
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP

    h, R, K, D = 0.2, 0.8, 50, 2
    ctx = _hip.Context(0)
    for N in args.sizes:
        g0, gf, space = generate_grid_swap(N, seed=1000 * N, dim=D)
        s = SCP(N, K * h + 1e-9, h, R, space, dim=D, device=0, verbose=False)
        s.set_initial_states(g0)
        s.set_final_states(gf)
        tr = s.generate_trajectories(max_iterations=15)
        dev = [ctx.tensor(np.ascontiguousarray(tr[k])) for k in ("positions", "velocities", "accelerations")]
        label = f"grid-swap solved ({s.last_info['n_iterations']} it.)"
        for S in (10, 32):
            measure(ctx, N, K, D, h, R, dev, S, args.reps, args.warmup, label)
        for S in (10, 32):
            s.stagger_starts(S)  # warm: workspaces
            t0 = time.perf_counter()
            st = s.stagger_starts(S)
            wall = time.perf_counter() - t0
            print(f"{label:26s} {N:5d} x {K} x {D}  S = {S:2d}  stagger_starts end to end {1e3*wall:.1f} ms (masks "
                  f"{st['lag_conflicts_ms']:.3f} ms, schedule {st['schedule_ms']:.3f} ms): violating segments "
                  f"{st['conflicts_before']} -> {st['conflicts_after']}, {st['n_delayed']} delayed, {st['n_unplaced']} unplaced, "
                  f"largest delay {st['max_delay']}, minimum distance after {st['min_distance_after']:.4f} m", flush=True)
        if not args.skip_repair:
            t0 = time.perf_counter()
            rep = s.repair_conflicts()
            wall = time.perf_counter() - t0
            print(f"{label:26s} {N:5d} x {K} x {D}          repair_conflicts end to end {1e3*wall:.1f} ms: violating segments "
                  f"{rep['conflicts_before']} -> {rep['conflicts_per_pass']}, {rep['passes']} passes, stopped by "
                  f"{rep['stopped_by']}", flush=True)
        del s
    ctx.close()


if __name__ == "__main__":
    main()
