"""Device time of the continuous-time separation check (scp_check_separation) next to the sampled check
(scp_check_avoidance) on the same trajectories, and the share of segments that reached the quartic.

    python tools/separation_times.py [--reps 30] [--warmup 5] [--skip-solves] [--list] [--clearance]

Shapes: 1024 x 50 x 2, 4096 x 50 x 2, 1024 x 50 x 3.  Data: (a) the grid-swap scenario of bench.py, solved trajectories
(QP#0 + SCP iterations, max 15); (b) random kinematically consistent trajectories in a 20^D box (|v| <= 2, |a| <= 15 per
axis).  Times are HIP events around each call's kernels (scp_ctx_last_pair_ms), the two passes alternating in one process:
median, min, quartiles and max over the repetitions after the warm-up.

--list adds the conflict list (scp_list_conflicts) on the same trajectories, alternating with the check in one loop, and a
small shape (128 x 50 x 2).  Its sort is not timed by itself: the call is repeated with capacity 0, which runs the same
pass and the same (then empty) sort launches but stores and sorts nothing, and the difference of the medians is reported
as the share of storing, sorting and gathering the records.

--clearance adds the clearance profile (scp_clearance_profile) on the same trajectories, alternating with the check in one
loop: device time of all its kernels, and the share of segments that reached the quartic for both -- the profile excludes a
segment against the bounds of its two vehicles and its step, the check against one bound for the whole call."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd")):
    sys.path.insert(0, p)


def random_case(N, K, D, seed, h=0.2, side=20.0):
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.0, side, (N, D))
    v0 = rng.uniform(-2.0, 2.0, (N, D))
    acc = np.empty((N, K, D))
    v = v0.copy()
    for k in range(K):
        a = np.clip(rng.uniform(-15.0, 15.0, (N, D)), (-2.0 - v) / h, (2.0 - v) / h)
        acc[:, k] = a
        v = v + h * a
    return p0, v0, acc


def q(x):
    """median, min, max of the timed calls in ms; fmt() prints them in us with the quartiles"""
    return float(np.median(x)), float(np.min(x)), float(np.max(x)), float(np.percentile(x, 25)), float(np.percentile(x, 75))


def fmt(s):
    return f"{s[0]*1e3:8.1f} us (min {s[1]*1e3:.1f}, p25 {s[3]*1e3:.1f}, p75 {s[4]*1e3:.1f}, max {s[2]*1e3:.1f})"


def measure(ctx, N, K, D, h, R, pos, vel, acc, reps, warmup, label):
    t_sep, t_chk = [], []
    for r in range(warmup + reps):
        st = ctx.check_separation(N, K, D, h, R, pos, vel, acc)
        a = ctx.last_pair_ms()
        chk = ctx.check_avoidance(N, K, D, R, pos)
        b = ctx.last_pair_ms()
        if r >= warmup:
            t_sep.append(a)
            t_chk.append(b)
    ctx.check_separation(N, K, D, h, R, pos, vel, acc)
    solved = ctx.last_separation_solved()
    seg = K * N * (N - 1) // 2
    s, c = q(t_sep), q(t_chk)
    print(f"{label:28s} {N:5d} x {K} x {D}  separation {fmt(s)}   "
          f"sampled check {fmt(c)}   ratio {s[0]/c[0]:.2f}   "
          f"quartic: {solved} of {seg} segments ({100.0*solved/seg:.3f} %)   min distance continuous {st['min_dist']:.4f} "
          f"sampled {st['sample_min_dist']:.4f} violating {st['n_violating']}", flush=True)


def measure_listing(ctx, N, K, D, h, R, pos, vel, acc, reps, warmup, label):
    import torch

    from path_planning import _hip

    n = len(ctx.list_conflicts(N, K, D, h, R, pos, vel, acc))
    cap = max(n, 1024)
    out = torch.empty(cap * _hip.CONFLICT_DTYPE.itemsize, dtype=torch.uint8, device=ctx.tdev)
    found = torch.zeros(1, dtype=torch.int64, device=ctx.tdev)
    pairs = N * (N - 1) // 2

    def call(capacity):
        ctx.check(ctx.lib.scp_list_conflicts(ctx.h, N, K, D, h, R, 0, pairs, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                             out.data_ptr(), capacity, found.data_ptr()))
        return ctx.last_pair_ms()

    t_chk, t_full, t_none = [], [], []
    for r in range(warmup + reps):
        ctx.check_separation(N, K, D, h, R, pos, vel, acc)
        a = ctx.last_pair_ms()
        b, c = call(cap), call(0)
        if r >= warmup:
            t_chk.append(a)
            t_full.append(b)
            t_none.append(c)
    k, f, z = q(t_chk), q(t_full), q(t_none)
    print(f"{label:28s} {N:5d} x {K} x {D}  check {fmt(k)}   "
          f"list {fmt(f)}   list, capacity 0 {fmt(z)}   list / check {f[0]/k[0]:.2f}   store + sort + gather "
          f"{(f[0]-z[0])*1e3:.1f} us = {100.0*(f[0]-z[0])/f[0]:.1f} % of the list   records {n} (capacity {cap})", flush=True)


def measure_clearance(ctx, N, K, D, h, R, pos, vel, acc, reps, warmup, label):
    t_chk, t_clr = [], []
    for r in range(warmup + reps):
        st = ctx.check_separation(N, K, D, h, R, pos, vel, acc)
        a = ctx.last_pair_ms()
        veh, step = ctx.clearance_profile(N, K, D, h, R, pos, vel, acc)
        b = ctx.last_pair_ms()
        if r >= warmup:
            t_chk.append(a)
            t_clr.append(b)
    solved_clr = ctx.last_clearance_solved()
    ctx.check_separation(N, K, D, h, R, pos, vel, acc)
    solved_chk = ctx.last_separation_solved()
    seg = K * N * (N - 1) // 2
    assert step["min_dist"].min() == veh["min_dist"].min() == st["min_dist"] and int(step["n_violating"].sum()) == st["n_violating"]
    k, c = q(t_chk), q(t_clr)
    print(f"{label:28s} {N:5d} x {K} x {D}  check {fmt(k)}   "
          f"clearance profile {fmt(c)}   profile / check {c[0]/k[0]:.2f}   "
          f"quartic: check {solved_chk} of {seg} segments ({100.0*solved_chk/seg:.3f} %), profile {solved_clr} "
          f"({100.0*solved_clr/seg:.3f} %)   vehicles in conflict {int((veh['n_violating'] > 0).sum())} of {N}, smallest "
          f"clearance {veh['min_dist'].min():.4f}, median {float(np.median(veh['min_dist'])):.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--list", action="store_true", help="also time scp_list_conflicts, and add the shape 128 x 50 x 2")
    ap.add_argument("--clearance", action="store_true", help="also time scp_clearance_profile beside the check")
    args = ap.parse_args()
    from path_planning import _hip
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP

    h, R, K = 0.2, 0.8, 50
    ctx = _hip.Context(0)
    for N, D in ((1024, 2), (4096, 2), (1024, 3)) + (((128, 2),) if args.list else ()):
        p0, v0, acc = random_case(N, K, D, 100 + N + D)
        a = ctx.tensor(acc)
        pos, vel = ctx.kinematics(N, K, D, h, a, ctx.tensor(p0), ctx.tensor(v0))
        measure(ctx, N, K, D, h, R, pos, vel, a, args.reps, args.warmup, "random, 20^D box")
        if args.list:
            measure_listing(ctx, N, K, D, h, R, pos, vel, a, args.reps, args.warmup, "random, 20^D box")
        if args.clearance:
            measure_clearance(ctx, N, K, D, h, R, pos, vel, a, args.reps, args.warmup, "random, 20^D box")
        if args.skip_solves:
            continue
        g0, gf, space = generate_grid_swap(N, seed=1000 * N, dim=D)
        s = SCP(N, K * h + 1e-9, h, R, space, dim=D, device=0, verbose=False)
        s.set_initial_states(g0)
        s.set_final_states(gf)
        tr = s.generate_trajectories(max_iterations=15)
        dev = [ctx.tensor(np.ascontiguousarray(tr[k])) for k in ("positions", "velocities", "accelerations")]
        measure(ctx, N, K, D, h, R, *dev, args.reps, args.warmup,
                f"grid-swap solved ({s.last_info['n_iterations']} it.)")
        if args.list:
            measure_listing(ctx, N, K, D, h, R, *dev, args.reps, args.warmup,
                            f"grid-swap solved ({s.last_info['n_iterations']} it.)")
        if args.clearance:
            measure_clearance(ctx, N, K, D, h, R, *dev, args.reps, args.warmup,
                              f"grid-swap solved ({s.last_info['n_iterations']} it.)")
        del s
    ctx.close()


if __name__ == "__main__":
    main()
