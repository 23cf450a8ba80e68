"""Device time of the order search of the staggered starts: ONE scp_schedule_starts_batch call with B candidate orders next to B
sequential scp_schedule_starts calls (the kernel as it was before the batch call existed) on the same masks and orders, and
SCP.stagger_starts with and without the search end to end.

    python tools/stagger_search_times.py [--reps 20] [--warmup 3] [--sizes 1024 4096] [--batches 1 16 64 256 1024] [--both-reads] [--skip-end-to-end]

Masks: (a) scp_lag_conflicts of the grid-swap scenario of bench.py after a solve (QP#0 + SCP iterations, max 15), N x 50 x 2,
S = 10 -- few non-zero words; (b) random words, every bit 0 .. S of every off-diagonal word set with probability 1.5 / N -- most
vehicles delayed, some unplaced.  Orders: candidate_orders(N, B, default_rng(N)).  Times are HIP events around each call's device
work (scp_ctx_last_pair_ms), the batch call and the B single calls alternating in one loop of one process: median, min,
quartiles and max over the repetitions after the warm-up.  The sequential side is a sum over B calls, so from B = 256 on it is
repeated max(3, 1280 // B) times instead of --reps (at 4096 vehicles 1024 single calls take 13 s).  Every candidate's delays of
the batch are compared with the single calls' once per line.  The last lines per mask repeat B = 256 with 256 and with 1024
threads per workgroup ("stg_batch_threads") and, with --both-reads, every B with the masks' columns read directly and from the
transposed copy ("stg_batch_transposed" 0 and 1: the transposing launch is inside the timed window; the call itself chooses the
copy from 16 candidates on).  The end-to-end figures are host wall clock of one warm call each."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from separation_times import fmt, q  # noqa: E402


def random_mask(ctx, N, S):
    import torch

    gen = torch.Generator(device=ctx.tdev).manual_seed(N)
    mask = torch.zeros((N, N), dtype=torch.int64, device=ctx.tdev)
    for s in range(S + 1):
        mask |= (torch.rand((N, N), device=ctx.tdev, generator=gen) < 1.5 / N).to(torch.int64) << s
    mask.fill_diagonal_(0)
    return mask


def measure(ctx, mask, S, orders, reps, warmup, label, sequential=True):
    """orders: (B, N) int32 device tensor.  Returns (batch median ms, sequential median ms or None)."""
    B, N = orders.shape
    seq_reps = reps if B < 256 else max(3, 1280 // B)
    t_batch, t_seq = [], []
    for r in range(warmup + reps):
        delays, stats, best = ctx.schedule_starts_batch(mask, S, orders)
        a = ctx.last_pair_ms()
        if r >= warmup:
            t_batch.append(a)
        if not sequential or (r >= warmup and len(t_seq) >= seq_reps):
            continue
        total = 0.0
        for b in range(B if r >= warmup else min(B, 16)):  # (warm-up: the kernel is loaded after one call)
            d, st = ctx.schedule_starts(mask, S, orders[b])
            total += ctx.last_pair_ms()
            if r == 0:
                assert d.tobytes() == delays[b].tobytes() and st["total_delay"] == int(stats["total_delay"][b]), (label, b)
        if r >= warmup:
            t_seq.append(total)
    a = q(t_batch)
    u = stats["n_unplaced"]
    line = (f"{label:24s} {N:5d}  S = {S:2d}  B = {B:4d}  batch {fmt(a)}  per candidate {1e3*a[0]/B:8.1f} us   unplaced "
            f"{int(u.min())} .. {int(u[0])} (index order) .. {int(u.max())}, best {best}")
    if not sequential:
        print(line, flush=True)
        return a[0], None
    b = q(t_seq)
    print(f"{line}   {B} single calls {fmt(b)} ({len(t_seq)} reps)  per call {1e3*b[0]/B:8.1f} us   sequential / batch "
          f"{b[0]/a[0]:.1f}", flush=True)
    return a[0], b[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--both-reads", action="store_true",
                    help="repeat every B with the masks' columns read directly and from the transposed copy")
    args = ap.parse_args()
    import torch

    from path_planning import _hip
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP
    from path_planning.solvers.stagger import candidate_orders

    h, R, K, D, S = 0.2, 0.8, 50, 2, 10
    ctx = _hip.Context(0)
    for N in args.sizes:
        g0, gf, space = generate_grid_swap(N, seed=1000 * N, dim=D)
        s = SCP(N, K * h + 1e-9, h, R, space, dim=D, device=0, verbose=False)
        s.set_initial_states(g0)
        s.set_final_states(gf)
        tr = s.generate_trajectories(max_iterations=15)
        dev = [ctx.tensor(np.ascontiguousarray(tr[k])) for k in ("positions", "velocities", "accelerations")]
        solved = ctx.lag_conflicts(N, K, D, h, R, *dev, S, device=True)
        orders = torch.as_tensor(candidate_orders(N, max(args.batches + [256]), np.random.default_rng(N))).to(ctx.tdev)
        for label, mask in ((f"grid-swap solved ({s.last_info['n_iterations']} it.)", solved), ("random 1.5 / N", random_mask(ctx, N, S))):
            words = int((mask != 0).sum())
            print(f"# {label}, N = {N}: {words} non-zero mask words", flush=True)
            for B in args.batches:
                measure(ctx, mask, S, orders[:B].contiguous(), args.reps, args.warmup, label)
            for threads in (256, 1024):
                ctx.set_option("stg_batch_threads", threads)
                measure(ctx, mask, S, orders[:256].contiguous(), args.reps, args.warmup, f"{label[:9]} {threads} threads", sequential=False)
            ctx.set_option("stg_batch_threads", 0)
            for transposed, name in ((0, "direct"), (1, "transposed")) if args.both_reads else ():
                ctx.set_option("stg_batch_transposed", transposed)
                for B in args.batches:
                    measure(ctx, mask, S, orders[:B].contiguous(), args.reps, args.warmup, f"{label[:9]} {name}", sequential=False)
            ctx.set_option("stg_batch_transposed", -1)
        if not args.skip_end_to_end:
            for kw in ({}, {"search": 256, "rounds": 4}):
                s.stagger_starts(S, **kw)  # warm: workspaces
                t0 = time.perf_counter()
                st = s.stagger_starts(S, **kw)
                wall = time.perf_counter() - t0
                se = st.get("search")
                print(f"grid-swap solved         {N:5d}  S = {S:2d}  stagger_starts({', '.join(f'{k}={v}' for k, v in kw.items())}) end to end "
                      f"{1e3*wall:.1f} ms (masks {st['lag_conflicts_ms']:.3f} ms, schedule {st['schedule_ms']:.3f} ms): violating "
                      f"segments {st['conflicts_before']} -> {st['conflicts_after']}, {st['n_delayed']} delayed, {st['n_unplaced']} "
                      f"unplaced, largest delay {st['max_delay']}, total delay {st['total_delay']}"
                      + (f"; best: candidate {se['best_candidate']} of round {se['best_round']} of {se['rounds_run']}, improved "
                         f"{se['improved']}" if se else ""), flush=True)
        del s
    ctx.close()


if __name__ == "__main__":
    main()
