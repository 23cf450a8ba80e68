"""What SCP.repair_conflicts does on the benchmark's scenario and on a small one, and what it costs.

    python tools/repair_times.py [--passes 6] [--sizes 1024 128] [--out profiles/repair_conflicts.txt]

Scenarios: grid-swap N x 50 x 2 with seed 1000 N (N = 1024 is bench.py's), h = 0.2 s, R = 0.8 m.  Per scenario: the plain
solve (wall time of generate_trajectories, SCP iterations), then repair_conflicts: violating segments before and after every
pass, holds, SCP iterations and ADMM steps per pass, cost ratio (sum of squared accelerations after / before), wall time, and
the device time of the two new calls (scp_update_holds per pass, the last scp_apply_holds of every pass; HIP events,
scp_ctx_last_pair_ms).  Solve and repair each run twice from the same state; the second run is the one reported (host clock
around calls that end in a device synchronise; single runs of milliseconds, so read the times as orders of magnitude).
Whether a scenario reaches zero conflicts is reported as found."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ba-path-planning_amd")):
    sys.path.insert(0, p)


def run(N, passes, emit):
    from path_planning.scenarios.position_generator import generate_grid_swap
    from path_planning.solvers.scp import SCP

    h, R, K, D = 0.2, 0.8, 50, 2
    g0, gf, space = generate_grid_swap(N, seed=1000 * N, dim=D)
    s = SCP(N, K * h + 1e-9, h, R, space, dim=D, device=0, verbose=False)
    s.set_initial_states(g0)
    s.set_final_states(gf)
    s.generate_trajectories(max_iterations=15)  # warm-up: allocations, the K x K blocks
    t0 = time.perf_counter()
    s.generate_trajectories(max_iterations=15)
    t_solve = time.perf_counter() - t0
    before = s.validate_solution(continuous=True, conflicts=True)
    emit(f"grid-swap {N} x {K} x {D}, seed {1000 * N}: plain solve {t_solve:.3f} s ({s.last_info['n_iterations']} SCP iterations), "
         f"{before['n_violating_segments']} violating segments in {before['n_conflicts']} conflicts, sample minimum "
         f"{before['min_pair_distance']:.4f} m, continuous minimum {before['min_pair_distance_continuous']:.4f} m")
    kept = {k: v.copy() for k, v in s.trajectories.items()}
    first = s.repair_conflicts(max_passes=passes)  # warm-up: the row planes, the QP workspace, the new kernels' code
    s.trajectories = kept
    rep = s.repair_conflicts(max_passes=passes)
    assert rep["conflicts_per_pass"] == first["conflicts_per_pass"] and rep["holds"] == first["holds"]  # deterministic
    after = s.validate_solution(continuous=True, conflicts=True)
    counts = " -> ".join(str(n) for n in [rep["conflicts_before"]] + rep["conflicts_per_pass"])
    emit(f"  repair: segments {counts}; passes {rep['passes']}, stopped by {rep['stopped_by']}, repaired {rep['repaired']}, holds "
         f"{rep['holds']}, cost ratio {rep['cost_ratio']:.5f}, wall time {rep['time_sec']:.3f} s ({rep['time_sec'] / t_solve:.2f} x the "
         f"plain solve)")
    emit(f"  per pass: SCP iterations {rep['iterations_per_pass']}, ADMM steps {rep['admm_steps_per_pass']}, update_holds "
         f"{['%.4f' % x for x in rep['update_holds_ms']]} ms, apply_holds {['%.4f' % x for x in rep['apply_holds_ms']]} ms")
    emit(f"  after: {after['n_violating_segments']} violating segments, sample minimum {after['min_pair_distance']:.4f} m, "
         f"continuous minimum {after['min_pair_distance_continuous']:.4f} m; violations acc {after['acc_violation']:.2e}, jerk "
         f"{after['jerk_violation']:.2e}, vel {after['vel_violation']:.2e}, pos {after['pos_violation']:.2e}, final position "
         f"{after['final_position_error']:.2e}")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:  # after every line: a run that is cut short leaves what it has
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for N in args.sizes:
        run(N, args.passes, emit)


if __name__ == "__main__":
    main()
