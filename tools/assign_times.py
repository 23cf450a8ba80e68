"""Times of the goal assignment (scp_assign_goals) and what it does to the SCP solve.

Rows "assign": one batched call, host clock around it (the call synchronises), after one untimed call of the same shape; the
best of `--reps`.  B = 1 at N = 128, 1024, 4096 on uniform points and on grid-swap-device scenarios, B = 4096 at N = 128.
Beside each B = 1 row scipy's linear_sum_assignment on the same quantised costs on the host, where scipy is importable
(otherwise the row says so); its optimum must equal cost_q.
Rows "solve": SCP iterations and wall time of generate_trajectories on grid-swap scenarios (host generator) of 128 and 1024
agents, with the given pairing and after SCP.assign_goals (T = 10 s, h = 0.2 s, R = 0.8 m, the batch CLI's configuration).
--wide: only the rows "assign-wide" (see wide_rows): scp_assign_goals against scp_assign_goals_wide, and wide alone beyond 4096.
usage: python tools/assign_times.py [--reps 3] [--out FILE] [--skip-solves] [--wide]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import assignment_ref  # noqa: E402  (the quantised costs for scipy)
from path_planning.scenarios import generate_grid_swap, generate_grid_swap_batch  # noqa: E402
from path_planning.scenarios.grid_swap_device import _context  # noqa: E402
from path_planning.solvers.scp import SCP  # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment
except ImportError:
    linear_sum_assignment = None


def scenarios(kind, N, B):
    if kind == "uniform":
        rng = np.random.default_rng(N + B)
        side = 2.0 * np.sqrt(N)  # the density of the grid-swap family (pitch 2 m)
        return rng.uniform(0.0, side, (B, N, 2)), rng.uniform(0.0, side, (B, N, 2))
    init, goal, _, _ = generate_grid_swap_batch(N, list(range(1, B + 1)), dim=2)
    return init.cpu().numpy(), goal.cpu().numpy()


def wide_rows(ctx, emit, reps):
    """Rows "assign-wide": scp_assign_goals and scp_assign_goals_wide on the same scenarios, alternating in one loop (the
    best of `reps` each, after one untimed call each), their outputs compared byte for byte; beyond 4096 vehicles wide alone
    (uniform and grid-swap-device points at 16384, a jittered grid with 1/16 of its goals permuted at 16384 and 65536)."""
    import assignment_wide_cases

    def timed(fn, start, goal):
        t0 = time.perf_counter()
        out = fn(start, goal, want_prices=True)
        return time.perf_counter() - t0, out

    shapes = [(kind, N, B) for N, B in ((128, 1), (1024, 1), (4096, 1), (128, 4096)) for kind in ("uniform", "grid-swap-device")]
    shapes += [("jittered-grid", 16384, 1), ("jittered-grid", 65536, 1), ("grid-swap-device", 16384, 1), ("uniform", 16384, 1)]
    for kind, N, B in shapes:
        if kind == "jittered-grid":
            pts = [x[None] for x in assignment_wide_cases.jittered_grid(N, 11, swaps=N // 16)]
        else:
            pts = scenarios(kind, N, B)
        start, goal = (ctx.tensor(x) for x in pts)
        methods = {"wide": ctx.assign_goals_wide}
        if N <= 4096:
            methods["single"] = ctx.assign_goals
        first = {m: timed(fn, start, goal) for m, fn in methods.items()}  # untimed: code objects, LDS limit, workspace
        n = reps if max(t for t, _ in first.values()) < 5.0 else 1
        best = {m: float("inf") for m in methods}
        for _ in range(n):
            for m, fn in methods.items():
                best[m] = min(best[m], timed(fn, start, goal)[0])
        st = first["wide"][1][1]
        row = {"row": "assign-wide", "points": kind, "N": N, "B": B, "reps": n, "wide_ms": best["wide"] * 1e3,
               "phases_max": int(st["phases"].max()), "rounds_max": int(st["rounds"].max()), "bids_max": int(st["bids"].max()),
               "status_nonzero": int((st["status"] != 0).sum())}
        if "single" in methods:
            (g1, s1, p1), (g2, s2, p2) = first["single"][1], first["wide"][1]
            row.update(single_ms=best["single"] * 1e3, single_over_wide=best["single"] / best["wide"],
                       same_bytes=bool((g1 == g2).all().item() and (p1 == p2).all().item() and s1.tobytes() == s2.tobytes()))
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--wide", action="store_true", help="only the rows that compare scp_assign_goals_wide with scp_assign_goals")
    a = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    ctx = _context(0)
    if a.wide:
        wide_rows(ctx, emit, a.reps)
        if a.out:
            with open(a.out, "w") as f:
                f.write("# python tools/assign_times.py --wide --out ...  (MI355X, one GPU; single and wide alternate in one loop: "
                        "best of `reps` calls each after one untimed call each, host clock around the synchronising call)\n")
                f.write("\n".join(lines) + "\n")
        return
    for N, B in ((128, 1), (128, 4096), (1024, 1), (4096, 1)):
        for kind in ("uniform", "grid-swap-device"):
            start, goal = (ctx.tensor(x) for x in scenarios(kind, N, B))
            ctx.assign_goals(start, goal)  # untimed: code object, LDS limit
            best = float("inf")
            for _ in range(a.reps):
                t0 = time.perf_counter()
                goal_of, st, _ = ctx.assign_goals(start, goal)
                best = min(best, time.perf_counter() - t0)
            line = ctx.straight_line_check(start, goal, goal_of, 0.3)
            before = ctx.straight_line_check(start, goal, None, 0.3)
            emit({"row": "assign", "points": kind, "N": N, "B": B, "ms_per_call": best * 1e3, "scenarios_per_s": B / best,
                  "phases_max": int(st["phases"].max()), "rounds_mean": float(st["rounds"].mean()),
                  "rounds_max": int(st["rounds"].max()), "bids_mean": float(st["bids"].mean()),
                  "status_nonzero": int((st["status"] != 0).sum()),
                  "cost_ratio_mean": float((st["cost_q"] / np.maximum(st["cost_q_identity"], 1)).mean()),
                  "opposed_before_mean": float(before["n_opposed"].mean()), "opposed_after_max": int(line["n_opposed"].max()),
                  "min_approach_before_min": float(before["min_approach"].min()),
                  "min_approach_after_min": float(line["min_approach"].min())})
            if B == 1:
                if linear_sum_assignment is None:
                    emit({"row": "host-lsa", "points": kind, "N": N, "note": "scipy is not importable here"})
                else:
                    c, _, _ = assignment_ref.quantise(start[0].cpu().numpy(), goal[0].cpu().numpy())
                    t0 = time.perf_counter()
                    r, col = linear_sum_assignment(c)
                    dt = time.perf_counter() - t0
                    emit({"row": "host-lsa", "points": kind, "N": N, "ms": dt * 1e3,
                          "same_optimum": bool(int(c[r, col].sum()) == int(st["cost_q"][0]))})
    if not a.skip_solves:
        for N in (128, 1024):
            init, goal, space = generate_grid_swap(N, seed=1)
            for assign in (False, True):
                solver = SCP(n_vehicles=N, time_horizon=10.0, time_step=0.2, min_distance=0.8, space_dims=space, device=0,
                             verbose=False)
                row = {"row": "solve", "scenario": "grid-swap seed 1", "N": N, "assign_goals": assign}
                for rep in range(2):  # (the second solve of the object: kernels loaded, workspaces built)
                    solver.set_initial_states(init)
                    solver.set_final_states(goal)
                    if assign:
                        t0 = time.perf_counter()
                        solver.assign_goals()
                        row["assign_ms"] = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    solver.generate_trajectories(max_iterations=15)
                    row["solve_ms"] = (time.perf_counter() - t0) * 1e3
                info = solver.last_info
                row.update(scp_iterations=int(info["n_iterations"]), initially_feasible=bool(info["initially_feasible"]),
                           converged=bool(info["converged"]),
                           min_pair_distance=float(solver.validate_solution()["min_pair_distance"]))
                if assign:
                    ai = solver.assignment_info
                    row.update(opposed_before=ai["line_before"]["n_opposed"], opposed_after=ai["line_after"]["n_opposed"],
                               line_min_approach_before=ai["line_before"]["min_approach"],
                               line_min_approach_after=ai["line_after"]["min_approach"])
                emit(row)
                solver.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/assign_times.py --out ...  (MI355X, one GPU; assign rows: best of 3 calls after one untimed "
                    "call of the same shape, host clock around the synchronising call; host-lsa: scipy on the same box)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
