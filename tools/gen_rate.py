"""Scenarios/s of the grid-swap-device generator (scp_generate_grid_swap) against the host generator generate_grid_swap.

Device rows: B = 1, 64, 1024 at N = 128 (2-D and 3-D) and single scenarios at N = 1024 and 4096; each is one batched call
timed with a host clock around it (the call synchronises), after one untimed call of the same shape; the best of `--reps`.
Host rows: generate_grid_swap on the same N / dim, one scenario per call (the host generator has no batch), B' scenarios
timed in a row (B' = min(B, --host-cap)).  Also reports the separation statistics of each device batch.
usage: python tools/gen_rate.py [--reps 5] [--host-cap 16] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))

import numpy as np  # noqa: E402

from path_planning.scenarios import generate_grid_swap, generate_grid_swap_batch  # noqa: E402

CASES = [(128, 2, 1), (128, 2, 64), (128, 2, 1024), (128, 3, 1), (128, 3, 64), (128, 3, 1024), (1024, 2, 1), (4096, 2, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cap", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for N, dim, B in CASES:
        seeds = list(range(1, B + 1))
        generate_grid_swap_batch(N, seeds, dim=dim)  # untimed: code objects, workspace
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, _, _, st = generate_grid_swap_batch(N, seeds, dim=dim)
            best = min(best, time.perf_counter() - t0)
        emit({"gen": "device", "N": N, "dim": dim, "B": B, "sec": best, "scenarios_per_s": B / best,
              "ok": int(st["ok"].sum()), "max_sweeps": int(st["sweeps"].max()), "unmet_blocks": int(st["unmet_blocks"].sum()),
              "conflicts": int(st["conflicts"].sum()), "min_approach_min": float(st["min_approach"].min())})
        hb = min(B, a.host_cap)
        t0 = time.perf_counter()
        for s in seeds[:hb]:
            generate_grid_swap(N, seed=s, dim=dim)
        dt = time.perf_counter() - t0
        emit({"gen": "host", "N": N, "dim": dim, "B": hb, "sec": dt, "scenarios_per_s": hb / dt})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
