"""Times of goal assignment by path length: scp_lattice_distances and scp_assign_costs, and what templating the auction kernel
did to scp_assign_goals.

The map: 181 x 181 cells at stride 1 (32761 lattice nodes) with two long walls; N starts and N goals on free cells drawn from a
seed, N = 256, 1024, 4096.
Rows "lattice-distances" and "assign-costs": device milliseconds between the two events of the call (scp_ctx_last_pair_ms),
after one untimed call of the same shape: the least, the median and the largest of `--reps` calls.  The costs are
path_costs(hops, d2, power=2) of the same points.
Rows "assign-goals" (with --against OTHER_LIB, a libscp_hip.so built from another commit): scp_assign_goals on the same points
through this tree's library and through the other one, both loaded into this process, called through the same few lines of
ctypes and in turn (this, other, this, other, ...), host clock around the synchronising call, after one untimed call each.  this_over_other is the ratio of the two
least times; spread_this / spread_other are (largest - least) / least of each library's own calls, the run-to-run spread a
ratio has to be read against.  The outputs of the two libraries are compared byte for byte.
usage: python tools/assign_paths_times.py [--reps 5] [--sizes 256 1024 4096] [--against OTHER_LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))

import numpy as np  # noqa: E402

from path_planning import _hip  # noqa: E402
from path_planning.scenarios.assignment import hop_totals, path_costs  # noqa: E402
from path_planning.scenarios.grid_swap_device import _context  # noqa: E402

SIDE, CELL = 181, 0.25


def the_map():
    occ = np.zeros((1, SIDE, SIDE), dtype=np.uint8)
    occ[0, 60:, 60] = 1
    occ[0, :120, 120] = 1
    return occ


def points(occ, N, seed):
    """N starts and N goals, each somewhere inside a free cell of its own"""
    rng = np.random.default_rng(seed)
    free = np.argwhere(occ[0] == 0)  # (y, x)
    pick = free[rng.choice(len(free), 2 * N, replace=False)]
    pts = (pick[:, ::-1] + rng.uniform(0.1, 0.9, (2 * N, 2))) * CELL
    return pts[:N], pts[N:]


def summary(ms):
    ms = sorted(ms)
    return {"ms_min": ms[0], "ms_median": ms[len(ms) // 2], "ms_max": ms[-1], "reps": len(ms)}


class Library:
    """scp_assign_goals of one build of the library, called directly: this tree's and another one side by side in one process"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("scp_ctx_create", "scp_ctx_destroy", "scp_assign_goals", "scp_abi_version"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _hip.PROTOTYPES[name]
        assert self.lib.scp_abi_version() == _hip.ABI_VERSION
        self.h = C.c_void_p()
        rc = self.lib.scp_ctx_create(0, None, C.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"scp_ctx_create of {path}: {rc}")

    def assign_goals(self, torch, start, goal):
        B, N, D = (int(v) for v in start.shape)
        goal_of = torch.empty((B, N), dtype=torch.int32, device=start.device)
        prices = torch.empty((B, N), dtype=torch.int64, device=start.device)
        stats = torch.empty(B * _hip.ASSIGN_STATS_DTYPE.itemsize, dtype=torch.uint8, device=start.device)
        rc = self.lib.scp_assign_goals(self.h, B, N, D, start.data_ptr(), goal.data_ptr(), goal_of.data_ptr(), prices.data_ptr(), 0,
                                       stats.data_ptr())
        if rc != 0:
            raise RuntimeError(f"scp_assign_goals: {rc}")
        return goal_of, stats.cpu().numpy().view(_hip.ASSIGN_STATS_DTYPE), prices

    def close(self):
        self.lib.scp_ctx_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--against", default=None, metavar="OTHER_LIB")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    import torch

    ctx = _context(0)
    libs = {"this": Library(_hip.library_path()), "other": Library(a.against)} if a.against else None
    occ = the_map()
    grid = _hip.occupancy_grid(2, [0.0, 0.0], CELL, (SIDE, SIDE))
    _, sat = ctx.occupancy_prepare(2, grid, occ)
    edges = ctx.lattice_edges(2, grid, sat, 1, 0)
    for N in a.sizes:
        p0, pf = points(occ, N, 1000 + N)
        d_p0, d_pf = ctx.tensor(p0), ctx.tensor(pf)
        ms = []
        for rep in range(a.reps + 1):  # (the first call is not timed)
            hops, _, _, _ = ctx.lattice_distances(2, grid, 1, edges, d_p0, d_pf)
            ms.append(ctx.last_pair_ms())
        hops = hops.cpu().numpy().view(np.uint16)
        emit({"row": "lattice-distances", "N": N, "nodes": SIDE * SIDE, **summary(ms[1:]), "max_hops": int(hops[hops != 0xFFFF].max()),
              "n_unreachable": int((hops == 0xFFFF).sum())})
        diff = p0[:, None, :] - pf[None, :, :]
        costs, how = path_costs(hops, (diff * diff).sum(-1), 2)
        d_costs = torch.as_tensor(costs.astype(np.int32)).to(ctx.tdev)[None]
        ms = []
        for rep in range(a.reps + 1):
            goal_of, st, _ = ctx.assign_costs(d_costs)
            ms.append(ctx.last_pair_ms())
        perm = goal_of[0].cpu().numpy()
        emit({"row": "assign-costs", "N": N, **summary(ms[1:]), "tie_bits": how["tie_bits"], "phases": int(st["phases"][0]),
              "rounds": int(st["rounds"][0]), "bids": int(st["bids"][0]), "status": int(st["status"][0]),
              "hops_identity": hop_totals(hops)["sum"], "hops_assigned": hop_totals(hops, perm)["sum"]})
        if libs is None:
            continue
        start, goal = d_p0[None].contiguous(), d_pf[None].contiguous()
        calls = {k: (lambda lib=lib: lib.assign_goals(torch, start, goal)) for k, lib in libs.items()}
        first = {k: fn() for k, fn in calls.items()}  # untimed: code objects, the LDS limit
        (g1, s1, q1), (g2, s2, q2) = first["this"], first["other"]
        same = bool((g1 == g2).all().item() and (q1 == q2).all().item() and s1.tobytes() == s2.tobytes())
        took = {k: [] for k in calls}
        for rep in range(a.reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                took[k].append((time.perf_counter() - t0) * 1e3)
        t, o = summary(took["this"]), summary(took["other"])
        emit({"row": "assign-goals", "N": N, "this": t, "other": o, "this_over_other": t["ms_min"] / o["ms_min"],
              "spread_this": (t["ms_max"] - t["ms_min"]) / t["ms_min"], "spread_other": (o["ms_max"] - o["ms_min"]) / o["ms_min"],
              "same_bytes": same, "rounds": int(s1["rounds"][0])})
    for lib in (libs or {}).values():
        lib.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/assign_paths_times.py --against <libscp_hip.so of the parent commit> --out ...  (MI355X, one GPU; "
                    "see the tool's docstring for what each row times)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
