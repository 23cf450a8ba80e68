"""The case of the shared-path entry points for the tests of what a context carries from one call to the next: a Case of
tests/ctx_state_cases.py (family "obstacle": every scratch workspace is poisoned before every call) that runs
scp_negotiate_paths with and without a path table of the caller's, then scp_path_load and one scp_reference_paths_shared on the
kept set.  register() adds it to that module's table, so that the table's own coverage test finds a case for the three entry
points and the harness of tests/test_ctx_state_gpu.py can run it by name; tests/test_shared_paths_cpu.py and
tests/test_shared_paths_gpu.py register it when they are imported and hold it to the table's criteria themselves.

Nothing here touches the GPU or imports torch at import time."""
import numpy as np

import ctx_state_cases as cs
import shared_path_cases as spc
import shared_path_ref as spr

NAME = "negotiate_paths"
SHARED_ENTRIES = ("scp_negotiate_paths", "scp_path_load", "scp_reference_paths_shared")


def ws_negotiate(N, K, D, nodes, max_path, groups):
    """scp_negotiate_paths without a path table of the caller's (the larger of the two forms): the current set (ref, path, info,
    path_cost), the load, the walks' rows of the largest group and the best set's paths, each part kept to 16 bytes"""
    def part(b):
        return (b + 15) & ~15
    return {"sep_ws": (part(N * (K + 1) * D * 8) + 2 * part(N * max_path * 4) + part(N * 16) + part(N * 4) + part(nodes * 4)
                       + part(-(-N // groups) * max_path * 4),) * 2}


def _info_words(info):
    """records of scp_path_info as their four int32 words"""
    return np.ascontiguousarray(info).view(np.int32).reshape(-1, 4)


def _run(ctx, inp):
    """the negotiation with and without a path table of the caller's, then its pieces: the load of the kept set and one
    re-routing of group 0 under it"""
    c = inp["c"]
    g = cs._grid(c.D, c.origin, c.cell, c.occ)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    out = {}
    for tag, want_path in (("_ws", False), ("", True)):
        ref = ctx.tensor(c.ref_in())
        path, info, path_cost, n_failed, overuse, best_round, n_kept = ctx.negotiate_paths(
            c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, c.share_weight, c.capacity, c.groups, c.rounds,
            want_path=want_path)
        out.update({"ref" + tag: cs._np(ref), "info" + tag: cs._np(info).view(np.int32).reshape(-1, 4)[:c.N].copy(),
                    "path_cost" + tag: cs._np(path_cost).view(np.uint32)[:c.N].copy(), "n_failed" + tag: int(n_failed.item()),
                    "overuse" + tag: cs._np(overuse).view(np.uint64).copy(), "best_round" + tag: int(best_round.item()),
                    "n_kept" + tag: int(n_kept.item())})
    out["path"] = cs._np(path)
    load, over = ctx.path_load(c.N, c.max_path, c.nodes, path, info, c.capacity)
    out.update(load=cs._np(load).view(np.uint32), overuse_kept=int(over.item()))
    n_kept = ctx.reference_paths_shared(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, path, info, path_cost, load,
                                        c.share_weight, c.capacity, c.groups, 0)
    out.update(again_ref=cs._np(ref), again_path=cs._np(path), again_info=cs._np(info).view(np.int32).reshape(-1, 4)[:c.N].copy(),
               again_path_cost=cs._np(path_cost).view(np.uint32)[:c.N].copy(), again_n_kept=int(n_kept.item()))
    return out


def _reference(inp):
    c = inp["c"]
    w = c.negotiate()
    m = c.map()
    load, over = spr.path_load(w["path"], w["info"], c.nodes, c.capacity)
    again = spr.reroute(c.D, c.origin, c.cell, c.dims, c.stride, m["edges"], m["pen"], c.p0, c.pf, c.K, c.max_path, w["ref"], w["path"],
                        w["info"], w["path_cost"], load, c.share_weight, c.capacity, c.groups, 0)
    return dict(want=w, load=load, over=over, again=again)


def _from_ref(ref, inp):
    w, again = ref["want"], ref["again"]
    out = {"path": w["path"], "load": ref["load"], "overuse_kept": int(ref["over"]), "again_ref": again[0], "again_path": again[1],
           "again_info": _info_words(again[2]), "again_path_cost": again[3], "again_n_kept": int(again[5])}
    for tag in ("_ws", ""):
        out.update({"ref" + tag: w["ref"], "info" + tag: _info_words(w["info"]), "path_cost" + tag: w["path_cost"],
                    "n_failed" + tag: int(w["n_failed"]), "overuse" + tag: np.array(w["overuse"], dtype=np.uint64),
                    "best_round" + tag: int(w["best_round"]), "n_kept" + tag: int(w["n_kept"])})
    return out


def _compare(out, ref, inp):
    """tests/test_shared_paths_gpu.py: every output equals the restatement"""
    cs.assert_same_bits(out, _from_ref(ref, inp), "shared paths")


CASE = cs.Case(NAME, "obstacle", SHARED_ENTRIES + cs.PATH_ENTRIES[:2], lambda: dict(c=cs._by_name(spc, "slab_3d")), _run, _reference,
               _from_ref, _compare,
               lambda inp: ws_negotiate(inp["c"].N, inp["c"].K, inp["c"].D, inp["c"].nodes, inp["c"].max_path, inp["c"].groups))


def register():
    """the case into the table of tests/ctx_state_cases.py (once)"""
    if NAME not in cs.CASES_BY_NAME:
        cs.CASES.append(CASE)
        cs.CASES_BY_NAME[NAME] = CASE
    return CASE
