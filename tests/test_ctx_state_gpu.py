"""No result may depend on what its context ran before.  Every stateless entry point works through a context that owns device
memory shared between entry points and outliving the call ("What a context owns"); the product runs whole chains of
them on one pooled context.  The cases of tests/ctx_state_cases.py run here on contexts that have a history: larger calls before
them, every scratch workspace poisoned between calls (scp_ctx_debug_fill), their neighbours in the shared workspace, early exits,
other sizes, another stream.

The baseline is fresh[case]: the case's outputs on a newly created context, held to the CPU reference by the criterion the
family's own test file uses.  Everything else is compared with it BIT FOR BIT in the canonical form of the case table: the
library has no floating-point atomics, and the suite already asserts bit identity across forced forks of the same calls.  After
every call scp_ctx_debug_state must show the words the next call relies on: the tickets of the one-launch passes, of the QP's
checks and row build and of scp_rel_step at zero, and the violations passes' scratch bitmap all zero."""
import numpy as np
import pytest

import ctx_state_cases as cs

pytestmark = pytest.mark.gpu

_FRESH = {}
SIZES = ("tm_bytes", "cmp_map_bytes", "cmp_tot_bytes", "wg_rows_bytes", "gen_ws_bytes", "sep_ws_bytes", "asg_ws_bytes", "asgw_ws_bytes",
         "rast_ws_bytes", "rast_host_bytes")


def new_context():
    from path_planning import _hip

    return _hip.Context(0)


def assert_invariants(ctx, label):
    st = ctx.debug_state()
    assert st["ticket"][:3] == [0, 0, 0], (label, st["ticket"])
    assert st["rel_ticket"] == 0, (label, st["rel_ticket"])
    assert st["cmp_map_nonzero"] == 0, (label, st["cmp_map_nonzero"])
    return st


def fresh(name):
    """the case on a newly created context (torch's default stream), held to its CPU reference; made once"""
    if name not in _FRESH:
        case = cs.CASES_BY_NAME[name]
        ctx = new_context()
        try:
            out = case.run(ctx)
            assert_invariants(ctx, f"{name} on a new context")
        finally:
            ctx.close()
        # what the coverage test of tests/test_ctx_state_cpu.py takes the case's word for: every entry point it names was called
        unseen = sorted(set(case.entries) - case.called)
        assert not unseen, f"{name} names entry points it never calls: {unseen}"
        case.compare(out, case.ref(), case.inputs())
        _FRESH[name] = out
    return _FRESH[name]


def check(ctx, name, label, poison=None):
    """the case on a context with a history: the bits of the fresh context, the invariants afterwards"""
    want = fresh(name)
    out = cs.CASES_BY_NAME[name].run(ctx, poison=poison)
    cs.assert_same_bits(out, want, f"{name} {label}")
    return assert_invariants(ctx, f"{name} {label}")


@pytest.fixture
def ctx():
    c = new_context()
    yield c
    c.close()


# ---- 0. the baseline -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.CASES_BY_NAME))
def test_fresh_context_gives_the_reference(name):
    fresh(name)


# ---- 1. poisoned workspaces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.CASES_BY_NAME))
def test_poisoned_workspaces(ctx, name):
    """After the family's grower every shared buffer is larger than the case needs, so no reallocation hides what is in it.  All
    ones read as NaN as a double, -1 as an int and the identity of no minimum, maximum or sum; with 1 in every word a counter or
    partial that only works from zero comes out one off."""
    case = cs.CASES_BY_NAME[name]
    cs.GROWERS[case.family].run(ctx)
    grown = assert_invariants(ctx, f"{name}: after the grower")
    for buf, (low, high) in cs.GROWERS[case.family].ws().items():
        key = buf if buf.endswith("_bytes") else buf + "_bytes"
        assert grown[key] >= low, (key, grown[key], low)  # the size table of the cases states what the library allocates
    for word in (0xFFFFFFFF, 0x00000001):  # (before every call of the case where its family is a chain of stateless calls)
        st = check(ctx, name, f"after debug_fill({word:#x})", poison=word)
        assert {k: st[k] for k in SIZES} == {k: grown[k] for k in SIZES}, "the case needed more of a buffer than its grower left"


# ---- 2. neighbours in the shared workspace ----------------------------------------------------------------------------------------------
def permuted_order():
    """a seeded permutation of the twelve users that puts the largest layout directly before the smallest"""
    need = {n: cs.CASES_BY_NAME[n].ws()["sep_ws"] for n in cs.PRODUCT_ORDER}
    largest = max(need, key=lambda n: need[n][0])
    smallest = min(need, key=lambda n: need[n][1])
    assert largest != smallest and need[largest][0] > need[smallest][1]
    rng = np.random.default_rng(2024)
    rest = [n for n in cs.PRODUCT_ORDER if n not in (largest, smallest)]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    at = int(rng.integers(0, len(rest) + 1))
    return rest[:at] + [largest, smallest] + rest[at:]


BETWEEN = ("trajectory", "pair33", "qp_lean")  # scp_rel_step, a one-launch pairwise pass, QP.solve: ticket words 0, 1 and 2 alternate


@pytest.mark.parametrize("order", ["product", "permuted"])
def test_neighbours_in_the_shared_workspace(ctx, order):
    names = list(cs.PRODUCT_ORDER) if order == "product" else permuted_order()
    assert sorted(names) == sorted(cs.SEP_WS_USERS.values())
    print(f"{order}: {names}")
    for i, name in enumerate(names):
        check(ctx, name, f"as user {i} of the {order} order")
        if i + 1 < len(names):
            check(ctx, BETWEEN[i % 3], f"between users {i} and {i + 1} of the {order} order")


# ---- 3. counters that sit side by side --------------------------------------------------------------------------------------------------
def test_counters_side_by_side(ctx):
    import test_near_violations_gpu as tn

    users = (("check_separation", ctx.last_separation_solved, (12, 13)), ("clearance_profile", ctx.last_clearance_solved, (14, 15)),
             ("delay_margins", ctx.last_delay_solved, (10, 11)), ("lag_conflicts", ctx.last_lag_solved, (8, 9)))
    counts = {name: fresh(name)["solved"] for name, _, _ in users}
    print(f"solved counts: {counts}")
    assert len(set(counts.values())) == 4 and min(counts.values()) > 0, counts  # (a condition on the inputs of the four cases)

    def words_of(st):
        return st["ticket"]

    own = {}
    for name, read, mine in users:
        before = words_of(ctx.debug_state())
        after = words_of(check(ctx, name, "before the other counters"))
        own[name] = read()
        changed = [w for w in range(16) if after[w] != before[w]]
        assert set(changed) <= set(mine) and after[mine[0]] + (after[mine[1]] << 32) == own[name], (name, before, after)
    assert own == counts
    assert {name: read() for name, read, _ in users} == own  # all four after the last call
    before = words_of(ctx.debug_state())
    for name, _, (lo, hi) in users:
        assert before[lo] + (before[hi] << 32) == own[name], (name, before)
    check(ctx, "schedule_starts_batch", "beside the counters")  # words 4 .. 7
    after = words_of(ctx.debug_state())
    changed = [w for w in range(16) if after[w] != before[w]]
    assert set(changed) <= {4, 5, 6, 7} and changed, (before, after)
    # the near form of the violations pass: word 3 takes the number of a call that staged a value that was not finite
    try:
        for case_name, falls_back in (("n33_2d", 0), ("nan", 1)):
            c = tn.make_case(case_name)
            N, K, D = c["prev"].shape
            got = tn.run_pass(ctx, 2, ctx.tensor(c["prev"]), ctx.tensor(c["new"]), N, K, D, (0, N * (N - 1) // 2), 1e-6, 1 << 16, None)
            assert got["near"] == 1 and got["fell_back"] == falls_back and not got["scratch"].any()
    finally:
        ctx.set_near_pass(1)
    last = words_of(assert_invariants(ctx, "after the near passes"))
    changed = [w for w in range(16) if last[w] != after[w]]
    assert changed == [3] and last[3] != 0, (after, last)
    assert {name: read() for name, read, _ in users} == own


# ---- 4. early exits leave the context usable --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.PAIR_SHAPES))
def test_a_row_list_that_is_too_short(ctx, name):
    """the overflow paths of tests/test_kernels_gpu.py in the one-launch, the one-workgroup-compaction and the three-launch form:
    nothing is merged, the count is reported -- and the scratch bitmap is clean, the tickets are back at zero"""
    import torch

    from path_planning import _hip

    single = cs.PAIR_SHAPES[name][4]
    inp = cs.CASES_BY_NAME[name].inputs()
    want = fresh(name)
    prob = inp["prob"]
    N, K, D = prob.N, prob.K, prob.D
    pos, new, p0, v0 = (ctx.tensor(a) for a in (inp["pos"], inp["pos_new"], prob.p0, prob.v0))
    if not single:
        ctx.lib.scp_ctx_set_option(ctx.h, b"single_launch_passes", 0)
    try:
        pp = _hip.PairPass(ctx, N, K, D, prob.R, prob.h)
        pp.linearize(pos, p0, v0, cs.MARGIN)
        bitmap0 = pp.bitmap.clone()
        sel = torch.full((2,), -1, dtype=torch.int64, device=ctx.tdev)
        calls = (lambda: ctx.lib.scp_collision_violations_at(ctx.h, N, K, D, prob.R, 0, prob.pairs, pos.data_ptr(), new.data_ptr(), cs.FEAS,
                                                             sel.data_ptr(), 2, pp.bitmap.data_ptr(), ctx.stats.data_ptr()),
                 lambda: ctx.lib.scp_collision_violations(ctx.h, N, K, D, prob.h, 0, prob.pairs, pp.eta.data_ptr(), pp.l.data_ptr(),
                                                          new.data_ptr(), p0.data_ptr(), v0.data_ptr(), cs.FEAS, sel.data_ptr(), 2,
                                                          pp.bitmap.data_ptr(), ctx.stats.data_ptr()))
        for call in calls:
            ctx.check(call())
            _, _, n_sel, _ = ctx.read_stats()
            assert n_sel == want["new_rows"].size > 2  # more rows than the list holds
            assert torch.equal(pp.bitmap, bitmap0)     # nothing merged
            assert_invariants(ctx, f"{name}: after a list that was too short")
    finally:
        if not single:
            ctx.lib.scp_ctx_set_option(ctx.h, b"single_launch_passes", 1)
    check(ctx, name, "after a list that was too short")


def test_a_conflict_list_that_is_too_short(ctx):
    import torch

    from path_planning import _hip

    inp = cs.CASES_BY_NAME["list_conflicts"].inputs()
    pos, vel, acc = cs._dev(ctx, inp["host"])
    N, K, D = pos.shape
    cap = 3
    out = torch.zeros(cap * _hip.CONFLICT_DTYPE.itemsize, dtype=torch.uint8, device=ctx.tdev)
    n_found = torch.zeros(1, dtype=torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.scp_list_conflicts(ctx.h, N, K, D, cs.H, cs.R_SEP, 0, N * (N - 1) // 2, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                         out.data_ptr(), cap, n_found.data_ptr()))
    assert int(n_found.item()) == fresh("list_conflicts")["list"].size > cap
    assert_invariants(ctx, "after a conflict list that was too short")
    for name in ("list_conflicts", "check_separation", "clearance_profile"):
        check(ctx, name, "after a conflict list that was too short")


def test_a_hold_table_that_is_too_small(ctx):
    case = cs.CASES_BY_NAME["update_holds"]
    inp = case.inputs()
    with cs.canary_outputs():
        got = cs._upd_run(ctx, inp, capacity=inp["start"].size + 1)
    assert got["needed"] == fresh("update_holds")["needed"] > inp["start"].size + 1
    assert got["table"].tobytes() == inp["start"].tobytes()  # untouched, the size needed reported
    assert_invariants(ctx, "after a hold table that was too small")
    for name in ("update_holds", "apply_holds"):
        check(ctx, name, "after a hold table that was too small")


def test_a_search_that_cannot_reach_the_goal(ctx):
    """max_path one node too short: status 4 for the vehicles concerned, their rows of ref untouched"""
    c = cs._by_name(cs.rpc, "max_path_short")
    want = c.want()
    assert (want["info"]["status"] == 4).any() and want["n_failed"] > 0
    with cs.canary_outputs():
        got = cs._paths_run(ctx, dict(c=c))
    for k in ("info", "info_ws"):
        np.testing.assert_array_equal(got[k], want["info"])
    for k in ("ref", "ref_ws"):
        np.testing.assert_array_equal(got[k].view(np.uint64), want["ref"].view(np.uint64))
    assert got["n_failed"] == got["n_failed_ws"] == want["n_failed"]
    assert_invariants(ctx, "after a search that failed")
    for name in ("reference_paths", "reference_paths_weighted", "shorten_paths"):
        check(ctx, name, "after a search that failed")


def test_a_rasterise_call_rejected_after_a_successful_one(ctx):
    from path_planning import _hip

    check(ctx, "rasterize", "first")
    c = cs.CASES_BY_NAME["rasterize"].inputs()["c"]
    with pytest.raises(_hip.HipError, match="rasterize_shapes"):
        from path_planning.scenarios.obstacles import pack_shapes

        ctx.rasterize_shapes(c.D, _hip.occupancy_grid(c.D, c.origin, c.cell, c.dims), pack_shapes(c.D, **c.shapes()), float("nan"))
    assert_invariants(ctx, "after a rejected rasterise call")
    check(ctx, "rasterize", "after a rejected call")


def test_an_auction_stopped_by_its_round_guard(ctx):
    start, goal = cs.asr.identical_goals(64)
    ref = cs.asr.auction(start, goal, max_rounds_per_phase=1)
    for fn in (ctx.assign_goals, ctx.assign_goals_wide):
        goal_of, st, prices = fn(start, goal, max_rounds_per_phase=1, want_prices=True)
        assert st["status"][0] == 1 == ref["status"] and goal_of.cpu().numpy()[0].tolist() == list(range(64))
        np.testing.assert_array_equal(prices.cpu().numpy()[0], ref["prices"])
    assert_invariants(ctx, "after a stopped auction")
    for name in ("assign_goals", "assign_goals_wide", "assign_costs"):
        check(ctx, name, "after a stopped auction")


def test_a_qp_stopped_at_max_iter(ctx):
    inp = cs.CASES_BY_NAME["qp_lean"].inputs()
    out = cs._qp_lean_run(ctx, inp, max_iter=25)
    assert out["info"]["iter"] == 25 and out["info"]["status_val"] in (2, -2), out["info"]
    assert fresh("qp_lean")["info"]["iter"] > 25
    assert_invariants(ctx, "after a QP stopped at max_iter")
    for name in ("qp_lean", "qp_generic"):
        check(ctx, name, "after a QP stopped at max_iter")


def test_a_persistent_solve_that_gives_up(ctx):
    """the existing switch of tests/test_qp_gpu.py: the persistent launch times out in its bounded spins, leaves without writing
    state back, and the solve is finished by the launches of the generic path"""
    inp = cs.CASES_BY_NAME["qp_lean"].inputs()
    out = cs._qp_lean_run(ctx, inp, fault=True)
    want = fresh("qp_lean")
    assert out["info"]["persist_gave_up"] == 1 and not out["info"]["pipeline"].startswith("persistent"), out["info"]
    assert out["info"]["status_val"] == 1 and out["info"]["iter"] == want["info"]["iter"]
    np.testing.assert_allclose(out["x"], want["x"], rtol=0, atol=1e-8)
    assert_invariants(ctx, "after a persistent solve that gave up")
    for name in ("qp_lean", "qp_generic", "solver_step"):
        check(ctx, name, "after a persistent solve that gave up")


# ---- 5. size changes --------------------------------------------------------------------------------------------------------------------
def test_pairwise_sizes_down_and_up(ctx):
    for i, name in enumerate(("pair700", "pair33", "pair300", "pair700")):
        check(ctx, name, f"as step {i} of 700 -> 33 -> 300 -> 700")


def test_distance_field_sizes_down_and_up(ctx):
    for i, name in enumerate(("field_3d", "field_2d", "field_row", "field_3d")):
        check(ctx, name, f"as step {i} of 3-D -> 2-D -> one row -> 3-D")
    assert cs.CASES_BY_NAME["field_row"].ws()["sep_ws"] == (0, 0)


# ---- 6. two contexts, two streams, one thread ---------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams():
    """fresh was made on the default stream: this also holds the whole chain to stream-ordered behaviour on a side stream, with
    inputs and outputs produced and consumed on the owning stream"""
    import torch

    want = {name: fresh(name) for name in cs.PRODUCT_ORDER}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = new_context()
    with torch.cuda.stream(s2):
        b = new_context()
    try:
        for name in cs.PRODUCT_ORDER:
            for which, stream, c in (("A", s1, a), ("B", s2, b)):
                with torch.cuda.stream(stream):
                    out = cs.CASES_BY_NAME[name].run(c)
                    cs.assert_same_bits(out, want[name], f"{name} on context {which}")
                    assert_invariants(c, f"{name} on context {which}")
    finally:
        for stream, c in ((s1, a), (s2, b)):
            with torch.cuda.stream(stream):
                c.close()
