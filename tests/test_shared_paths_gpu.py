"""Shared paths on the GPU: scp_path_load, scp_reference_paths_shared and scp_negotiate_paths against tests/shared_path_ref.py
(integers exactly, the reference points bit for bit), what a call must leave untouched, the argument checks, and the planner's
surface: set_path_sharing, find_reference / shorten_reference / set_corridors on the two-door scene, the CLI."""
import numpy as np
import pytest

import shared_path_cases as sc
import shorten_ref as sr
import weighted_path_ref as wr

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sc.all_cases()}
GARBAGE = 0x5EED5EED


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _grid(c):
    from path_planning import _hip

    return _hip.occupancy_grid(c.D, c.origin, c.cell, c.occ.shape[::-1])


def _map(ctx, c):
    """(grid, sat, edges, pen or None) of a case on the device"""
    g = _grid(c)
    occ, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    pen = None
    if c.weight is not None:
        pen = ctx.lattice_penalties(c.D, g, ctx.obstacle_distance(c.D, g, occ, 1), c.stride, c.prefer, c.weight)
        np.testing.assert_array_equal(pen.cpu().numpy().view(np.uint32), c.map()["pen"])
    return g, sat, edges, pen


def _i32(ctx, array):
    """a device tensor of the 32-bit words of an int32 / uint32 / record array"""
    import torch

    return torch.as_tensor(np.ascontiguousarray(array).view(np.int32).copy()).to(ctx.tdev)


def _info_tensor(ctx, info):
    import torch

    return torch.as_tensor(np.ascontiguousarray(info).view(np.uint8).copy()).to(ctx.tdev)


def _records(t, N):
    from path_planning import _hip

    return t.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:N].copy()


def _same_set(got, want, what):
    """(ref, path, info, path_cost) against the restatement's"""
    np.testing.assert_array_equal(got[0].view(np.uint64), want[0].view(np.uint64), err_msg=f"{what}: ref")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: path")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: info")
    np.testing.assert_array_equal(got[3], want[3], err_msg=f"{what}: path_cost")


def _negotiate(ctx, c, dev=None, want_path=True, **changed):
    """one scp_negotiate_paths of a case: numpy copies of everything it writes"""
    g, _, edges, pen = dev or _map(ctx, c)
    kw = dict(share_weight=c.share_weight, capacity=c.capacity, groups=c.groups, rounds=c.rounds)
    kw.update(changed)
    ref = ctx.tensor(c.ref_in())
    path, info, path_cost, n_failed, overuse, best_round, n_kept = ctx.negotiate_paths(
        c.N, c.K, c.D, g, c.stride, edges, ctx.tensor(c.p0), ctx.tensor(c.pf), c.max_path, ref, pen=pen, want_path=want_path, **kw)
    return {"set": (ref.cpu().numpy(), path.cpu().numpy() if want_path else None, _records(info, c.N),
                    path_cost.cpu().numpy().view(np.uint32)[:c.N].copy()),
            "n_failed": int(n_failed.item()), "overuse": [int(v) for v in overuse.cpu().numpy().view(np.uint64)],
            "best_round": int(best_round.item()), "n_kept": int(n_kept.item())}


def _assert_negotiated(got, w, what):
    assert got["overuse"] == w["overuse"], what
    assert (got["best_round"], got["n_kept"], got["n_failed"]) == (w["best_round"], w["n_kept"], w["n_failed"]), what
    _same_set(got["set"], (w["ref"], w["path"], w["info"], w["path_cost"]), what)


@pytest.mark.parametrize("name", list(CASES))
def test_path_load_equals_the_restatement(ctx, name):
    """the load and the overuse of every round's set; both outputs pre-filled with garbage: they are written, not accumulated"""
    import torch

    c = CASES[name]
    w = c.want()
    for r, (_, path, info, _) in enumerate(w["sets"]):
        load = torch.full((c.nodes,), GARBAGE, dtype=torch.int32, device=ctx.tdev)
        overuse = torch.full((1,), GARBAGE, dtype=torch.int64, device=ctx.tdev)
        ctx.path_load(c.N, c.max_path, c.nodes, _i32(ctx, path), _info_tensor(ctx, info), c.capacity, load=load, overuse=overuse)
        assert int(overuse.item()) == w["overuse"][r], f"round {r}"
        got = load.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, np.bincount(np.concatenate([path[i, :info["n_nodes"][i]] for i in range(c.N)]),
                                                       minlength=c.nodes).astype(np.uint32))
        if r < c.rounds:
            np.testing.assert_array_equal(got, w["loads"][r])


@pytest.mark.parametrize("name", list(CASES))
def test_reference_paths_shared_equals_the_restatement(ctx, name):
    """every round of the restatement's negotiation as one call: the round's set and load in, the next set out -- ref, path,
    info, path_cost, cost_out and n_kept.  The call reads nothing of an inactive vehicle and only the status of a skipped one
    (the load is given), so all four outputs of both are pre-filled with a pattern no search writes -- the status kept -- and
    must come back byte for byte, their cost rows holding the sentinel; the kept vehicles of short_max_path keep their rows."""
    import torch

    c = CASES[name]
    w = c.want()
    g, _, edges, pen = _map(ctx, c)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    kept_total = 0
    for r in range(c.rounds):
        before, after = ([np.array(a, copy=True) for a in w["sets"][q]] for q in (r, r + 1))
        idle = np.array([i % c.groups != r % c.groups or before[2]["status"][i] != 0 for i in range(c.N)])
        for given in (before, after):  # the same pattern into what goes in and into what must come out
            status = given[2]["status"][idle].copy()
            given[0][idle] = c.ref_in()[idle]
            given[1][idle] = 0x51515151
            given[2].view(np.int32).reshape(c.N, 4)[idle] = 0x52525252
            given[2]["status"][idle] = status
            given[3][idle] = 0x53535353
        ref, path, info, path_cost = ctx.tensor(before[0]), _i32(ctx, before[1]), _info_tensor(ctx, before[2]), _i32(ctx, before[3])
        cost = torch.as_tensor(np.full((c.N, c.nodes), sc.COST_SENTINEL, dtype=np.uint32).view(np.int32)).to(ctx.tdev)
        n_kept = ctx.reference_paths_shared(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, path, info, path_cost,
                                            _i32(ctx, w["loads"][r]), c.share_weight, c.capacity, c.groups, r % c.groups, pen=pen,
                                            cost=cost)
        got = (ref.cpu().numpy(), path.cpu().numpy(), _records(info, c.N), path_cost.cpu().numpy().view(np.uint32))
        _same_set(got, after, f"round {r + 1}")
        np.testing.assert_array_equal(cost.cpu().numpy().view(np.uint32), w["costs"][r], err_msg=f"round {r + 1}: cost_out")
        assert (w["costs"][r][idle] == sc.COST_SENTINEL).all() and (idle.any() or c.groups == 1)
        for a, b in zip(got, before):
            assert a[idle].tobytes() == b[idle].tobytes(), f"round {r + 1}: a row of an inactive or skipped vehicle was written"
        kept_total += int(n_kept.item())
    assert kept_total == w["n_kept"]


@pytest.mark.parametrize("name", list(CASES))
def test_negotiate_paths_equals_the_restatement(ctx, name):
    """every output, after the context's workspaces were filled with a pattern, and again on the same context: nothing depends
    on what the context ran before; without the path table the other outputs are the same"""
    c = CASES[name]
    w = c.want()
    dev = _map(ctx, c)
    ctx.debug_fill(0xDEADBEEF)
    got = _negotiate(ctx, c, dev)
    print(f"{name}: {c.nodes} nodes, N = {c.N}, groups {c.groups}, rounds {c.rounds}: overuse {got['overuse']}, best round "
          f"{got['best_round']}, {ctx.last_pair_ms():.3f} ms on the device")
    _assert_negotiated(got, w, "after debug_fill")
    failed = w["info"]["status"] != 0
    np.testing.assert_array_equal(got["set"][0][failed].view(np.uint64), c.ref_in()[failed].view(np.uint64))
    ctx.debug_fill(0x00000000)
    _assert_negotiated(_negotiate(ctx, c, dev), w, "second call")
    without = _negotiate(ctx, c, dev, want_path=False)
    assert without["overuse"] == w["overuse"] and without["best_round"] == w["best_round"]
    np.testing.assert_array_equal(without["set"][0].view(np.uint64), w["ref"].view(np.uint64))
    np.testing.assert_array_equal(without["set"][2], w["info"])


@pytest.mark.parametrize("name", ["two_doors", "slab_3d", "large", "statuses"])
def test_workgroup_size_does_not_matter(ctx, name):
    c = CASES[name]
    dev = _map(ctx, c)
    try:
        for threads in (64, 256, 1024):
            ctx.set_option("ref_path_threads", threads)
            _assert_negotiated(_negotiate(ctx, c, dev), c.want(), f"{threads} threads")
    finally:
        ctx.set_option("ref_path_threads", 0)


def test_the_other_searches_at_64_threads(ctx):
    """"ref_path_threads" = 64, the width this feature adds to the option, in the four searches that share it: the hop paths
    and the weighted paths, the hop matrix and the cost matrix give the bytes of their restatements"""
    import assign_paths_ref as ar
    import reference_path_cases as rc
    import weighted_path_cases as wc

    hop = {c.name: c for c in rc.all_cases()}["rand2d_13x11_s2_c1"]
    wtd = {c.name: c for c in wc.all_cases()}["rand2d_13x11_s2"]
    try:
        ctx.set_option("ref_path_threads", 64)
        g = _grid(hop)
        _, sat = ctx.occupancy_prepare(hop.D, g, hop.occ)
        edges = ctx.lattice_edges(hop.D, g, sat, hop.stride, hop.clearance)
        ref = ctx.tensor(hop.ref_in())
        path, info, dist, n_failed = ctx.reference_paths(hop.N, hop.K, hop.D, g, hop.stride, edges, ctx.tensor(hop.p0), ctx.tensor(hop.pf),
                                                         hop.max_path, ref, want_dist=True)
        w = hop.want()
        np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint64), w["ref"].view(np.uint64))
        np.testing.assert_array_equal(path.cpu().numpy(), w["path"])
        np.testing.assert_array_equal(_records(info, hop.N), w["info"])
        np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint16), w["dist"])
        assert int(n_failed.item()) == w["n_failed"]
        want_hops, want_src, want_dst, want_dist, _ = ar.hop_matrix(hop.D, hop.origin, hop.cell, hop.occ, hop.stride, hop.clearance,
                                                                    hop.pf, hop.p0)
        hops, src_node, dst_node, fields = ctx.lattice_distances(hop.D, g, hop.stride, edges, ctx.tensor(hop.pf), ctx.tensor(hop.p0),
                                                                  want_dist=True)
        np.testing.assert_array_equal(hops.cpu().numpy().view(np.uint16), want_hops)
        np.testing.assert_array_equal(fields.cpu().numpy().view(np.uint16), want_dist)
        np.testing.assert_array_equal(src_node.cpu().numpy(), want_src)
        np.testing.assert_array_equal(dst_node.cpu().numpy(), want_dst)

        g = _grid(wtd)
        occ, sat = ctx.occupancy_prepare(wtd.D, g, wtd.occ)
        edges = ctx.lattice_edges(wtd.D, g, sat, wtd.stride, wtd.clearance)
        pen = ctx.lattice_penalties(wtd.D, g, ctx.obstacle_distance(wtd.D, g, occ, 1), wtd.stride, wtd.prefer, wtd.weight)
        ref = ctx.tensor(wtd.ref_in())
        path, info, path_cost, cost, n_failed = ctx.reference_paths_weighted(wtd.N, wtd.K, wtd.D, g, wtd.stride, edges, ctx.tensor(wtd.p0),
                                                                             ctx.tensor(wtd.pf), wtd.max_path, ref, pen=pen, want_cost=True)
        w = wtd.want()
        np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint64), w["ref"].view(np.uint64))
        np.testing.assert_array_equal(path.cpu().numpy(), w["path"])
        np.testing.assert_array_equal(_records(info, wtd.N), w["info"])
        np.testing.assert_array_equal(path_cost.cpu().numpy().view(np.uint32)[:wtd.N], w["path_cost"])
        np.testing.assert_array_equal(cost.cpu().numpy().view(np.uint32)[:wtd.N], w["cost"])
        w_costs, w_src, w_dst, w_cost = wr.cost_matrix(wtd.D, wtd.origin, wtd.cell, wtd.dims, wtd.stride, w["edges"], w["pen"], wtd.pf,
                                                       wtd.p0)
        costs, src_node, dst_node, fields = ctx.lattice_costs(wtd.D, g, wtd.stride, edges, ctx.tensor(wtd.pf), ctx.tensor(wtd.p0), pen=pen,
                                                              want_cost=True)
        np.testing.assert_array_equal(costs.cpu().numpy().view(np.uint32), w_costs)
        np.testing.assert_array_equal(fields.cpu().numpy().view(np.uint32), w_cost)
        np.testing.assert_array_equal(src_node.cpu().numpy(), w_src)
        np.testing.assert_array_equal(dst_node.cpu().numpy(), w_dst)
    finally:
        ctx.set_option("ref_path_threads", 0)


@pytest.mark.parametrize("name", ["wide_doors", "statuses", "large"])
def test_no_rounds_is_the_weighted_search(ctx, name):
    c = CASES[name]
    g, _, edges, pen = dev = _map(ctx, c)
    ref = ctx.tensor(c.ref_in())
    path, info, path_cost, _, n_failed = ctx.reference_paths_weighted(c.N, c.K, c.D, g, c.stride, edges, ctx.tensor(c.p0),
                                                                      ctx.tensor(c.pf), c.max_path, ref, pen=pen)
    plain = (ref.cpu().numpy(), path.cpu().numpy(), _records(info, c.N), path_cost.cpu().numpy().view(np.uint32)[:c.N])
    got = _negotiate(ctx, c, dev, rounds=0)
    _same_set(got["set"], plain, "rounds = 0")
    assert got["overuse"] == c.want()["overuse"][:1] and got["best_round"] == 0 and got["n_kept"] == 0
    assert got["n_failed"] == int(n_failed.item())
    # share_weight = 0: every round reproduces round 0
    free = _negotiate(ctx, c, dev, share_weight=0)
    _same_set(free["set"], plain, "share_weight = 0")
    assert free["overuse"] == c.want()["overuse"][:1] * (c.rounds + 1) and free["best_round"] == 0


@pytest.mark.parametrize("name", ["two_doors", "statuses"])
def test_shorten_paths_takes_the_negotiated_paths(ctx, name):
    from path_planning import _hip

    c = CASES[name]
    w = c.want()
    g, sat, edges, pen = _map(ctx, c)
    p0, pf, ref = ctx.tensor(c.p0), ctx.tensor(c.pf), ctx.tensor(c.ref_in())
    path, info, *_ = ctx.negotiate_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, c.share_weight, c.capacity,
                                         c.groups, c.rounds, pen=pen)
    kept, out = ctx.shorten_paths(c.N, c.K, c.D, g, sat, c.stride, c.clearance, p0, pf, c.max_path, path, info, ref)
    w_ref, w_kept, w_out, _ = sr.shorten_paths(c.D, c.origin, c.cell, c.map()["sat"], c.stride, c.clearance, c.p0, c.pf, c.K,
                                               w["path"], w["info"], w["ref"])
    np.testing.assert_array_equal(kept.cpu().numpy(), w_kept)
    got_out = out.cpu().numpy().view(_hip.SHORTEN_INFO_DTYPE)[:c.N]
    np.testing.assert_array_equal(got_out["n_kept"], w_out["n_kept"])
    np.testing.assert_array_equal(got_out["length"].view(np.uint64), w_out["length"].view(np.uint64))
    np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint64), w_ref.view(np.uint64))


def test_argument_checks(ctx):
    from path_planning import _hip

    c = CASES["two_doors"]
    w = c.want()
    g, _, edges, pen = _map(ctx, c)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)

    def negotiate(N=c.N, K=c.K, stride=c.stride, max_path=c.max_path, edges=edges, **kw):
        args = dict(share_weight=70, capacity=1, groups=4, rounds=2)
        args.update(kw)
        return ctx.negotiate_paths(N, K, c.D, g, stride, edges, p0, pf, max_path, ctx.tensor(c.ref_in()), pen=pen, **args)

    negotiate(rounds=64, groups=c.N, share_weight=32768)
    for bad, match in ((dict(rounds=65), "rounds"), (dict(rounds=-1), "rounds"), (dict(groups=0), "groups"),
                       (dict(groups=c.N + 1), "groups"), (dict(capacity=0), "capacity"), (dict(share_weight=-1), "share_weight"),
                       (dict(share_weight=32769), "share_weight"), (dict(N=0), "shape"), (dict(K=0), "shape"),
                       (dict(stride=0), "stride"), (dict(max_path=0), "max_path"), (dict(max_path=c.nodes + 1), "max_path"),
                       (dict(edges=None), "null")):
        with pytest.raises(_hip.HipError, match=match):
            negotiate(**bad)

    before = w["sets"][0]
    load = _i32(ctx, w["loads"][0])

    def shared(path="given", load=load, **kw):
        args = dict(share_weight=70, capacity=1, groups=4, group=0)
        args.update(kw)
        ref, info, path_cost = ctx.tensor(before[0]), _info_tensor(ctx, before[2]), _i32(ctx, before[3])
        return ctx.reference_paths_shared(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref,
                                          _i32(ctx, before[1]) if path == "given" else path, info, path_cost, load, pen=pen, **args)

    shared(groups=c.N, group=c.N - 1)
    for bad, match in ((dict(group=4), "group"), (dict(group=-1), "group"), (dict(groups=0), "groups"), (dict(groups=c.N + 1), "groups"),
                       (dict(capacity=0), "capacity"), (dict(share_weight=32769), "share_weight"), (dict(path=None), "null"),
                       (dict(load=None), "null")):
        with pytest.raises(_hip.HipError, match=match):
            shared(**bad)

    path, info = _i32(ctx, before[1]), _info_tensor(ctx, before[2])
    for bad, match in ((dict(N=0), "shape"), (dict(max_path=0), "shape"), (dict(nodes=0), "nodes"), (dict(nodes=32769), "nodes"),
                       (dict(capacity=0), "capacity"), (dict(path=None), "null"), (dict(info=None), "null")):
        args = dict(N=c.N, max_path=c.max_path, nodes=c.nodes, path=path, info=info, capacity=1)
        args.update(bad)
        with pytest.raises(_hip.HipError, match=match):
            ctx.path_load(**args)


# ---- nothing depends on what the context ran before -------------------------------------------------------------------------------
def test_context_state_case():
    """the case of tests/shared_path_ctx_case.py through the harness of tests/test_ctx_state_gpu.py: on a new context it gives
    the restatement and calls every entry point it names; after the family's grower, with every scratch workspace filled with
    all ones and then with 1 in every word before EVERY call, it gives the same bits and needs no more of any buffer"""
    import ctx_state_cases as cs
    import shared_path_ctx_case as scc
    import test_ctx_state_gpu as tcs

    case = scc.register()
    tcs.fresh(scc.NAME)
    assert set(scc.SHARED_ENTRIES) <= case.called
    c = tcs.new_context()
    try:
        cs.GROWERS[case.family].run(c)
        grown = tcs.assert_invariants(c, "after the grower")
        for word in (0xFFFFFFFF, 0x00000001):
            st = tcs.check(c, scc.NAME, f"after debug_fill({word:#x})", poison=word)
            assert {k: st[k] for k in tcs.SIZES} == {k: grown[k] for k in tcs.SIZES}, "the case needed more of a buffer than its grower left"
        tcs.check(c, scc.NAME, "a second time on the same context")
    finally:
        c.close()
    # its neighbours in the shared workspace: the product's order of the other users with the negotiation where SCP runs it
    # (after the weighted search, before the shortening), then directly behind the user with the largest layout
    names = list(cs.PRODUCT_ORDER)
    at = names.index("reference_paths_weighted") + 1
    largest = max(names, key=lambda n: cs.CASES_BY_NAME[n].ws()["sep_ws"][0])
    assert cs.CASES_BY_NAME[largest].ws()["sep_ws"][0] > case.ws()["sep_ws"][1]
    c = tcs.new_context()
    try:
        for i, name in enumerate(names[:at] + [scc.NAME] + names[at:] + [largest, scc.NAME]):
            tcs.check(c, name, f"as user {i} of the product order with the negotiation in it")
    finally:
        c.close()


# ---- the planner's surface -------------------------------------------------------------------------------------------------------
def _planner(S):
    from path_planning.solvers.scp import SCP

    s = SCP(n_vehicles=S.N, time_horizon=S.T, time_step=S.h, min_distance=S.R, space_dims=S.space, verbose=False)
    s.set_initial_states(S.p0)
    s.set_final_states(S.pf)
    s.set_obstacles(*S.grid())
    return s


def test_planner_spreads_the_fleet_over_the_doors(ctx):
    """the two-door scene: with sharing the overuse falls, fewer paths pass the busier door, and the corridors around the
    negotiated paths have no blocked segment (K >= every E)"""
    S = sc.TwoDoorScene
    s = _planner(S)
    s.set_search_metric("length")
    ref0, plain = s.find_reference(stride=S.stride)
    assert "sharing" not in plain
    s.set_path_sharing(share=1.0)
    ref, info = s.find_reference(stride=S.stride)
    sh = info["sharing"]
    assert (sh["share_weight"], sh["capacity"], sh["groups"], sh["rounds"]) == (70, 1, 4, 8) and len(sh["overuse"]) == 9
    assert sh["overuse"][sh["best_round"]] < sh["overuse"][0] and sh["overuse"][sh["best_round"]] == min(sh["overuse"])
    w = S.case().want()
    assert sh["overuse"] == w["overuse"] and sh["best_round"] == w["best_round"] and sh["n_kept"] == w["n_kept"]
    assert 0 < sh["best_round"] < sh["rounds"]
    np.testing.assert_array_equal(info["n_nodes"], w["info"]["n_nodes"])
    np.testing.assert_array_equal(info["cost"], w["path_cost"].astype(np.int64))
    load0, load1 = (sc.sp.path_load(*w["sets"][r][1:3], 576, 1)[0] for r in (0, w["best_round"]))
    assert sh["max_load"] == int(load1.max())

    def through(reference, y):  # the vehicles whose reference passes the door cell (12, y)
        cells = np.floor(reference / S.cell).astype(int)
        return int(((cells[..., 0] == 12) & (cells[..., 1] == y)).any(axis=1).sum())

    doors0, doors1 = [through(ref0, y) for y in S.doors], [through(ref, y) for y in S.doors]
    print(f"overuse {sh['overuse']}, best round {sh['best_round']}; vehicles through the doors {doors0} -> {doors1}; largest load "
          f"{int(load0.max())} -> {int(load1.max())}")
    assert doors0 == [int(load0[y * 24 + 12]) for y in S.doors] == [S.N, 0]
    assert doors1 == [int(load1[y * 24 + 12]) for y in S.doors] and sum(doors1) == S.N and max(doors1) < max(doors0)
    assert int(info["n_nodes"].max()) + 1 <= S.K
    co = s.set_corridors(reference=ref)
    assert co["n_blocked"] == 0 and co["n_open"] == 0 and co["shrink"] < 0.2 * S.cell
    # shorten_reference shortens the negotiated paths, set_corridors("search") runs the negotiation itself
    _, short = s.shorten_reference(stride=S.stride, clearance=0)
    assert short["sharing"]["overuse"] == sh["overuse"]
    np.testing.assert_array_equal(short["cost"], info["cost"])
    s.set_search_metric("hops")
    with pytest.raises(ValueError, match="set_search_metric"):
        s.find_reference(stride=S.stride)
    s.set_path_sharing()
    s.find_reference(stride=S.stride)
    s.close()


def test_cli_runs_through(capsys):
    from path_planning.cli import compute_trajectories as ct

    solver = ct.main(["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--min-distance", "0.8", "--space", "0", "0",
                      "20", "20", "--seed", "1", "--no-plots", "--obstacle-discs", "13.2,7.3,0.6", "--corridor-search",
                      "--corridor-metric", "length", "--corridor-share", "1.0", "--corridor-share-capacity", "1",
                      "--corridor-share-groups", "2", "--corridor-share-rounds", "3"])
    out = capsys.readouterr().out
    print(out)
    import re

    assert solver is not None and "4 of 4 paths found" in out and re.search(r", overuse \d+ -> \d+ \(round \d of 3\)", out)
    assert solver._sharing == (70, 1, 2, 3)
