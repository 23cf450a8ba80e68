"""The weighted lattice search on the GPU: scp_lattice_penalties, scp_reference_paths_weighted and scp_lattice_costs against
tests/weighted_path_ref.py (integers exactly, the reference points bit for bit), the argument checks, and the planner's
surface: set_search_metric, find_reference / shorten_reference by length and clearance, assign_goals(cost="length"), the CLI."""
import time

import numpy as np
import pytest

import reference_path_cases as rc
import shorten_ref as sr
import weighted_path_cases as wc
import weighted_path_ref as wr

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in wc.all_cases()}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _grid(c):
    from path_planning import _hip

    return _hip.occupancy_grid(c.D, c.origin, c.cell, c.occ.shape[::-1])


def _map(ctx, c, with_pen=True):
    """(grid, sat, edges, pen or None) of a case on the device"""
    g = _grid(c)
    occ, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    pen = None
    if with_pen and c.weight is not None:
        pen = ctx.lattice_penalties(c.D, g, ctx.obstacle_distance(c.D, g, occ, 1), c.stride, c.prefer, c.weight)
    return g, sat, edges, pen


def _run(ctx, c, want_path=True, want_cost=True, with_pen=True):
    """penalties and one weighted search of a case: numpy copies of everything the calls write"""
    from path_planning import _hip

    g, _, edges, pen = _map(ctx, c, with_pen)
    ref = ctx.tensor(c.ref_in())
    path, info, path_cost, cost, n_failed = ctx.reference_paths_weighted(
        c.N, c.K, c.D, g, c.stride, edges, ctx.tensor(c.p0), ctx.tensor(c.pf), c.max_path, ref, pen=pen, want_path=want_path,
        want_cost=want_cost)
    return {"pen": pen.cpu().numpy().view(np.uint32) if pen is not None else None, "ref": ref.cpu().numpy(),
            "path": path.cpu().numpy() if want_path else None, "info": info.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:c.N].copy(),
            "path_cost": path_cost.cpu().numpy().view(np.uint32)[:c.N].copy(),
            "cost": cost.cpu().numpy().view(np.uint32)[:c.N] if want_cost else None, "n_failed": int(n_failed.item())}


def _assert_equal(got, want, keys=("pen", "info", "path", "path_cost", "cost", "ref", "n_failed")):
    for k in keys:
        if k == "ref":
            np.testing.assert_array_equal(got[k].view(np.uint64), want[k].view(np.uint64), err_msg=k)
        elif k == "n_failed" or want[k] is None:
            assert got[k] == want[k], k
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_restatement(ctx, name):
    """(measured on one MI355X: the longest searches are the open 8193 x 1 strip, 38.9 ms for 8192 sweeps, the serpentine at the
    product limit, 11.3 ms, and the 32768-node map, 9.1 ms; every other case stays below 0.2 ms)"""
    c = CASES[name]
    want = c.want()
    t0 = time.perf_counter()
    got = _run(ctx, c)
    print(f"{name}: {c.nodes} nodes, N = {c.N}: edges, penalties, search and copies in {time.perf_counter() - t0:.3f} s, search "
          f"{ctx.last_pair_ms():.3f} ms on the device")
    _assert_equal(got, want)
    # the rows of ref of a failed vehicle keep the marked bytes they were given
    failed = want["info"]["status"] != 0
    np.testing.assert_array_equal(got["ref"][failed].view(np.uint64), c.ref_in()[failed].view(np.uint64))
    # a second call with the same inputs: the same bytes
    _assert_equal(_run(ctx, c), got)
    # without the optional outputs: info, path_cost and ref are unchanged
    _assert_equal(_run(ctx, c, want_path=False, want_cost=False), want, keys=("info", "path_cost", "ref", "n_failed"))


def test_null_penalties_are_zero_penalties(ctx):
    c = CASES["empty_map"]
    want = c.want()
    assert not want["pen"].any() and (want["field"] == 0xFFFFFFFF).all()
    got = _run(ctx, c)
    _assert_equal(got, want)
    _assert_equal(_run(ctx, c, with_pen=False), dict(got, pen=None))


@pytest.mark.parametrize("name", ["detour", "rand3d_7_s1", "ties", "limit"])
def test_workgroup_size_does_not_matter(ctx, name):
    c = CASES[name]
    try:
        for threads in (256, 512, 1024):
            ctx.set_option("ref_path_threads", threads)
            _assert_equal(_run(ctx, c), c.want())
    finally:
        ctx.set_option("ref_path_threads", 0)


@pytest.mark.parametrize("name", ["rand2d_13x11_s2", "rand3d_7_s1"])
def test_lattice_costs(ctx, name):
    """the matrix and every field against the restatement with n_src != n_dst; the row of source a is the field of the path
    search with goal a: one sweep serves both kernels"""
    c = CASES[name]
    want = c.want()
    src, dst = c.pf, np.concatenate([c.p0, c.pf[:2]])  # 5 sources, 7 destinations (some off the lattice in the random cases)
    g, _, edges, pen = _map(ctx, c)
    costs, src_node, dst_node, cost = ctx.lattice_costs(c.D, g, c.stride, edges, ctx.tensor(src), ctx.tensor(dst), pen=pen,
                                                        want_cost=True)
    w_costs, w_src, w_dst, w_cost = wr.cost_matrix(c.D, c.origin, c.cell, c.dims, c.stride, want["edges"], want["pen"], src, dst)
    np.testing.assert_array_equal(src_node.cpu().numpy(), w_src)
    np.testing.assert_array_equal(dst_node.cpu().numpy(), w_dst)
    np.testing.assert_array_equal(costs.cpu().numpy().view(np.uint32), w_costs)
    cost = cost.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(cost, w_cost)
    fields = _run(ctx, c)["cost"]
    searched = want["info"]["status"] == 0  # (a vehicle with status 1 has no field, though its goal may have a node)
    assert searched.sum() >= 3
    np.testing.assert_array_equal(cost[searched], fields[searched])
    same = w_src[:, None] == w_dst[None, :]
    assert (w_costs[same & (w_src[:, None] >= 0)] == 0).all()
    without = ctx.lattice_costs(c.D, g, c.stride, edges, ctx.tensor(src), ctx.tensor(dst), pen=pen)
    assert without[3] is None
    np.testing.assert_array_equal(without[0].cpu().numpy().view(np.uint32), w_costs)


@pytest.mark.parametrize("name", ["rand2d_13x11_s2", "rand3d_7_s1"])
def test_workgroup_size_does_not_matter_to_lattice_costs(ctx, name):
    """the matrix, both node lists and every field are the restatement's bytes at every width, with and without the fields"""
    c = CASES[name]
    want = c.want()
    outside = (np.asarray(c.origin, dtype=np.float64) - 10.0 * c.cell)[None, :c.D]
    src, dst = c.pf, np.concatenate([c.p0, c.pf[:2], outside])  # 5 sources, 8 destinations, the last one off the grid
    g, _, edges, pen = _map(ctx, c)
    w_costs, w_src, w_dst, w_cost = wr.cost_matrix(c.D, c.origin, c.cell, c.dims, c.stride, want["edges"], want["pen"], src, dst)
    assert len(src) != len(dst) and w_dst[-1] == -1 and (w_src >= 0).any() and (w_costs != 0xFFFFFFFF).any()
    try:
        for threads in (256, 512, 1024):
            ctx.set_option("ref_path_threads", threads)
            for want_cost in (True, False):
                costs, src_node, dst_node, cost = ctx.lattice_costs(c.D, g, c.stride, edges, ctx.tensor(src), ctx.tensor(dst), pen=pen,
                                                                    want_cost=want_cost)
                np.testing.assert_array_equal(src_node.cpu().numpy(), w_src, err_msg=f"src_node at {threads}")
                np.testing.assert_array_equal(dst_node.cpu().numpy(), w_dst, err_msg=f"dst_node at {threads}")
                np.testing.assert_array_equal(costs.cpu().numpy().view(np.uint32), w_costs, err_msg=f"costs at {threads}")
                if want_cost:
                    np.testing.assert_array_equal(cost.cpu().numpy().view(np.uint32), w_cost, err_msg=f"fields at {threads}")
                else:
                    assert cost is None
    finally:
        ctx.set_option("ref_path_threads", 0)


@pytest.mark.parametrize("name", ["detour", "rand2d_13x11_s2", "limit"])
def test_shorten_paths_takes_the_weighted_path(ctx, name):
    from path_planning import _hip

    c = CASES[name]
    want = c.want()
    g, sat, edges, pen = _map(ctx, c)
    p0, pf, ref = ctx.tensor(c.p0), ctx.tensor(c.pf), ctx.tensor(c.ref_in())
    path, info, _, _, _ = ctx.reference_paths_weighted(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, pen=pen)
    kept, out = ctx.shorten_paths(c.N, c.K, c.D, g, sat, c.stride, c.clearance, p0, pf, c.max_path, path, info, ref)
    w_ref, w_kept, w_out, _ = sr.shorten_paths(c.D, c.origin, c.cell, want["sat"], c.stride, c.clearance, c.p0, c.pf, c.K,
                                               want["path"], want["info"], want["ref"])
    np.testing.assert_array_equal(kept.cpu().numpy(), w_kept)
    got_out = out.cpu().numpy().view(_hip.SHORTEN_INFO_DTYPE)[:c.N]
    for k in ("n_kept", "n_vertices"):
        np.testing.assert_array_equal(got_out[k], w_out[k])
    for k in ("length", "length_before"):
        np.testing.assert_array_equal(got_out[k].view(np.uint64), w_out[k].view(np.uint64))
    np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint64), w_ref.view(np.uint64))


def test_argument_checks(ctx):
    from path_planning import _hip

    c = CASES["rand2d_13x11_s2"]
    g, _, edges, pen = _map(ctx, c)
    occ, _ = ctx.occupancy_prepare(c.D, g, c.occ)
    field = ctx.obstacle_distance(c.D, g, occ, 1)
    # the product limit: 32768 passes, 32769 does not; negative values; strides without a lattice
    ctx.lattice_penalties(c.D, g, field, c.stride, 32768, 1)
    ctx.lattice_penalties(c.D, g, field, c.stride, 2, 16384)
    for prefer, weight in ((32769, 1), (3, 10923), (1, 32769), (2**16, 2**16), (-1, 1), (1, -1)):
        with pytest.raises(_hip.HipError):
            ctx.lattice_penalties(c.D, g, field, c.stride, prefer, weight)
    with pytest.raises(_hip.HipError, match="exceeds"):
        ctx.lattice_penalties(c.D, g, field, c.stride, 181, 182)
    for stride in (0, -1, 12):
        with pytest.raises(_hip.HipError):
            ctx.lattice_penalties(c.D, g, field, stride, 1, 1)
    with pytest.raises(_hip.HipError, match="null"):
        ctx.lattice_penalties(c.D, g, None, c.stride, 1, 1)
    p0, pf, ref = ctx.tensor(c.p0), ctx.tensor(c.pf), ctx.tensor(c.ref_in())
    for N, K, stride, max_path in ((0, c.K, c.stride, 5), (c.N, 0, c.stride, 5), (c.N, c.K, 0, 5), (c.N, c.K, 12, 5),
                                   (c.N, c.K, c.stride, 0), (c.N, c.K, c.stride, c.nodes + 1)):
        with pytest.raises(_hip.HipError):
            ctx.reference_paths_weighted(N, K, c.D, g, stride, edges, p0, pf, max_path, ref, pen=pen)
    with pytest.raises(_hip.HipError, match="null"):
        ctx.reference_paths_weighted(c.N, c.K, c.D, g, c.stride, None, p0, pf, 5, ref, pen=pen)
    with pytest.raises(_hip.HipError, match="null"):
        ctx.lattice_costs(c.D, g, c.stride, None, p0, pf, pen=pen)
    for stride in (0, 12):
        with pytest.raises(_hip.HipError):
            ctx.lattice_costs(c.D, g, stride, edges, p0, pf, pen=pen)
    # a stride other than the masks': another lattice, refused where it is not supported at all
    big = np.zeros((1, 129, 256), dtype=np.uint8)  # 33 024 nodes at stride 1
    gb = _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (256, 129))
    with pytest.raises(_hip.HipError, match="nodes"):
        ctx.reference_paths_weighted(c.N, c.K, 2, gb, 1, edges, p0, pf, 5, ref)
    assert big.size == 33024


# ---- the planner's surface -------------------------------------------------------------------------------------------------------
def _planner(S, **kw):
    from path_planning.solvers.scp import SCP

    s = SCP(n_vehicles=S.N, time_horizon=S.T, time_step=S.h, min_distance=S.R, space_dims=S.space, verbose=False, **kw)
    s.set_initial_states(S.p0)
    s.set_final_states(S.pf)
    s.set_obstacles(*S.grid())
    return s


def test_default_arguments_give_the_hop_search(ctx):
    W = rc.WallScene
    s = _planner(W)
    want = {c.name: c for c in rc.all_cases()}["wall_scene"].want()
    ref, info = s.find_reference()
    np.testing.assert_array_equal(ref.view(np.uint64), want["ref"].view(np.uint64))
    assert info["metric"] == "hops" and info["keep_clear"] == 0 and info["penalties_ms"] == 0.0
    np.testing.assert_array_equal(info["cost"], want["info"]["n_nodes"].astype(np.int64) - 1)
    for bad in (dict(metric="metres"), dict(metric="hops", keep_clear=1), dict(metric="length", keep_clear=-1),
                dict(metric="length", keep_clear=1.0), dict(metric="length", keep_clear=True),
                dict(metric="length", keep_clear=2, clear_weight=-1.0), dict(metric="length", keep_clear=2, clear_weight="1"),
                dict(metric="length", keep_clear=2, clear_weight=float("nan")), dict(metric="length", keep_clear=469, clear_weight=1.0)):
        with pytest.raises(ValueError):
            s.set_search_metric(**bad)
    s.set_search_metric("length", keep_clear=468, clear_weight=1.0)  # 468 * 70 = 32760
    s.set_search_metric()
    again, _ = s.find_reference()
    np.testing.assert_array_equal(again.view(np.uint64), ref.view(np.uint64))
    assert not s._obstacles.node_penalties
    s.close()


def test_keep_clear_takes_the_wide_gap(ctx):
    """the two-gap scene: the path by hops squeezes through the near gap, the path by length with keep_clear = 2 keeps rho >= 2
    at every node; its corridors carry a solve that stays inside them"""
    T = wc.TwoGaps
    c = T.case()
    want = c.want()
    s = _planner(T)
    hop_ref, hop_info = s.find_reference(stride=T.stride)
    hop_want = rc.Case("h", c.D, c.occ, c.origin, c.cell, c.stride, 0, c.K, c.p0, c.pf, max_path=c.max_path).want()
    np.testing.assert_array_equal(hop_ref.view(np.uint64), hop_want["ref"].view(np.uint64))
    s.set_search_metric("length", keep_clear=T.keep_clear)
    ref, info = s.find_reference(stride=T.stride)
    np.testing.assert_array_equal(ref.view(np.uint64), want["ref"].view(np.uint64))
    np.testing.assert_array_equal(info["cost"], want["path_cost"].astype(np.int64))
    np.testing.assert_array_equal(info["n_nodes"], want["info"]["n_nodes"])
    assert info["metric"] == "length" and info["keep_clear"] == 2 and info["penalties_ms"] > 0 and info["search_ms"] > 0
    assert s.find_reference(stride=T.stride)[1]["penalties_ms"] == 0.0 and list(s._obstacles.node_penalties) == [(2, 2, 70)]
    rho = want["rho"]
    for i in range(T.N):
        assert (rho[want["path"][i, :want["info"]["n_nodes"][i]]] >= 2).all()
        assert (rho[hop_want["path"][i, :hop_want["info"]["n_nodes"][i]]] < 2).any()
    # keep_clear = 0: length only, no penalties are made
    s.set_search_metric("length")
    _, plain = s.find_reference(stride=T.stride)
    flat = wc.WCase(c.base).want()
    np.testing.assert_array_equal(plain["cost"], flat["path_cost"].astype(np.int64))
    assert plain["penalties_ms"] == 0.0 and list(s._obstacles.node_penalties) == [(2, 2, 70)]
    # shorten_reference takes the weighted path
    s.set_search_metric("length", keep_clear=T.keep_clear)
    short, sinfo = s.shorten_reference(stride=T.stride, clearance=0)
    w_short, _, w_out, _ = sr.shorten_paths(c.D, c.origin, c.cell, want["sat"], c.stride, 0, c.p0, c.pf, c.K, want["path"],
                                            want["info"], want["ref"])
    np.testing.assert_array_equal(short.view(np.uint64), w_short.view(np.uint64))
    np.testing.assert_array_equal(sinfo["n_kept"], w_out["n_kept"])
    np.testing.assert_array_equal(sinfo["cost"], want["path_cost"].astype(np.int64))
    # the corridors around the weighted path carry a solve
    co = s.set_corridors(reference=ref)
    assert co["n_blocked"] == 0 and co["n_open"] == 0
    s.generate_trajectories(max_iterations=15)
    assert s.validate_corridor()["inside"]
    s.close()


def test_assign_goals_by_length(ctx):
    A = wc.AssignScene
    want = A.want()
    assert not np.array_equal(want["by_length"], want["by_path"])
    s = _planner(A)
    s.set_search_metric("length", keep_clear=A.keep_clear)
    perm = s.assign_goals(cost="length", stride=A.stride, power=1)
    np.testing.assert_array_equal(perm, want["by_length"])
    info = s.assignment_info
    L = want["lengths"].astype(np.int64)
    assert info["length_identity"] == {"sum": int(np.trace(L)), "max": int(np.diag(L).max())}
    assert info["length_assigned"]["sum"] == int(L[np.arange(A.N), perm].sum()) <= info["length_identity"]["sum"]
    assert info["shift"] == 0 and info["max_cost"] == int(L.max()) and info["keep_clear"] == A.keep_clear
    assert info["n_unreachable_identity"] == info["n_unreachable_assigned"] == 0 and info["distances_ms"] > 0
    np.testing.assert_array_equal(s.final_positions.reshape(A.N, A.D), A.pf[perm])
    s.set_search_metric()
    np.testing.assert_array_equal(s.assign_goals(cost="path", stride=A.stride, power=1), want["by_path"])
    assert "length_assigned" not in s.assignment_info
    with pytest.raises(ValueError, match="cost="):
        s.assign_goals(cost="metres")
    s.close()


def test_cli_runs_through(ctx, capsys):
    from path_planning.cli import compute_trajectories as ct

    # four vehicles in 20 x 20 (the scene of the other CLI tests); the disc sits on the straight line of vehicle 0
    solver = ct.main(["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--min-distance", "0.8", "--space", "0", "0",
                      "20", "20", "--seed", "1", "--no-plots", "--obstacle-discs", "13.2,7.3,0.6", "--corridor-search",
                      "--corridor-metric", "length", "--corridor-keep-clear", "1"])
    out = capsys.readouterr().out
    print(out)
    assert solver is not None and "by length (keep clear 1 cells)" in out and "4 of 4 paths found" in out
    assert "every segment stays inside its box" in out and solver.validate_corridor()["inside"]
