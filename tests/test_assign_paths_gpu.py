"""Goal assignment by path length on the GPU: scp_lattice_distances and scp_assign_costs against tests/assign_paths_ref.py byte
for byte, the argument checks, and the feature through SCP.assign_goals(cost="path") on a wall with one gap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_paths_ref as P  # noqa: E402
import assignment_ref as R  # noqa: E402
import reference_path_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KEYS = ("cost_q", "cost_q_identity", "quantum", "phases", "rounds", "bids", "status")
ORIGIN, CELL = [-1.5, 0.25, 2.0], 0.4


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


# ---- scp_lattice_distances -----------------------------------------------------------------------------------------------------
def _at(D, *cells):
    """points given in cell coordinates (fractions included)"""
    return np.array([[ORIGIN[d] + CELL * c[d] for d in range(D)] for c in cells])


def _wall_13x11():
    """13 x 11 cells: a wall across x = 6 with the gap y = 4, 5, and a closed pocket around the cells (10 .. 11, 8 .. 9).  At
    stride 2 the cells x = 12 and y = 10 belong to no node."""
    occ = np.zeros((1, 11, 13), dtype=np.uint8)
    occ[0, :, 6] = 1
    occ[0, 4:6, 6] = 0
    occ[0, 7, 9:13] = occ[0, 10, 9:13] = occ[0, 7:11, 9] = occ[0, 7:11, 12] = 1
    pts = _at(2, (1.3, 1.6), (10.5, 8.5), (-1.0, 3.0), (8.5, 2.5), (6.5, 0.5), (1.7, 1.2), (12.5, 2.5), (11.2, 9.3), (np.nan, 2.0),
              (3.5, 10.5), (0.5, 13.0), (5.2, 4.9))
    return occ, pts


def _maps():
    """name -> (D, occ, stride, clearance, [(src, dst), ...])"""
    out = {}
    occ, pts = _wall_13x11()
    calls = [(pts[:3], pts[3:8]), (pts[:1], pts[3:4]), (pts[1:2], pts[7:8]), (pts, pts)]
    out["wall-13x11-stride1"] = (2, occ, 1, 0, calls)
    out["wall-13x11-stride2"] = (2, occ, 2, 0, calls)
    out["wall-13x11-stride1-clearance1"] = (2, occ, 1, 1, calls[:1])  # (the gap is two cells wide: closed)
    rng = np.random.default_rng(654)
    occ = (rng.random((4, 5, 6)) < 0.12).astype(np.uint8)
    pts = np.concatenate([_at(3, *rng.uniform(0.0, [6.0, 5.0, 4.0], (9, 3))), _at(3, (2.0, 2.0, 4.5))])
    out["3d-6x5x4"] = (3, occ, 1, 0, [(pts[:3], pts[3:8]), (pts, pts)])
    occ = (rng.random((1, 30, 40)) < 0.3).astype(np.uint8)  # 1200 nodes: more than one pass of the threads; pockets
    pts = _at(2, *rng.uniform(0.0, [40.0, 30.0], (11, 2)))
    out["random-40x30"] = (2, occ, 1, 0, [(pts[:5], pts[5:])])
    occ = np.zeros((1, 181, 181), dtype=np.uint8)  # 32761 nodes: near the limit of the LDS
    occ[0, 20:, 60] = occ[0, :160, 120] = 1
    out["walls-181x181"] = (2, occ, 1, 0, [(_at(2, (3.5, 170.5), (100.2, 90.7)), _at(2, (178.5, 2.5), (3.5, 170.5), (60.5, 50.5)))])
    return out


MAPS = _maps()


@pytest.mark.parametrize("name", list(MAPS))
def test_lattice_distances_equal_the_restatement(ctx, name):
    from path_planning import _hip

    D, occ, stride, clearance, calls = MAPS[name]
    g = _hip.occupancy_grid(D, ORIGIN[:D], CELL, occ.shape[::-1])
    _, sat = ctx.occupancy_prepare(D, g, occ)
    edges = ctx.lattice_edges(D, g, sat, stride, clearance)
    for src, dst in calls:
        want_hops, want_src, want_dst, want_dist, want_edges = P.hop_matrix(D, ORIGIN[:D], CELL, occ, stride, clearance, src, dst)
        np.testing.assert_array_equal(edges.cpu().numpy().view(np.uint32), want_edges)
        hops, src_node, dst_node, dist = ctx.lattice_distances(D, g, stride, edges, ctx.tensor(src), ctx.tensor(dst), want_dist=True)
        assert hops.shape == (len(src), len(dst)) and dist.shape == want_dist.shape
        np.testing.assert_array_equal(src_node.cpu().numpy(), want_src, err_msg="src_node")
        np.testing.assert_array_equal(dst_node.cpu().numpy(), want_dst, err_msg="dst_node")
        np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint16), want_dist, err_msg="dist")
        np.testing.assert_array_equal(hops.cpu().numpy().view(np.uint16), want_hops, err_msg="hops")
        # without the optional output: the same hops
        again, _, _, none = ctx.lattice_distances(D, g, stride, edges, ctx.tensor(src), ctx.tensor(dst))
        assert none is None
        np.testing.assert_array_equal(again.cpu().numpy().view(np.uint16), want_hops)
        assert ctx.last_pair_ms() > 0.0


@pytest.mark.parametrize("name", ["wall-13x11-stride2", "3d-6x5x4"])
def test_workgroup_size_does_not_matter_to_lattice_distances(ctx, name):
    """the matrix, both node lists and every field are the restatement's bytes at every width, with and without the fields"""
    from path_planning import _hip

    D, occ, stride, clearance, calls = MAPS[name]
    pts = calls[-1][0]
    src, dst = pts[:3], pts[3:]  # 3 sources; 9 / 7 destinations; both maps have a point without a node among them
    g = _hip.occupancy_grid(D, ORIGIN[:D], CELL, occ.shape[::-1])
    _, sat = ctx.occupancy_prepare(D, g, occ)
    edges = ctx.lattice_edges(D, g, sat, stride, clearance)
    want_hops, want_src, want_dst, want_dist, _ = P.hop_matrix(D, ORIGIN[:D], CELL, occ, stride, clearance, src, dst)
    assert len(src) != len(dst) and (want_dst == -1).any() and (want_src >= 0).any() and (want_hops != 0xFFFF).any()
    try:
        for threads in (256, 512, 1024):
            ctx.set_option("ref_path_threads", threads)
            for want in (True, False):
                hops, src_node, dst_node, dist = ctx.lattice_distances(D, g, stride, edges, ctx.tensor(src), ctx.tensor(dst),
                                                                       want_dist=want)
                np.testing.assert_array_equal(src_node.cpu().numpy(), want_src, err_msg=f"src_node at {threads}")
                np.testing.assert_array_equal(dst_node.cpu().numpy(), want_dst, err_msg=f"dst_node at {threads}")
                np.testing.assert_array_equal(hops.cpu().numpy().view(np.uint16), want_hops, err_msg=f"hops at {threads}")
                if want:
                    np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint16), want_dist, err_msg=f"dist at {threads}")
                else:
                    assert dist is None
    finally:
        ctx.set_option("ref_path_threads", 0)


def test_lattice_distances_cover_the_listed_inputs():
    """the restatement's own answers on the wall map show every kind of input the rule names (so the comparison above is
    not one of empty against empty)"""
    D, occ, stride, clearance, calls = MAPS["wall-13x11-stride2"]
    pts = calls[3][0]
    hops, src_node, _, dist, _ = P.hop_matrix(D, ORIGIN[:D], CELL, occ, stride, clearance, pts, pts)
    assert src_node.tolist() == [0, 4 * 6 + 5, -1, 6 + 4, -1, 0, -1, 4 * 6 + 5, -1, -1, -1, 2 * 6 + 2]
    assert hops[0, 5] == 0 and hops[0, 0] == 0 and hops[1, 7] == 0          # the same node
    assert hops[0, 3] == hops[3, 0] == 5 and hops[0, 11] == 2                 # through the gap (block (3, 2)); symmetric
    assert hops[0, 1] == hops[1, 3] == 0xFFFF                                 # into and out of the closed pocket
    assert (hops[[2, 4, 6, 8, 9, 10]] == 0xFFFF).all() and (dist[2] == 0xFFFF).all()  # points without a node
    assert (dist[1] != 0xFFFF).sum() == 1 and (dist[0] != 0xFFFF).sum() == 6 * 5 - 4 - 4  # four wall blocks; the pocket and its ring
    hops1 = P.hop_matrix(D, ORIGIN[:D], CELL, occ, 1, 0, pts, pts)[0]
    assert hops1[0, 6] != 0xFFFF and hops1[0, 9] != 0xFFFF and hops1[1, 7] == 1  # at stride 1 every cell is a node


def test_lattice_distances_argument_checks(ctx):
    from path_planning import _hip

    D, occ, stride, clearance, calls = MAPS["wall-13x11-stride2"]
    g = _hip.occupancy_grid(D, ORIGIN[:D], CELL, occ.shape[::-1])
    _, sat = ctx.occupancy_prepare(D, g, occ)
    edges = ctx.lattice_edges(D, g, sat, stride, clearance)
    src, dst = ctx.tensor(calls[0][0]), ctx.tensor(calls[0][1])
    for bad_stride, s, d in ((0, src, dst), (12, src, dst), (stride, src[:0], dst), (stride, src, dst[:0])):
        with pytest.raises(_hip.HipError) as e:
            ctx.lattice_distances(D, g, bad_stride, edges, s, d)
        assert e.value.code == -1, e.value
    gb = _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (256, 129))  # 33 024 nodes at stride 1
    with pytest.raises(_hip.HipError, match="nodes"):
        ctx.lattice_distances(2, gb, 1, edges, src, dst)


# ---- scp_assign_costs ----------------------------------------------------------------------------------------------------------
def _compare(name, goal_of, st, prices, ref, b=0):
    np.testing.assert_array_equal(goal_of[b], ref["goal_of"], err_msg=f"{name}: goal_of")
    np.testing.assert_array_equal(prices[b], ref["prices"], err_msg=f"{name}: prices")
    for k in STAT_KEYS:
        if k == "quantum":
            assert np.float64(st[k][b]).view(np.uint64) == np.float64(ref[k]).view(np.uint64), (name, k, st[k][b])
        else:
            assert int(st[k][b]) == int(ref[k]), (name, k, st[k][b], ref[k])


def _assign(ctx, cost, **kw):
    goal_of, st, prices = ctx.assign_costs(cost, want_prices=True, **kw)
    return goal_of.cpu().numpy(), st, prices.cpu().numpy()


@pytest.mark.parametrize("name", sorted(P.gpu_matrices()))
def test_assign_costs_equal_the_restatement(ctx, name):
    c = P.gpu_matrices()[name]
    goal_of, st, prices = _assign(ctx, c)
    _compare(name, goal_of, st, prices, P.reference(name))
    assert ctx.last_pair_ms() > 0.0
    goal_of32, st32, prices32 = _assign(ctx, c.astype(np.int32)[None])  # (the dtype of the call itself, batched)
    assert goal_of32.tobytes() == goal_of.tobytes() and st32.tobytes() == st.tobytes() and prices32.tobytes() == prices.tobytes()


@pytest.mark.parametrize("name", ["uniform-2d-65", "uniform-3d-130", "identical-goals-64", "reversed-lines-32"])
def test_assign_costs_give_the_bytes_of_assign_goals(ctx, name):
    """the two instantiations of one kernel: on the quantised costs of a coordinate case the matrix form finds the same
    assignment and total; prices, rounds and phases are the restatement's (eps_0 comes from max c, not from the box)"""
    start, goal = R.gpu_cases()[name]
    c, _, _ = R.quantise(start, goal)
    goal_of, st, prices = _assign(ctx, c)
    _compare(name, goal_of, st, prices, P.auction_costs(c))
    old = R.reference(name)
    assert int(st["cost_q"][0]) == old["cost_q"] and int(st["cost_q_identity"][0]) == old["cost_q_identity"]


def test_assign_costs_batch(ctx):
    mats = [P.gpu_matrices()["random-65"], P.random_matrix(65, 1, high=3), P.random_matrix(65, 2, high=2 ** 31, sentinel_rows=0)]
    goal_of, st, prices = _assign(ctx, np.stack(mats))
    _compare("batch-0", goal_of, st, prices, P.reference("random-65"), b=0)
    for b in (1, 2):
        _compare(f"batch-{b}", goal_of, st, prices, P.auction_costs(mats[b]), b=b)


def test_assign_costs_round_guard_and_bad_input(ctx):
    import torch

    from path_planning import _hip

    c = P.gpu_matrices()["all-equal-17"]  # everybody bids for goal 0: one round does not finish the phase
    ref = P.auction_costs(c, max_rounds_per_phase=1)
    goal_of, st, prices = _assign(ctx, c, max_rounds_per_phase=1)  # (returns: the call is SCP_OK)
    assert st["status"][0] == 1 and goal_of[0].tolist() == list(range(17)) and st["cost_q"][0] == st["cost_q_identity"][0]
    _compare("guard", goal_of, st, prices, ref)
    bad = P.gpu_matrices()["random-64"].copy()
    bad[63, 63] = -1
    for m in (bad, np.stack([P.gpu_matrices()["random-64"], bad])):
        with pytest.raises(_hip.HipError, match="negative") as e:
            ctx.assign_costs(m)
        assert e.value.code == -1, e.value
    with pytest.raises(_hip.HipError) as e:
        ctx.assign_costs(torch.zeros((1, 4097, 4097), dtype=torch.int32, device=ctx.tdev))
    assert e.value.code == -1, e.value
    for m in (np.zeros((3, 3)), np.zeros((3, 4), dtype=np.int64), np.full((2, 2), 2 ** 31, dtype=np.int64)):
        with pytest.raises(ValueError):
            ctx.assign_costs(m)
    # the call still works after the refusals
    goal_of, st, prices = _assign(ctx, P.gpu_matrices()["random-64"])
    _compare("after", goal_of, st, prices, P.reference("random-64"))


def test_assign_goals_costs_api(ctx):
    from path_planning.scenarios.assignment import assign_goals_costs

    c = P.gpu_matrices()["sentinel-rows-40"]
    ref = P.reference("sentinel-rows-40")
    goal_of, info = assign_goals_costs(c)
    assert isinstance(goal_of, np.ndarray) and goal_of.tolist() == ref["goal_of"].tolist()
    assert {k: info[k] for k in STAT_KEYS} == {k: ref[k] for k in STAT_KEYS} and info["assign_ms"] > 0.0
    assert info["cost_q"] < 40 * 999 + 1  # no sentinel entry in the optimum
    goal_of, info = assign_goals_costs(np.stack([c, c.T]))
    assert goal_of.shape == (2, 40) and goal_of[0].cpu().numpy().tolist() == ref["goal_of"].tolist()
    assert info["cost_q"].tolist() == [ref["cost_q"], P.auction_costs(c.T)["cost_q"]]


# ---- end to end: a wall with one gap ----------------------------------------------------------------------------------------------
class Fleet:
    """The map of reference_path_cases.WallScene (10 x 10 m, a wall across x = 5 with the gap 4 < y < 6.5).  Three vehicles
    start left of the wall low down, three right of it high up; three goals lie right of it low down, three left of it high
    up.  By straight-line distance every vehicle's nearest goal lies 2 m away behind the wall; by path length its own side's
    goals are nearer (checked on the CPU in test_the_fleet_is_what_it_claims)."""
    W = rc.WallScene
    p0 = np.array([[4.0, 0.75], [4.0, 1.75], [4.0, 2.75], [6.0, 7.25], [6.0, 8.25], [6.0, 9.25]])
    pf = np.array([[4.0, 7.25], [6.0, 0.75], [4.0, 8.25], [6.0, 1.75], [4.0, 9.25], [6.0, 2.75]])
    LINE = [1, 3, 5, 0, 2, 4]

    @classmethod
    def solver(cls, p0=None, pf=None, T=None, h=None):
        from path_planning.solvers.scp import SCP

        p0, pf = cls.p0 if p0 is None else p0, cls.pf if pf is None else pf
        s = SCP(n_vehicles=len(p0), time_horizon=cls.W.T if T is None else T, time_step=cls.W.h if h is None else h,
                min_distance=cls.W.R, space_dims=cls.W.space, verbose=False)
        s.set_initial_states(p0)
        s.set_final_states(pf)
        return s


def _cpu_pairings(occ, origin, cell, stride, p0, pf, power=2):
    """(hops, the pairing by straight-line distance, the pairing by path length) of the two restatements"""
    from path_planning.scenarios.assignment import path_costs

    hops = P.hop_matrix(2, list(origin), cell, occ, stride, 0, p0, pf)[0]
    d2 = ((p0[:, None, :] - pf[None, :, :]) ** 2).sum(-1)
    costs, how = path_costs(hops, d2, power)
    return hops, R.auction(p0, pf)["goal_of"], P.auction_costs(costs), how


def test_the_fleet_is_what_it_claims():
    from path_planning.scenarios.assignment import hop_totals

    occ, origin, cell = Fleet.W.grid()
    hops, line, path, _ = _cpu_pairings(occ, origin, cell, Fleet.W.stride(), Fleet.p0, Fleet.pf)
    assert line.tolist() == Fleet.LINE and path["goal_of"].tolist() != Fleet.LINE
    assert hop_totals(hops, path["goal_of"])["sum"] < hop_totals(hops, line)["sum"]
    assert hop_totals(hops)["n_unreachable"] == 0


def test_assign_goals_by_path(ctx):
    from path_planning.scenarios.assignment import describe, hop_totals

    occ, origin, cell = Fleet.W.grid()
    hops, line, path, how = _cpu_pairings(occ, origin, cell, Fleet.W.stride(), Fleet.p0, Fleet.pf)
    s = Fleet.solver()
    with pytest.raises(ValueError, match="set_obstacles"):
        s.assign_goals(cost="path")
    with pytest.raises(ValueError, match="cost="):
        s.assign_goals(cost="hops")
    s.set_obstacles(occ, origin, cell)
    assert s.assign_goals().tolist() == line.tolist() and "hops_assigned" not in s.assignment_info
    perm = s.assign_goals(cost="path")  # (recomputed from the goals as given: it does not compose with the call before)
    info = s.assignment_info
    assert perm.tolist() == path["goal_of"].tolist() and s.goal_assignment is perm
    np.testing.assert_array_equal(s.final_positions.reshape(-1, 2), Fleet.pf[perm])
    by_line, by_path, given = hop_totals(hops, line), hop_totals(hops, perm), hop_totals(hops)
    assert info["hops_assigned"] == {"sum": by_path["sum"], "max": by_path["max"]} and by_path["sum"] < by_line["sum"]
    assert info["hops_identity"] == {"sum": given["sum"], "max": given["max"]}
    assert info["n_unreachable_identity"] == info["n_unreachable_assigned"] == 0 and info["status"] == 0
    assert (info["tie_bits"], info["unreachable_cost"], info["max_hops"]) == (how["tie_bits"], how["unreachable_cost"], how["max_hops"])
    assert (info["cost_q"], info["rounds"], info["phases"]) == (path["cost_q"], path["rounds"], path["phases"])
    assert info["stride"] == Fleet.W.stride() and info["clearance"] == 0 and info["lattice"] == (20, 20)
    assert info["distances_ms"] > 0.0 and info["assign_ms"] > 0.0 and info["edges_ms"] > 0.0
    assert "line_after" in info and f"{given['sum']} -> {by_path['sum']} lattice moves" in describe(info)
    ref, found = s.find_reference()
    assert found["n_failed"] == 0 and found["edges_ms"] == 0.0  # every vehicle has its path; the masks were shared
    assert int(found["n_nodes"].sum()) == by_path["sum"] + 6   # a path of h hops has h + 1 nodes
    # power = 1 and another lattice go through the same calls
    hops1, _, path1, _ = _cpu_pairings(occ, origin, cell, 1, Fleet.p0, Fleet.pf, power=1)
    assert s.assign_goals(cost="path", stride=1, power=1).tolist() == path1["goal_of"].tolist()
    assert s.assignment_info["hops_assigned"]["sum"] == hop_totals(hops1, path1["goal_of"])["sum"]
    for bad in (dict(stride=0), dict(clearance=-1), dict(power=3)):
        with pytest.raises(ValueError):
            s.assign_goals(cost="path", **bad)
    s.close()


def test_a_goal_in_a_closed_pocket(ctx):
    occ, origin, cell = Fleet.W.grid()
    occ = occ.copy()
    occ[0, 28, 28:38] = occ[0, 37, 28:38] = occ[0, 28:38, 28] = occ[0, 28:38, 37] = 1  # a ring around the cells 29 .. 36
    pf = Fleet.pf.copy()
    pf[4] = [8.125, 8.125]
    hops, _, path, _ = _cpu_pairings(occ, origin, cell, Fleet.W.stride(), Fleet.p0, pf)
    assert (hops[:, 4] == 0xFFFF).all() and (np.delete(hops, 4, 1) != 0xFFFF).all()
    s = Fleet.solver(pf=pf)
    s.set_obstacles(occ, origin, cell)
    with pytest.raises(ValueError, match=r"no pairing connects every vehicle.* vehicle \d"):
        s.assign_goals(cost="path")
    assert s.goal_assignment is None  # nothing was permuted
    perm = s.assign_goals(cost="path", allow_unreachable=True)
    info = s.assignment_info
    assert perm.tolist() == path["goal_of"].tolist() and sorted(perm.tolist()) == list(range(6))
    assert info["n_unreachable_assigned"] == 1 and info["n_unreachable_identity"] == 1
    assert info["cost_q"] >= info["unreachable_cost"] and info["cost_q"] < 2 * info["unreachable_cost"]
    s.close()


def test_a_whole_solve_after_the_assignment(ctx):
    """N = 4, K = 20: the pairing by path length, the searched reference, corridors, the SCP solve and the corridor check"""
    occ, origin, cell = Fleet.W.grid()
    p0, pf = Fleet.p0[[0, 2, 3, 5]], Fleet.pf[[0, 1, 4, 5]]
    s = Fleet.solver(p0=p0, pf=pf, T=8.0, h=0.4)
    assert s.K == 20
    s.set_obstacles(occ, origin, cell)
    perm = s.assign_goals(cost="path")
    hops, line, path, _ = _cpu_pairings(occ, origin, cell, s.assignment_info["stride"], p0, pf)
    assert perm.tolist() == path["goal_of"].tolist() != line.tolist()
    co = s.set_corridors(reference="search")
    assert co["n_blocked"] == 0 and co["n_open"] == 0 and s.last_info["reference"]["n_failed"] == 0
    s.generate_trajectories(max_iterations=15)
    out = s.validate_corridor()
    assert out["inside"] and out["n_outside"] == 0
    assert s.validate_solution()["collision_free"]
    s.close()
