"""The weighted lattice search without a GPU: tests/weighted_path_ref.py against an independent Bellman-Ford, the octile
formula, symmetry and the hop search; that the cases of tests/weighted_path_cases.py expose what they are named for; the cost
limit; scenarios.assignment.length_costs; and the host surface (ABI rows, argument checks, CLI flags)."""
import inspect
import os
import re

import numpy as np
import pytest

import assign_paths_ref as ar
import reference_path_cases as rc
import reference_path_ref as rr
import weighted_path_cases as wc
import weighted_path_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in wc.all_cases()}


def _hop_want(c):
    return rc.Case("hops", c.D, c.occ, c.origin, c.cell, c.stride, c.clearance, c.K, c.p0, c.pf, max_path=c.max_path).want()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.nodes <= 200])
def test_dijkstra_equals_bellman_ford(name):
    c = CASES[name]
    want = c.want()
    seen = 0
    for i in range(c.N):
        if want["info"]["status"][i] in (0, 3, 4):
            goal = int(want["info"]["goal_node"][i])
            np.testing.assert_array_equal(want["cost"][i], wr.bellman_ford(c.L, want["edges"], want["pen"], goal))
            assert want["cost"][i, goal] == 0
            seen += 1
        else:
            assert (want["cost"][i] == wr.UNREACHED).all() and want["path_cost"][i] == wr.UNREACHED
    assert seen or name == "one_node" or (want["info"]["status"] != 0).all()


def test_every_case_is_covered_by_name():
    """the cases the rules name, and what each of them must show"""
    assert {"detour", "improve_late", "ties", "one_node", "start_is_goal", "status_1_2", "status_3", "status_4", "rand2d_13x11_s2",
            "rand3d_7_s1", "empty_map", "limit", "cap_8192", "cap_8193", "node_cap", "block_min", "wave2d_s9", "wave3d_s5",
            "thread3d_s3"} == set(CASES)
    st = {n: CASES[n].want()["info"]["status"].tolist() for n in ("one_node", "start_is_goal", "status_1_2", "status_3", "status_4")}
    assert st["one_node"] == [0, 0, 1, 2] and st["start_is_goal"] == [0, 0] and st["status_3"] == [3, 0, 0] and st["status_4"] == [4, 4, 0]
    assert set(st["status_1_2"]) == {0, 1, 2}
    assert CASES["cap_8192"].nodes == 8192 and CASES["cap_8193"].nodes == 8193 and CASES["node_cap"].nodes == rr.MAX_NODES
    assert CASES["rand2d_13x11_s2"].nodes % 64 and CASES["rand3d_7_s1"].nodes % 64 and CASES["rand3d_7_s1"].N == 5
    used = np.bitwise_or.reduce(CASES["rand3d_7_s1"].want()["edges"])
    assert int(used) & 0x7FFFFFF == 0x7FFFFFF  # all 26 directions and the node itself
    w = CASES["start_is_goal"].want()
    assert w["info"]["n_nodes"][0] == 1 and w["path_cost"][0] == 0 and (w["cost"][0] != wr.UNREACHED).all()
    for name in ("one_node", "status_1_2", "status_3", "status_4"):  # a failed vehicle's marked rows of ref stay
        c = CASES[name]
        failed = c.want()["info"]["status"] != 0
        assert failed.any()
        np.testing.assert_array_equal(c.want()["ref"][failed].view(np.uint64), c.ref_in()[failed].view(np.uint64))
        assert (c.want()["path"][failed] == -1).all() and (c.want()["info"]["n_nodes"][failed] == 0).all()


def test_detour_has_more_moves_than_the_hop_path():
    c = CASES["detour"]
    want, hop = c.want(), _hop_want(c)
    assert want["info"]["n_nodes"][0] == 9 > hop["info"]["n_nodes"][0] == 8
    # the cost along the fewest-move path is higher: a search that stops when the start is first reached is wrong
    nodes = hop["path"][0, :8]
    along = sum(wr.edge_cost(want["pen"], int(a), int(b), next(n for n in range(27) if rr.neighbour(c.L, int(a), n) == b))
                for a, b in zip(nodes[:-1], nodes[1:]))
    assert along > int(want["path_cost"][0]) == 1294


def test_improve_late_lowers_a_finite_cost():
    """synchronous Bellman-Ford rounds on the case: some node's first finite cost is lowered in a later round, and relaxing
    every node only once (as a level sweep does) ends with another field"""
    c = CASES["improve_late"]
    want = c.want()
    goal = int(want["info"]["goal_node"][0])
    INF = 1 << 50
    cost = np.full(c.nodes, INF, dtype=np.int64)
    cost[goal] = 0
    first = cost.copy()
    pen = want["pen"].astype(np.int64)
    for _ in range(c.nodes):
        new = cost.copy()
        for node in range(c.nodes):
            for n, nb in wr._neighbours(c.L, want["edges"], node):
                new[node] = min(new[node], cost[nb] + 2 * wr.W[wr.move_len(n)] + pen[node] + pen[nb])
        newly = (cost == INF) & (new != INF)
        first[newly] = new[newly]
        if (new == cost).all():
            break
        cost = new
    np.testing.assert_array_equal(np.where(cost == INF, wr.UNREACHED, cost), want["cost"][0])
    lowered = (first != INF) & (cost < first)
    assert lowered.any() and lowered[int(want["info"]["start_node"][0])]
    assert want["info"]["n_nodes"][0] == 14 > _hop_want(c)["info"]["n_nodes"][0] == 6
    assert first[int(want["info"]["start_node"][0])] == 6300 > want["path_cost"][0] == 5528


def test_block_min_is_not_the_centre_cell():
    c = CASES["block_min"]
    want = c.want()
    field = want["field"]
    assert field[0, 4, 4] == 4 and field[0, 5, 4] == 1 and wr.block_minimum(2, field, 3)[4] == 1
    assert want["rho"][4] == 1 and want["pen"][4] == 50 * (3 - 1) != 50 * (3 - 2)
    # the exact integer square root at the edges of its range
    for v in (0, 1, 2, 3, 4, 8, 9, 2**31 - 1, 65535**2 - 1, 65535**2, 2**32 - 1):
        f = np.full((1, 1, 1), v, dtype=np.uint32)
        pen, rho = wr.penalties(2, f, 1, 32768, 1)
        assert rho[0] ** 2 <= v < (rho[0] + 1) ** 2 and pen[0] == 32768 - min(int(rho[0]), 32768)


@pytest.mark.parametrize("name, node, centre, wave", [("wave2d_s9", 4, (13, 13, 0), True), ("wave3d_s5", 0, (2, 2, 2), True),
                                                      ("thread3d_s3", 13, (4, 4, 4), False)])
def test_large_blocks_have_their_minimum_off_the_centre(name, node, centre, wave):
    """the cases for the two forms of the penalties kernel (one wave per node from 64 cells per block on): the named block's
    minimum differs from its centre cell, lies only on cells a wave reads in its second pass, and the search passes that block
    or its neighbours with a penalty"""
    c = CASES[name]
    want = c.want()
    s, field = c.stride, want["field"]
    assert (s ** c.D >= 64) == wave
    X = rr.node_coords(c.L, node)
    block = field[X[2] * (s if c.D == 3 else 1):X[2] * (s if c.D == 3 else 1) + (s if c.D == 3 else 1), X[1] * s:(X[1] + 1) * s,
                  X[0] * s:(X[0] + 1) * s]
    least = int(block.min())
    assert least == 1 == want["rho"][node] ** 2 and int(field[centre[2], centre[1], centre[0]]) > least
    assert want["pen"][node] == c.weight * (c.prefer - 1) and wr.block_minimum(c.D, field, s)[node] == least
    where = [wc._block_cell(s, (x, y, z)) for z, y, x in np.argwhere(block == least)]
    assert min(where) >= (64 if wave else 2 * s * s)  # the second pass of the wave / the last layer of the thread's loop
    if wave:
        assert any(w % 64 >= 1 for w in where)
    assert (want["info"]["status"] == 0).all() and len(set(want["pen"].tolist())) >= 3
    if name == "wave2d_s9":  # vehicle 0 goes around the block whose centre cell alone would make it free
        assert want["path"][0, :3].tolist() == [3, 1, 5] and node not in want["path"][0]
    for i in range(c.N):  # the penalties decide the cost: without them the path is cheaper
        assert want["path_cost"][i] > wc.WCase(c.base).want()["path_cost"][i]


def test_octile_costs_on_open_maps():
    for name in ("ties", "empty_map", "cap_8192"):
        c = CASES[name]
        want = c.want()
        assert want["pen"] is None or not want["pen"].any()
        for i in range(c.N):
            goal = int(want["info"]["goal_node"][i])
            nodes = np.arange(c.nodes) if c.nodes <= 200 else np.array([0, 77, 4097, c.nodes - 1])
            assert [int(want["cost"][i, a]) for a in nodes] == [wc.octile(c.L, a, goal) for a in nodes]
            assert int(want["path_cost"][i]) == wc.octile(c.L, want["info"]["start_node"][i], goal)
    # direction order decides among equal costs: straight moves first
    w = CASES["ties"].want()
    assert w["path"][1, :6].tolist() == [6, 7, 8, 9, 16, 23] and w["path"][0, :6].tolist() == [0, 7, 14, 21, 28, 35]
    assert w["path_cost"].tolist() == [990, 816, 816, 420]


@pytest.mark.parametrize("name", ["detour", "improve_late", "rand2d_13x11_s2", "rand3d_7_s1", "status_3"])
def test_symmetry_of_the_edge_costs(name):
    c = CASES[name]
    want = c.want()
    for i in range(c.N):
        if want["info"]["status"][i] == 0:
            start, goal = int(want["info"]["start_node"][i]), int(want["info"]["goal_node"][i])
            assert wr.cost_field(c.L, want["edges"], want["pen"], start)[goal] == want["cost"][i, start] == want["path_cost"][i]


def test_straight_moves_only_is_140_per_hop():
    """a corridor one cell wide with two bends: only straight moves exist, so with zero penalties cost = 140 hops and the
    path is the hop search's"""
    occ = np.ones((1, 7, 9), dtype=np.uint8)
    occ[0, 1, 1:8] = occ[0, 1:6, 7] = occ[0, 5, 2:8] = 0
    base = rc.Case("corridor", 2, occ, [0.0, 0.0], 1.0, 1, 0, 7, [rc._centre(1, 1), rc._centre(7, 3)], [rc._centre(2, 5), rc._centre(1, 1)])
    want, hop = wc.WCase(base).want(), base.want()
    assert (np.bitwise_or.reduce(want["edges"]) & ~np.uint32(1 << 13 | 1 << 10 | 1 << 16 | 1 << 12 | 1 << 14)) == 0
    np.testing.assert_array_equal(want["path"], hop["path"])
    np.testing.assert_array_equal(want["info"], hop["info"])
    np.testing.assert_array_equal(want["path_cost"], 140 * (hop["info"]["n_nodes"].astype(np.uint32) - 1))
    for i in range(2):
        full = rr.distances(base.L, hop["edges"], int(hop["info"]["goal_node"][i]))
        reached = full != rr.UNREACHED
        np.testing.assert_array_equal(want["cost"][i][reached], 140 * full[reached].astype(np.uint32))
        assert (want["cost"][i][~reached] == wr.UNREACHED).all()
    zero = wc.WCase(base, prefer=0, weight=0).want()
    np.testing.assert_array_equal(zero["cost"], want["cost"])
    marked = wc.WCase(base).ref_in()
    np.testing.assert_array_equal(want["ref"].view(np.uint64), base.want()["ref"].view(np.uint64))
    assert not np.array_equal(marked, want["ref"])


def test_the_limit():
    """weight * prefer = 32768 on the serpentine: thousands of moves at the largest edge cost stay below 2^32 - 1, as does the
    bound for any path the lattice can hold; 32769 is refused"""
    c = CASES["limit"]
    want = c.want()
    assert (want["pen"][(want["edges"] >> np.uint32(13) & np.uint32(1)) != 0] == 32768).all()
    m = want["info"]["n_nodes"]
    assert m.max() > 2000
    reached = want["cost"] != wr.UNREACHED
    assert int(want["cost"][reached].max()) == int(want["path_cost"][0]) == (int(m[0]) - 1) * (140 + 65536) < 2**32 - 1
    assert (rr.MAX_NODES - 1) * (2 * wr.W[3] + 2 * wr.MAX_PRODUCT) < 2**32 - 1
    field = np.zeros((1, 4, 4), dtype=np.uint32)
    for prefer, weight in ((32769, 1), (1, 32769), (181, 182), (-1, 1), (1, -1)):
        with pytest.raises(ValueError):
            wr.penalties(2, field, 1, prefer, weight)
    assert wr.penalties(2, field, 1, 2, 16384)[0].max() == 32768


def test_cost_matrix_of_the_restatement():
    c = CASES["rand2d_13x11_s2"]
    want = c.want()
    src, dst = c.pf, np.concatenate([c.p0, c.pf[:2], [[99.0, 99.0]]])
    costs, src_node, dst_node, cost = wr.cost_matrix(c.D, c.origin, c.cell, c.dims, c.stride, want["edges"], want["pen"], src, dst)
    assert costs.shape == (5, 8) and dst_node[-1] == -1 and (costs[:, -1] == wr.UNREACHED).all()
    for a in range(5):
        np.testing.assert_array_equal(cost[a], want["cost"][a])  # (the goal of vehicle a is source a)
        assert costs[a, 5 + a] == 0 if a < 2 else True
        assert costs[a, a] == want["path_cost"][a]


def test_length_costs():
    from path_planning.scenarios.assignment import COST_UNREACHED, MAX_COST, length_costs

    U = COST_UNREACHED
    L = np.array([[140, 198, U], [338, 0, 280], [U, 99, 4000]], dtype=np.uint32)
    cost, how = length_costs(L)
    assert how == {"shift": 0, "unreachable_cost": 3 * 4000 + 1, "max_cost": 4000} and cost.dtype == np.int64
    np.testing.assert_array_equal(cost, [[140, 198, 12001], [338, 0, 280], [12001, 99, 4000]])
    np.testing.assert_array_equal(length_costs(L.view(np.int32))[0], cost)  # (the int32 view the binding returns)
    sq, how2 = length_costs(L, power=2)
    assert how2["shift"] == 0 and sq[2, 2] == 4000**2 and sq[0, 2] == 3 * 4000**2 + 1 == how2["unreachable_cost"]
    # U beats any assignment without an unreachable pair
    assert how["unreachable_cost"] > 3 * cost[L != U].max() - 1
    # the shift: the smallest t with N ((Lmax >> t)^power + 1) <= 2^31 - 1
    big = np.array([[136474728, 70076292], [5, U]], dtype=np.uint32)
    for power in (1, 2):
        cost, how = length_costs(big, power)
        t = how["shift"]
        assert 2 * ((136474728 >> t) ** power + 1) <= MAX_COST and (t == 0 or 2 * ((136474728 >> (t - 1)) ** power + 1) > MAX_COST)
        assert cost.max() == how["unreachable_cost"] == 2 * (136474728 >> t) ** power + 1 <= MAX_COST
        assert cost[1, 0] == (5 >> t) ** power
    assert length_costs(big, 1)[1]["shift"] == 0 and length_costs(big, 2)[1]["shift"] == 13
    worst = np.full((4096, 4096), 2**32 - 2, dtype=np.uint32)
    cost, how = length_costs(worst, 2)
    assert cost.max() * 4096 + 4096 <= MAX_COST and how["max_cost"] == 2**32 - 2
    none, how = length_costs(np.full((2, 2), U, dtype=np.uint32))
    assert how == {"shift": 0, "unreachable_cost": 1, "max_cost": 0} and (none == 1).all()
    for bad in (dict(costs=L.astype(np.float64)), dict(costs=L[:2]), dict(costs=L, power=3), dict(costs=L, power=True),
                dict(costs=np.array([[-2, 1], [1, 1]], dtype=np.int64)), dict(costs=np.array([[2**32, 1], [1, 1]], dtype=np.int64))):
        with pytest.raises(ValueError):
            length_costs(**bad)
    assert list(inspect.signature(length_costs).parameters.items())[1][1].default == 1


def test_two_gap_scene_on_the_cpu():
    """the near gap is narrow: the fewest-move path passes nodes with rho < 2; a path with rho >= 2 everywhere exists and the
    weighted search with keep_clear = 2 finds it"""
    T = wc.TwoGaps
    c = T.case()
    want, hop = c.want(), _hop_want(c)
    assert c.L == (20, 20, 1) and (want["info"]["status"] == 0).all() and (hop["info"]["status"] == 0).all()
    for i in range(T.N):
        assert (want["rho"][want["path"][i, :want["info"]["n_nodes"][i]]] >= 2).all()
        assert (want["rho"][hop["path"][i, :hop["info"]["n_nodes"][i]]] < 2).any()
        assert want["info"]["n_nodes"][i] + 1 <= T.K  # E <= K: no blocked segment at any clearance


def test_assign_scene_on_the_cpu():
    A = wc.AssignScene
    want = A.want()
    i = np.arange(A.N)
    H, L = want["hops"].astype(np.int64), want["lengths"].astype(np.int64)
    assert (H != ar.UNREACHED).all() and (L != wr.UNREACHED).all()
    assert want["by_path"].tolist() == [1, 0, 2] and want["by_length"].tolist() == [2, 0, 1]
    assert H[i, want["by_path"]].sum() == 39 < H[i, want["by_length"]].sum() == 40
    assert L[i, want["by_length"]].sum() == 6518 < L[i, want["by_path"]].sum() == 6552
    best = min(L[i, list(p)].sum() for p in __import__("itertools").permutations(range(A.N)))
    assert best == 6518


def test_the_abi_rows_and_the_python_surface():
    from path_planning import _hip
    from path_planning.cli import compute_trajectories as ct
    from path_planning.scenarios.assignment import describe
    from path_planning.solvers._obstacles import ObstacleMap, search_metric
    from path_planning.solvers.scp import SCP

    header = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert _hip.ABI_VERSION == 7 == int(re.search(r"#define SCP_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define SCP_PENALTY_MAX_PRODUCT (\d+)", header).group(1)) == _hip.PENALTY_MAX_PRODUCT == wr.MAX_PRODUCT
    assert _hip.COST_UNREACHED == wr.UNREACHED == 0xFFFFFFFF and _hip.MOVE_WEIGHTS == wr.W[1:] == (70, 99, 121)
    lib = _hip.load_library()
    for name, arity in (("scp_lattice_penalties", 8), ("scp_reference_paths_weighted", 17), ("scp_lattice_costs", 14)):
        assert name in _hip.EXPORTS and len(_hip.PROTOTYPES[name][1]) == arity and hasattr(lib, name)
        assert re.search(rf"^int {name}\(scp_ctx\* ctx,", header, flags=re.M), name
    for name in ("lattice_penalties", "reference_paths_weighted", "lattice_costs"):
        assert callable(getattr(_hip.Context, name))
    sig = inspect.signature(_hip.Context.reference_paths_weighted).parameters
    assert [sig[k].default for k in ("pen", "want_path", "want_cost")] == [None, True, False]
    assert list(inspect.signature(ObstacleMap.penalties).parameters)[1:] == ["stride", "prefer", "weight"]
    sig = inspect.signature(SCP.set_search_metric).parameters
    assert [(k, p.default) for k, p in sig.items()][1:] == [("metric", "hops"), ("keep_clear", 0), ("clear_weight", 1.0)]
    assert SCP._metric == ("hops", 0, 0)

    assert search_metric("hops", 0, 1.0) == (0, 70) and search_metric("length", 3, 0.5) == (3, 35)
    assert search_metric("length", 468, 1.0) == (468, 70) and search_metric("length", 2, 0) == (2, 0)
    for bad in (("metres", 0, 1.0), ("hops", 1, 1.0), ("length", -1, 1.0), ("length", 1.0, 1.0), ("length", True, 1.0),
                ("length", 2, -1.0), ("length", 2, "1"), ("length", 2, float("inf")), ("length", 469, 1.0), ("length", 1, 500.0)):
        with pytest.raises(ValueError):
            search_metric(*bad)

    class TwoRanks:
        world = 2

    s = SCP.__new__(SCP)
    s.shard, s.N = TwoRanks(), 3
    for call in (lambda: s.set_search_metric("length"), lambda: s.assign_goals(cost="length")):
        with pytest.raises(ValueError, match="one rank"):
            call()

    parser = ct.build_parser()
    args = parser.parse_args(["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "length", "--corridor-keep-clear",
                              "2", "--corridor-clear-weight", "0.5"])
    assert (args.corridor_metric, args.corridor_keep_clear, args.corridor_clear_weight) == ("length", 2, 0.5)
    assert ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    args = parser.parse_args(["--assign-goals", "--assign-cost", "length", "--obstacle-discs", "5,5,1", "--corridor-keep-clear", "1"])
    assert args.assign_cost == "length" and ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    none = parser.parse_args([])
    assert none.corridor_metric is None and none.corridor_keep_clear is None and none.corridor_clear_weight is None
    for argv in (["--corridor-metric", "length"], ["--obstacle-discs", "5,5,1", "--corridor-metric", "length"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-keep-clear", "1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "hops", "--corridor-keep-clear", "1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "length", "--corridor-keep-clear", "-1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "length", "--corridor-clear-weight", "2"],
                 ["--assign-cost", "length", "--obstacle-discs", "5,5,1"], ["--assign-goals", "--assign-cost", "length"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    with pytest.raises(SystemExit):
        parser.parse_args(["--corridor-metric", "metres"])

    line = {"min_approach": 0.5, "arg_i": 0, "arg_j": 1, "n_close": 0, "n_opposed": 2}
    info = {"quantum": 1.0, "status": 0, "phases": 3, "rounds": 11, "line_before": line, "line_after": dict(line, n_opposed=0),
            "length_identity": {"sum": 6552, "max": 3848}, "length_assigned": {"sum": 6518, "max": 3230},
            "n_unreachable_identity": 0, "n_unreachable_assigned": 0, "distances_ms": 0.25, "assign_ms": 0.5}
    assert describe(info).startswith("Goal assignment by weighted path length: 6552 -> 6518 in lattice costs")
