"""Reference paths by a lattice search, without a GPU: the properties of the restatement (tests/reference_path_ref.py) that the
device code is held to exactly, the corridor property that makes such a path a usable reference, the struct layout, the
Python surface and the end-to-end scene."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path

import corridor_cases as cc
import corridor_ref as cr
import reference_path_cases as rc
import reference_path_ref as rr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scp_hip.h")

CASES = {c.name: c for c in rc.all_cases()}
SMALL = [n for n, c in CASES.items() if c.nodes <= 4096 and c.N <= 10]


def _graph(L, edges):
    """the lattice as a sparse adjacency matrix, from the bits alone"""
    rows, cols = [], []
    for node in range(edges.size):
        for n in range(27):
            if n != rr.SELF and int(edges[node]) >> n & 1:
                rows.append(node)
                cols.append(rr.neighbour(L, node, n))
    return sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(edges.size, edges.size))


def test_direction_order():
    assert rr.DIRECTION_ORDER[:6] == [4, 10, 12, 14, 16, 22] and len(rr.DIRECTION_ORDER) == 26 and rr.SELF not in rr.DIRECTION_ORDER
    assert [n for n in rr.DIRECTION_ORDER if rr.direction(n)[2] == 0] == [10, 12, 14, 16, 9, 11, 15, 17]
    assert rr.direction(0) == (-1, -1, -1) and rr.direction(13) == (0, 0, 0) and rr.direction(26) == (1, 1, 1)


@pytest.mark.parametrize("name", ["rand2d_13x11_s2_c1", "rand2d_50x37_s3_c0", "rand3d_5_s1_c1", "rand3d_16_s2_c0"])
def test_edges_by_brute_force(name):
    """every bit from the cells themselves: the neighbour lies in the lattice and the grown, clipped range of the two blocks is
    free; symmetric; bit 13 implied by every other bit; a 2-D mask has no bit with dz != 0"""
    c = CASES[name]
    edges, occ, s, cl = c.want()["edges"], c.occ, c.stride, c.clearance
    for node in range(c.nodes):
        X = rr.node_coords(c.L, node)
        for n in range(27):
            Y = [X[d] + rr.direction(n)[d] for d in range(3)]
            inside = all(0 <= Y[d] < c.L[d] for d in range(3))
            free = False
            if inside:
                lo = [max(min(X[d], Y[d]) * s - cl, 0) if d < c.D else 0 for d in range(3)]
                hi = [min(max(X[d], Y[d]) * s + s - 1 + cl, c.dims[d] - 1) if d < c.D else 0 for d in range(3)]
                free = occ[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].sum() == 0
            assert bool(int(edges[node]) >> n & 1) == (inside and free), (node, n)
            if inside and free:
                assert int(edges[rr.node_id(c.L, Y)]) >> (26 - n) & 1 and int(edges[node]) >> rr.SELF & 1
    assert not (edges >> np.uint32(27)).any()


@pytest.mark.parametrize("name", SMALL)
def test_dist_paths_and_points(name):
    c = CASES[name]
    w = c.want()
    edges, info = w["edges"], w["info"]
    graph = _graph(c.L, edges)
    assert (graph != graph.T).nnz == 0
    for i in range(c.N):
        status, m, start, goal = (int(v) for v in info[i])
        if status in (1, 2):
            assert m == 0 and (w["path"][i] == -1).all() and (w["dist"][i] == rr.UNREACHED).all()
            continue
        # dist against an independent shortest-path computation
        d = shortest_path(graph, unweighted=True, indices=goal)
        full = np.where(np.isinf(d), rr.UNREACHED, d).astype(np.uint16)
        np.testing.assert_array_equal(rr.distances(c.L, edges, goal), full)
        cut = full.copy()
        if full[start] != rr.UNREACHED:
            cut[full > full[start]] = rr.UNREACHED
        np.testing.assert_array_equal(w["dist"][i], cut)
        if status != 0:
            assert status == (3 if full[start] == rr.UNREACHED else 4) and m == 0 and (w["path"][i] == -1).all()
            assert status == 3 or int(full[start]) + 1 > c.max_path
            np.testing.assert_array_equal(w["ref"][i].view(np.uint64), c.ref_in()[i].view(np.uint64))
            continue
        path = w["path"][i]
        assert m == int(full[start]) + 1 <= c.max_path and path[0] == start and path[m - 1] == goal and (path[m:] == -1).all()
        for t in range(m - 1):
            a, b = int(path[t]), int(path[t + 1])
            assert full[b] == full[a] - 1
            steps = [n for n in rr.DIRECTION_ORDER if int(edges[a]) >> n & 1 and full[rr.neighbour(c.L, a, n)] == full[a] - 1]
            assert rr.neighbour(c.L, a, steps[0]) == b  # a chain of set edges, the first in direction order
        ref = w["ref"][i]
        np.testing.assert_array_equal(ref[0].view(np.uint64), c.p0[i].view(np.uint64))
        np.testing.assert_array_equal(ref[c.K].view(np.uint64), c.pf[i].view(np.uint64))
        # every point lies on the polyline p0, centres, pf
        V = np.vstack([c.p0[i]] + [[c.origin[d] + c.cell * c.stride * (rr.node_coords(c.L, int(n))[d] + 0.5) for d in range(c.D)]
                                   for n in path[:m]] + [c.pf[i]])
        for j in range(c.K + 1):
            q = min(j * (m + 1) // c.K, m)
            a, b = V[q], V[q + 1]
            t = np.clip(np.dot(ref[j] - a, b - a) / max(np.dot(b - a, b - a), 1e-300), 0.0, 1.0)
            assert np.linalg.norm(a + t * (b - a) - ref[j]) < 1e-9
    assert w["n_failed"] == int((info["status"] != 0).sum())


def test_forced_statuses():
    assert CASES["one_node"].want()["info"]["status"].tolist() == [0, 0, 1, 2]
    assert CASES["one_node"].want()["info"]["n_nodes"].tolist() == [1, 1, 0, 0]
    w = CASES["status_1_2"].want()["info"]
    assert w["status"].tolist() == [1, 1, 1, 2, 2, 2, 1, 0]
    assert w["start_node"].tolist() == [6, -1, -1, 0, 0, 0, 6, 0] and w["goal_node"].tolist() == [-1, -1, -1, -1, -1, 6, -1, 11]
    assert CASES["closed_wall"].want()["info"]["status"].tolist() == [3, 0, 0]
    assert CASES["max_path_short"].want()["info"]["status"].tolist() == [4, 4, 0]
    assert CASES["max_path_exact"].want()["info"]["n_nodes"].tolist() == [12, 12, 7]
    for K in (1, 2, 3):
        assert (CASES[f"long_path_K{K}"].want()["info"]["n_nodes"] + 1 > 5 * K).all()  # E far beyond K
    s = CASES["serpentine"].want()["info"]
    assert s["status"].tolist() == [0, 0, 0] and s["n_nodes"][0] > 2000 and s["n_nodes"][2] == 1
    assert CASES["node_cap"].nodes == rr.MAX_NODES and CASES["node_cap"].want()["info"]["n_nodes"].tolist() == [256, 239]
    assert CASES["many_vehicles"].N == 600


def _property_cases():
    """random maps with found paths: (D, origin, cell, sat, stride, clearance, K, ref row, E)"""
    rng = np.random.default_rng(2024)
    out = []
    for trial in range(400):
        D = 2 + trial % 2
        dims = tuple(int(rng.integers(6, 15)) for _ in range(D)) if D == 2 else tuple(int(rng.integers(4, 8)) for _ in range(D))
        stride, clearance = int(rng.integers(1, 4)), int(rng.integers(0, 3))
        if min(dims) < stride:
            continue
        K = int(rng.choice([2, 3, 4, 6, 10, 25]))
        occ = cc.random_grid(rng, dims, rng.choice([0.03, 0.08, 0.15]))
        origin, cell = list(rng.uniform(-2, 2, D)), float(rng.choice([0.25, 0.4, 1.0]))
        sat = cr.summed_table(occ)
        edges = rr.lattice_edges(D, sat, stride, clearance)
        L = rr.lattice(D, (list(dims) + [1])[:3], stride)
        passable = np.nonzero(edges >> np.uint32(rr.SELF) & np.uint32(1))[0]
        if passable.size < 2:
            continue
        N = 5
        p0 = rc.block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
        pf = rc.block_points(rng, D, origin, cell, stride, L, rng.choice(passable, N))
        straight = p0[:, None, :] + (np.arange(K + 1) / K)[None, :, None] * (pf - p0)[:, None, :]
        ref, _, info, _, _ = rr.reference_paths(D, origin, cell, sat, stride, edges, p0, pf, K, edges.size, straight)
        for i in np.nonzero(info["status"] == 0)[0]:
            out.append((D, origin, cell, sat, stride, clearance, K, ref[i], int(info["n_nodes"][i]) + 1))
    return out


def test_corridor_property():
    """A vehicle whose path has E <= K has no blocked corridor segment, at any clearance; the same whenever
    2 clearance >= stride ceil(E / K)."""
    n_first, n_second, by_dim = 0, 0, {2: 0, 3: 0}
    for D, origin, cell, sat, stride, clearance, K, ref, E in _property_cases():
        first = E <= K
        second = 2 * clearance >= stride * -(-E // K)
        if not (first or second):
            continue
        _, n_blocked = cr.corridor_boxes(D, origin, cell, sat, ref[None], 0)
        assert n_blocked == 0, (D, stride, clearance, K, E)
        n_first += first
        n_second += second and not first
        by_dim[D] += 1
    print(f"corridor property: {n_first} vehicles with E <= K, {n_second} more with 2 c >= s ceil(E / K); by dimension {by_dim}")
    assert n_first + n_second >= 500 and n_second >= 50 and min(by_dim.values()) >= 100


def test_struct_layout_matches_the_header(tmp_path):
    from path_planning import _hip

    names = ["status", "n_nodes", "start_node", "goal_node"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(scp_path_info), ' +
                   ", ".join(f"offsetof(scp_path_info, {f})" for f in names) + ', SCP_LATTICE_MAX_NODES);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _hip.PathInfo
    assert got[:5] == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in names] == [16, 0, 4, 8, 12]
    assert _hip.PATH_INFO_DTYPE == rr.PATH_INFO_DTYPE and _hip.PATH_INFO_DTYPE.itemsize == 16
    assert [_hip.PATH_INFO_DTYPE.fields[f][1] for f in names] == got[1:5]
    assert got[5] == _hip.LATTICE_MAX_NODES == rr.MAX_NODES == 32768


def test_default_search_stride():
    from path_planning.scenarios.obstacles import default_search_stride

    assert default_search_stride((40, 40), 40, 2) == 2        # 40 / 2 <= 38
    assert default_search_stride((40, 40), 50, 2) == 1
    assert default_search_stride((1024, 1024), 50, 2) == 22   # 1024 / 22 <= 48 (the node cap alone would allow 6)
    assert default_search_stride((1024, 1024), 500, 2) == 6   # 170 x 170 nodes
    assert default_search_stride((256, 256, 256), 50, 3) == 8
    assert default_search_stride((256, 128), 500, 2) == 1     # exactly 32768 nodes
    assert default_search_stride((257, 128), 500, 2) == 2
    assert default_search_stride((30, 20), 1, 2) == 30 and default_search_stride((30, 20), 3, 2) == 30
    for dims, K, D in (((333, 77), 17, 2), ((90, 80, 70), 9, 3)):
        s = default_search_stride(dims, K, D)
        ok = lambda t: np.prod([n // t for n in dims]) <= 32768 and max(dims) / t <= max(K - 2, 1)
        assert ok(s) and not any(ok(t) for t in range(1, s))
    with pytest.raises(ValueError):
        default_search_stride((40,), 40, 2)


def test_python_surface():
    from path_planning import _hip
    from path_planning.cli import compute_trajectories as ct
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.find_reference)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("stride", None), ("clearance", 0), ("max_path", None),
                                                                       ("allow_unreachable", False)]
    sig = inspect.signature(SCP.set_corridors)
    assert [sig.parameters[k].default for k in ("reference", "max_grow", "pad", "allow_open")] == [None, 8, 0.02, False]
    for name in ("scp_lattice_edges", "scp_reference_paths"):
        assert name in _hip.EXPORTS
    assert callable(_hip.Context.lattice_edges) and callable(_hip.Context.reference_paths)
    assert set(_hip.PATH_STATUS) == {0, 1, 2, 3, 4}
    g = _hip.occupancy_grid(2, [0.0, 0.0], 0.5, (13, 11))
    assert _hip.lattice_shape(2, g, 3) == (4, 3, 1) and _hip.lattice_shape(3, _hip.occupancy_grid(3, [0] * 3, 1.0, (9, 8, 7)), 2) == (4, 4, 3)

    # set_corridors(reference="search") goes through find_reference with its defaults; any other string is an error
    class OneRank:
        world = 1

    s = SCP.__new__(SCP)
    s.shard = OneRank()
    calls = []

    def fake(*a, **kw):
        calls.append((a, kw))
        raise RuntimeError("find_reference was called")

    s.find_reference = fake
    with pytest.raises(RuntimeError, match="find_reference was called"):
        s.set_corridors(reference="search")
    assert calls == [((), {})]
    with pytest.raises(ValueError, match="search"):
        s.set_corridors(reference="straight")
    s._obstacles = None
    del s.find_reference
    with pytest.raises(ValueError, match="set_obstacles"):
        s.find_reference()

    parser = ct.build_parser()
    args = parser.parse_args(["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-stride", "3", "--corridor-clearance", "1"])
    assert args.corridor_search and args.corridor_stride == 3 and args.corridor_clearance == 1
    assert ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    none = parser.parse_args([])
    assert not none.corridor_search and none.corridor_stride is None and none.corridor_clearance is None
    assert ct.obstacle_discs(parser, none) is None
    for argv in (["--corridor-search"], ["--obstacle-discs", "5,5,1", "--corridor-stride", "3"],
                 ["--obstacle-discs", "5,5,1", "--corridor-clearance", "1"], ["--corridor-stride", "2"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))


def test_wall_scene_on_the_cpu():
    """the scene of the GPU end-to-end test: the straight lines are blocked, the searched reference has corridors without a
    blocked segment or an open state, and its boxes are not empty inside the workspace"""
    from path_planning.solvers.scp import check_position_boxes, corridor_shrink, straight_reference

    W = rc.WallScene
    c = CASES["wall_scene"]
    w = c.want()
    occ, origin, cell = W.grid()
    assert occ.shape == (1, 40, 40) and c.stride == 2 and c.L == (20, 20, 1) and c.max_path == 320
    free = np.nonzero(occ[0, :, 20] == 0)[0]
    assert free.min() == 17 and free.max() == 24  # the gap: 4.25 m .. 6.25 m
    _, blocked_straight = cr.corridor_boxes(W.D, origin, cell, w["sat"], straight_reference(W.p0, W.pf, W.K), W.max_grow)
    assert blocked_straight > 0
    assert (w["info"]["status"] == 0).all() and (w["info"]["n_nodes"] + 1 <= W.K).all()
    cells, n_blocked = cr.corridor_boxes(W.D, origin, cell, w["sat"], w["ref"], W.max_grow)
    lo, hi, n_open = cr.state_boxes(W.D, origin, cell, cells, corridor_shrink(-15.0, 15.0, W.h, W.pad))
    assert n_blocked == 0 and n_open == 0
    check_position_boxes(W.N, W.K, W.D, W.space[:2], W.space[2:], lo, hi)
    # every reference point keeps the body (radius R / 2) off the wall: it lies in a free cell
    idx = np.floor((w["ref"] - origin) / cell).astype(int)
    assert (occ[0, idx[..., 1], idx[..., 0]] == 0).all()
    # every vehicle uses the gap
    for i in range(W.N):
        at_wall = w["ref"][i][np.abs(w["ref"][i][:, 0] - 5.0) < 0.3]
        assert at_wall.size and (at_wall[:, 1] > 4.25).all() and (at_wall[:, 1] < 6.25).all()
