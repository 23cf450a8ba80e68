"""Static obstacles without a GPU: the properties of the numpy restatement (tests/corridor_ref.py) that the device code is
held to bit for bit, the rasteriser, the chord bound behind the shrink, and the host-side errors of the Python surface."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import corridor_cases as cc
import corridor_ref as cr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scp_hip.h")

GRIDS = [((37, 29), 2), ((13, 11, 9), 3)]


def _case(seed, dims, D, N=5, K=7):
    rng = np.random.default_rng(seed)
    occ = cc.random_grid(rng, dims)
    origin, cell = [-1.5, 0.25, 2.0][:D], 0.4
    ref = cc.random_walk_reference(rng, occ, D, origin, cell, N, K)
    return occ, origin, cell, ref


def _count(occ, lo, hi):
    return int(occ[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].sum())


def test_summed_table_counts_by_brute_force():
    rng = np.random.default_rng(0)
    occ = cc.random_grid(rng, (13, 11, 9), 0.3)
    sat = cr.summed_table(occ)
    assert sat.dtype == np.int32 and sat[-1, -1, -1] == occ.sum()
    for _ in range(200):
        a = [int(rng.integers(0, n)) for n in (13, 11, 9)]
        b = [int(rng.integers(a[d], n)) for d, n in enumerate((13, 11, 9))]
        assert cr.occupied_in(sat, a, b) == _count(occ, a, b)


@pytest.mark.parametrize("dims,D", GRIDS)
@pytest.mark.parametrize("max_grow", [0, 1, 3, 8])
def test_boxes_are_free_contain_the_seeds_and_are_locally_maximal(dims, D, max_grow):
    occ, origin, cell, ref = _case(3, dims, D)
    gd = (list(dims) + [1])[:3]
    cells, n_blocked = cr.corridor_boxes(D, origin, cell, cr.summed_table(occ), ref, max_grow)
    judged = 0
    for i in range(cells.shape[0]):
        for g in range(cells.shape[1]):
            lo, hi = cells[i, g, :3], cells[i, g, 3:]
            seeds = [[int(np.floor((ref[i, g + e, d] - origin[d]) / cell)) for d in range(D)] + [0] * (3 - D) for e in (0, 1)]
            s_lo, s_hi = np.minimum(*seeds), np.maximum(*seeds)
            if hi[0] < lo[0]:  # the walk stays on free cells, but a diagonal step may span an occupied one: blocked
                assert tuple(cells[i, g]) == cr.BLOCKED and _count(occ, s_lo, s_hi) > 0
                continue
            judged += 1
            assert _count(occ, lo, hi) == 0
            assert (lo <= s_lo).all() and (hi >= s_hi).all() and (lo >= 0).all() and (hi < gd).all()
            assert (s_lo - lo <= max_grow).all() and (hi - s_hi <= max_grow).all()
            for d in range(D):  # every direction is stopped by max_grow, the grid edge or an occupied slab
                a, b = lo.copy(), hi.copy()
                a[d] = b[d] = lo[d] - 1
                assert s_lo[d] - lo[d] == max_grow or lo[d] == 0 or _count(occ, a, b) > 0
                a, b = lo.copy(), hi.copy()
                a[d] = b[d] = hi[d] + 1
                assert hi[d] - s_hi[d] == max_grow or hi[d] == gd[d] - 1 or _count(occ, a, b) > 0
    assert judged + n_blocked == cells.shape[0] * cells.shape[1] and judged > n_blocked


def test_forced_cases_of_the_box_rule():
    occ = np.zeros((1, 6, 8), dtype=np.uint8)
    occ[0, 2, 3] = 1
    sat = cr.summed_table(occ)
    origin, cell = [0.0, 0.0], 1.0
    ref = np.array([
        [[0.5, 0.5], [1.5, 0.5], [3.5, 2.5]],     # second segment: a seed on the occupied cell
        [[0.5, 0.5], [-0.5, 0.5], [0.5, 0.5]],    # a reference point outside the grid (both segments)
        [[0.5, 0.5], [np.nan, 0.5], [0.5, 0.5]],  # a NaN coordinate
        [[2.5, 1.5], [4.5, 3.5], [4.5, 3.5]],     # two free cells whose seed range spans the occupied one; then a free seed
        [[7.5, 5.5], [7.5, 5.5], [8.0, 5.5]],     # the last cell; x = 8.0 is outside (cell 8 of 8)
    ])
    cells, n_blocked = cr.corridor_boxes(2, origin, cell, sat, ref, 8)
    blocked = cells[..., 3] < cells[..., 0]
    assert blocked.tolist() == [[False, True], [True, True], [True, True], [True, False], [False, True]]
    assert n_blocked == 7 and (cells[blocked] == cr.BLOCKED).all()
    # an all-free grid: every box reaches every face within max_grow
    free = cr.summed_table(np.zeros((1, 6, 8), dtype=np.uint8))
    cells, n_blocked = cr.corridor_boxes(2, origin, cell, free, ref[:1], 8)
    assert n_blocked == 0 and (cells[0] == [0, 0, 0, 7, 5, 0]).all()


def test_state_boxes_open_entries():
    cells = np.array([[[0, 0, 0, 3, 3, 0], [2, 1, 0, 5, 2, 0], cr.BLOCKED, [4, 4, 0, 6, 6, 0], [6, 4, 0, 8, 6, 0]]], dtype=np.int32)
    lo, hi, n_open = cr.state_boxes(2, [1.0, -1.0], 0.5, cells, 0.1)
    assert np.isinf(lo[0, 0]).all() and n_open == 2  # states 2 and 3: a blocked neighbour (state 0 does not count)
    assert np.isinf(lo[0, [2, 3]]).all() and np.isinf(hi[0, [2, 3]]).all()
    np.testing.assert_array_equal([lo[0, 4, 0], hi[0, 4, 0]], [1.0 + 0.5 * 6 + 0.1, 1.0 + 0.5 * 7 - 0.1])  # one column of cells
    np.testing.assert_array_equal(lo[0, 1], [1.0 + 0.5 * 2 + 0.1, -1.0 + 0.5 * 1 + 0.1])
    np.testing.assert_array_equal(hi[0, 1], [1.0 + 0.5 * 4 - 0.1, -1.0 + 0.5 * 3 - 0.1])
    lo, hi, n_open = cr.state_boxes(2, [1.0, -1.0], 0.5, cells, 0.3)  # 2 shrink > the width of state 4's intersection
    assert n_open == 3 and np.isinf(lo[0, 4]).all() and np.isinf(hi[0, 4]).all()


def test_chord_bound():
    """a quadratic with second derivative a leaves the chord of its end values by at most |a| h^2 / 8"""
    rng = np.random.default_rng(5)
    n = 10_000
    p, v, a = rng.normal(0, 5, n), rng.normal(0, 2, n), rng.uniform(-15, 15, n)
    h = rng.uniform(0.05, 0.5, n)
    t = np.linspace(0.0, 1.0, 65)[:, None] * h
    q = p + t * v + 0.5 * t * t * a
    chord = q[0] + (t / h) * (q[-1] - q[0])
    dev = np.abs(q - chord).max(axis=0)
    bound = np.abs(a) * h * h / 8
    assert (dev <= bound * (1 + 1e-9) + 1e-12).all()
    assert (dev >= 0.999 * bound).all()  # (attained at the midpoint, which the sampling holds)


@pytest.mark.parametrize("dims,D", GRIDS)
def test_end_states_in_shrunk_boxes_keep_the_segment_inside(dims, D):
    """Section 3's property: end states inside the shrunk state boxes and |a| <= acc_max put the whole segment, as judged by
    the exact check, inside its un-shrunk box."""
    rng = np.random.default_rng(11)
    occ, origin, cell, ref = _case(7, dims, D, N=6, K=9)
    h, amax = 0.2, 15.0
    shrink = amax * h * h / 8
    cells, _ = cr.corridor_boxes(D, origin, cell, cr.summed_table(occ), ref, 3)
    lo, hi, _ = cr.state_boxes(D, origin, cell, cells, shrink)
    L, H = cr.segment_boxes_metres(D, origin, cell, cells)
    judged = 0
    for i in range(cells.shape[0]):
        for g in range(1, cells.shape[1] - 1):  # both end states have a box
            if np.isinf(lo[i, g]).any() or np.isinf(lo[i, g + 1]).any():
                continue
            for _ in range(20):
                a = rng.uniform(-amax, amax, D)
                p = rng.uniform(lo[i, g], hi[i, g])
                end = rng.uniform(lo[i, g + 1], hi[i, g + 1])
                v = (end - p - 0.5 * h * h * a) / h
                assert cr.segment_excess(D, h, L[i, g], H[i, g], p, v, a) <= 1e-12
                judged += 1
    assert judged > 200


def test_check_reference_on_constructed_segments():
    cells = np.array([[[2, 2, 0, 5, 3, 0], cr.BLOCKED, [2, 2, 0, 5, 3, 0]]], dtype=np.int32)  # box [1, 3] x [1, 2] at cell 0.5
    pos = np.array([[[1.5, 1.5], [0.0, 0.0], [1.0, 2.0]]])
    vel = np.array([[[2.0, 0.0], [0.0, 0.0], [0.0, 0.0]]])
    acc = np.array([[[-4.0, 0.0], [0.0, 0.0], [0.0, 0.0]]])
    st = cr.check_corridor(2, 1.0, [0.0, 0.0], 0.5, cells, pos, vel, acc, 0.0)
    # segment 0: x peaks at t* = 0.5 with 2.0 (inside by 1), ends at 1.5; y constant 1.5 -> excess = max(-0.5, ...) = -0.5
    # segment 2: exactly on the faces x = 1 and y = 2 -> excess 0, not outside
    assert st["max_excess"][0] == 0.0 and st["segment"][0] == 2 and st["n_blocked"][0] == 1 and st["n_outside"][0] == 0
    assert cr.segment_excess(2, 1.0, [1.0, 1.0], [3.0, 2.0], pos[0, 0], vel[0, 0], acc[0, 0]) == -0.5
    acc[0, 0, 0] = -1.0  # the interior extremum moves past h: the end value 1.5 + 2 - 0.5 = 3.0 is on the face
    assert cr.segment_excess(2, 1.0, [1.0, 1.0], [3.0, 2.0], pos[0, 0], vel[0, 0], acc[0, 0]) == 0.0
    vel[0, 0, 0], acc[0, 0, 0] = 4.0, -8.0  # t* = 0.5, peak 1.5 + 2 - 1 = 2.5 ... and back to 1.5: only the peak shows it
    pos[0, 0, 0] = 2.0
    assert cr.segment_excess(2, 1.0, [1.0, 1.0], [3.0, 2.0], pos[0, 0], vel[0, 0], acc[0, 0]) == 0.0
    pos[0, 0, 0] = 2.25
    st = cr.check_corridor(2, 1.0, [0.0, 0.0], 0.5, cells, pos, vel, acc, 0.0)
    assert st["max_excess"][0] == 0.25 and st["segment"][0] == 0 and st["n_outside"][0] == 1
    none = cr.check_corridor(2, 1.0, [0.0, 0.0], 0.5, cells[:, 1:2], pos[:, 1:2], vel[:, 1:2], acc[:, 1:2], 0.0)
    assert none["max_excess"][0] == -np.inf and none["segment"][0] == cr.NO_SEGMENT and none["n_blocked"][0] == 1


@pytest.mark.parametrize("D", [2, 3])
def test_rasterize_is_conservative(D):
    from path_planning.scenarios.obstacles import rasterize

    rng = np.random.default_rng(2)
    space = [0.0, -1.0, 6.0, 4.0] if D == 2 else [0.0, -1.0, 0.5, 6.0, 4.0, 3.0]
    disc = [2.3, 1.1, 0.9] if D == 2 else [2.3, 1.1, 1.6, 0.9]
    box = [4.0, 0.2, 5.1, 1.3] if D == 2 else [4.0, 0.2, 1.0, 5.1, 1.3, 2.2]
    margin, cell = 0.2, 0.3
    occ, origin, cell = rasterize(space, cell, discs=[disc], boxes=[box], margin=margin)
    assert occ.dtype == np.uint8 and occ.ndim == 3 and (D == 3 or occ.shape[0] == 1)
    pts = rng.uniform(space[:D], space[D:], size=(40_000, D))
    d_disc = np.linalg.norm(pts - disc[:D], axis=1) - disc[D]
    d_box = np.linalg.norm(np.maximum(np.maximum(np.array(box[:D]) - pts, pts - np.array(box[D:])), 0.0), axis=1)
    near = (d_disc < margin) | (d_box < margin)
    assert near.sum() > 1000
    idx = np.minimum(np.floor((pts - origin) / cell).astype(int), np.array(occ.shape[::-1][:D]) - 1)
    hit = occ[idx[:, 2] if D == 3 else 0, idx[:, 1], idx[:, 0]] != 0
    assert hit[near].all()  # a point closer than the margin to an obstacle lies in an occupied cell
    far = (d_disc > margin + cell * np.sqrt(D)) & (d_box > margin + cell * np.sqrt(D))
    assert not hit[far].any()  # ... and the grid is not occupied a cell diagonal beyond


def test_rasterize_and_host_api_errors():
    from path_planning.scenarios.obstacles import rasterize
    from path_planning.solvers.scp import check_position_boxes, corridor_shrink, straight_reference

    for bad in (dict(cell=0.0), dict(cell=np.inf), dict(cell=1e-4), dict(cell=0.5, margin=-1.0), dict(cell=0.5, discs=[(1, 2)]),
                dict(cell=0.5, boxes=[(3, 3, 1, 1)])):
        with pytest.raises(ValueError):
            rasterize([0, 0, 10, 10], **bad)
    with pytest.raises(ValueError):
        rasterize([0, 0, 10], 0.5)
    N, K, D = 2, 5, 2
    lo, hi = np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)
    a, b = check_position_boxes(N, K, D, [0, 0], [10, 10], lo, hi)
    assert a.shape == (N, K, D) and a.flags.c_contiguous
    lo[1, 3, 0], hi[1, 3, 0] = 4.0, 3.0
    with pytest.raises(ValueError, match="vehicle 1, state 3, coordinate 0"):
        check_position_boxes(N, K, D, [0, 0], [10, 10], lo, hi)
    lo[1, 3, 0], hi[1, 3, 0] = 11.0, 12.0  # not empty by itself, empty inside the workspace
    with pytest.raises(ValueError, match="state 3"):
        check_position_boxes(N, K, D, [0, 0], [10, 10], lo, hi)
    lo[1, 3, 0], hi[1, 3, 0] = -np.inf, np.inf
    lo[0, 0, 0], hi[0, 0, 0] = 5.0, 4.0  # state 0 is never constrained
    check_position_boxes(N, K, D, [0, 0], [10, 10], lo, hi)
    with pytest.raises(ValueError, match="shape"):
        check_position_boxes(N, K, D, [0, 0], [10, 10], lo[:, :-1], hi[:, :-1])
    lo[0, 1, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        check_position_boxes(N, K, D, [0, 0], [10, 10], lo, hi)
    with pytest.raises(ValueError):
        corridor_shrink(-15.0, 15.0, 0.2, -0.01)
    assert corridor_shrink(-15.0, 10.0, 0.2, 0.02) == 15.0 * 0.2 * 0.2 / 8.0 + 0.02
    ref = straight_reference([[0.0, 0.0]], [[4.0, 2.0]], 4)
    np.testing.assert_array_equal(ref[0], [[0, 0], [1, 0.5], [2, 1], [3, 1.5], [4, 2]])


def test_struct_layouts_match_the_header(tmp_path):
    from path_planning import _hip

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu ", sizeof(scp_occupancy_grid), offsetof(scp_occupancy_grid, origin), '
                   'offsetof(scp_occupancy_grid, cell), offsetof(scp_occupancy_grid, dims), offsetof(scp_occupancy_grid, reserved));\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(scp_corridor_stats), offsetof(scp_corridor_stats, max_excess), '
                   'offsetof(scp_corridor_stats, segment), offsetof(scp_corridor_stats, n_blocked), '
                   'offsetof(scp_corridor_stats, n_outside), offsetof(scp_corridor_stats, reserved));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G, S = _hip.OccupancyGrid, _hip.CorridorStats
    assert got[:5] == [ctypes.sizeof(G), G.origin.offset, G.cell.offset, G.dims.offset, G.reserved.offset] == [48, 0, 24, 32, 44]
    names = ["max_excess", "segment", "n_blocked", "n_outside", "reserved"]
    assert got[5:] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] == [32, 0, 8, 12, 16, 24]
    assert _hip.CORRIDOR_STATS_DTYPE == cr.CORRIDOR_STATS_DTYPE and _hip.CORRIDOR_STATS_DTYPE.itemsize == 32
    assert [_hip.CORRIDOR_STATS_DTYPE.fields[f][1] for f in names] == got[6:]


def test_python_surface():
    import inspect

    from path_planning import _hip
    from path_planning.cli import compute_trajectories
    from path_planning.solvers.scp import SCP

    for name in ("set_obstacles", "set_corridors", "set_position_boxes", "validate_corridor"):
        assert callable(getattr(SCP, name))
    sig = inspect.signature(SCP.set_corridors)
    assert [sig.parameters[k].default for k in ("reference", "max_grow", "pad", "allow_open")] == [None, 8, 0.02, False]
    for name in ("scp_occupancy_prepare", "scp_corridor_boxes", "scp_corridor_state_boxes", "scp_qp_set_position_boxes",
                 "scp_solver_set_position_boxes", "scp_check_corridor"):
        assert name in _hip.EXPORTS
    assert "set_position_boxes" in dir(_hip.QP) and "set_position_boxes" in dir(_hip.NativeSolver)
    args = compute_trajectories.build_parser().parse_args(["--obstacle-discs", "5,5,1", "4,2,0.5", "--corridor-cell", "0.25",
                                                           "--corridor-grow", "6"])
    assert args.obstacle_discs == ["5,5,1", "4,2,0.5"] and args.corridor_cell == 0.25 and args.corridor_grow == 6
    assert compute_trajectories.build_parser().parse_args([]).obstacle_discs is None


def test_end_to_end_scene_has_corridors():
    """the scene of the GPU end-to-end test: no blocked segment, no open state, boxes inside the workspace"""
    from path_planning.solvers.scp import check_position_boxes, corridor_shrink

    E = cc.EndToEnd
    occ, origin, cell = E.grid()
    assert occ.shape == (1, 40, 40) and 30 < occ.sum() < 200
    cells, n_blocked = cr.corridor_boxes(E.D, origin, cell, cr.summed_table(occ), E.reference(), E.max_grow)
    lo, hi, n_open = cr.state_boxes(E.D, origin, cell, cells, corridor_shrink(-15.0, 15.0, E.h, E.pad))
    assert n_blocked == 0 and n_open == 0
    check_position_boxes(E.N, E.K, E.D, E.space[:2], E.space[2:], lo, hi)
    # the straight line of vehicle 0 goes through the disc: its corridor is blocked there
    from path_planning.solvers.scp import straight_reference

    _, blocked_straight = cr.corridor_boxes(E.D, origin, cell, cr.summed_table(occ), straight_reference(E.p0, E.pf, E.K), E.max_grow)
    assert blocked_straight > 0
