"""The shape rasteriser on the GPU: scp_rasterize_shapes against tests/rasterize_ref.py on every map of
tests/rasterize_cases.py (array_equal), at two sizes of its work items, its argument errors, and one fleet planned end to end
around an oblique wall and a building given as shapes -- through the planner and through the command line."""
import ctypes

import numpy as np
import pytest

import rasterize_cases as rc

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rc.all_cases()}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _rasterize(ctx, c):
    from path_planning import _hip
    from path_planning.scenarios.obstacles import pack_shapes

    grid = _hip.occupancy_grid(c.D, c.origin, c.cell, c.dims)
    occ = ctx.rasterize_shapes(c.D, grid, pack_shapes(c.D, **c.shapes()), c.margin)
    assert occ.dtype.itemsize == 1 and tuple(occ.shape) == c.want().shape
    return occ.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_device_grid_equals_the_reference(ctx, name):
    c = CASES[name]
    got = _rasterize(ctx, c)
    assert ctx.last_pair_ms() >= 0.0
    assert set(np.unique(got).tolist()) <= {0, 1}
    np.testing.assert_array_equal(got, c.want())
    if c.n_shapes == 0 or name.endswith("_outside"):
        assert not got.any()
    # the call clears the grid itself: a second call into new memory, after a different map, gives the same grid
    _rasterize(ctx, CASES["65x3_mixed_m0.4"])
    np.testing.assert_array_equal(_rasterize(ctx, c), got)


@pytest.mark.parametrize("name", rc.MIXED)
def test_the_size_of_a_work_item_does_not_matter(ctx, name):
    """64 cells per item cuts the polygon over 256 x 256 cells into 1024 items and most shapes of the small maps into
    several; 2^24 makes every shape one item whose workgroup loops over all of its cells"""
    c = CASES[name]
    try:
        for cells in (64, 1 << 24):
            ctx.set_option("raster_item_cells", cells)
            np.testing.assert_array_equal(_rasterize(ctx, c), c.want(), err_msg=f"raster_item_cells={cells}")
    finally:
        ctx.set_option("raster_item_cells", 0)
    from path_planning import _hip

    for bad in (1, 63, (1 << 24) + 1, -5):
        with pytest.raises(_hip.HipError):
            ctx.set_option("raster_item_cells", bad)


def test_invalid_records_are_rejected_with_a_message(ctx):
    import torch

    from path_planning import _hip

    grid = _hip.occupancy_grid(2, [0.0, 0.0], 0.5, (8, 8))
    grid3 = _hip.occupancy_grid(3, [0.0, 0.0, 0.0], 0.5, (4, 4, 4))
    occ = torch.full((1, 8, 8), 7, dtype=torch.uint8, device=ctx.tdev)
    tri = np.array([[1.0, 1.0], [3.0, 1.0], [1.0, 3.0]])
    nan, inf = float("nan"), float("inf")

    def call(D, g, records, vertices=tri, margin=0.25, n_shapes=None, n_vertices=None):
        rec = np.zeros(len(records), dtype=_hip.OBSTACLE_SHAPE_DTYPE)
        for i, (kind, first, n, p) in enumerate(records):
            rec["kind"][i], rec["first_vertex"][i], rec["n_vertices"][i] = kind, first, n
            rec["p"][i][:len(p)] = p
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        return ctx.lib.scp_rasterize_shapes(ctx.h, D, ctypes.byref(g), len(rec) if n_shapes is None else n_shapes,
                                            rec.ctypes.data_as(ctypes.POINTER(_hip.ObstacleShape)),
                                            len(v) if n_vertices is None else n_vertices, v.ctypes.data_as(_hip.pd), margin,
                                            occ.data_ptr())

    good = [(0, 0, 0, [2.0, 2.0, 0, 0, 0, 0, 0.5]), (3, 0, 3, [])]
    bad = [
        dict(records=[(4, 0, 0, [])]), dict(records=[(-1, 0, 0, [])]),
        dict(records=[(0, 0, 0, [nan, 2.0, 0, 0, 0, 0, 0.5])]), dict(records=[(0, 0, 0, [2.0, 2.0, 0, 0, 0, 0, inf])]),
        dict(records=[(0, 0, 0, [2.0, 2.0, 0, 0, 0, 0, -0.5])]),
        dict(records=[(1, 0, 0, [2.0, 2.0, 0, 1.0, 3.0, 0])]), dict(records=[(1, 0, 0, [2.0, nan, 0, 3.0, 3.0, 0])]),
        dict(records=[(2, 0, 0, [1.0, 1.0, 0, 2.0, 2.0, 0, -1e-9])]), dict(records=[(2, 0, 0, [1.0, 1.0, 0, inf, 2.0, 0, 0.1])]),
        dict(records=[(3, 0, 2, [])]), dict(records=[(3, 0, 4097, [])]), dict(records=[(3, 1, 3, [])]), dict(records=[(3, -1, 3, [])]),
        dict(records=[(3, 0, 3, [])], vertices=np.array([[1.0, 1.0], [nan, 1.0], [1.0, 3.0]])),
        dict(records=good, margin=-0.1), dict(records=good, margin=nan), dict(records=good, margin=inf),
        dict(records=good, n_shapes=-1), dict(records=good, n_shapes=65537), dict(records=good, n_vertices=-1),
        dict(records=good, n_vertices=(1 << 20) + 1),
        dict(D=3, g=grid3, records=[(3, 0, 3, [1.0, 0.5])]), dict(D=3, g=grid3, records=[(3, 0, 3, [nan, 0.5])]),
        dict(D=4, records=good), dict(g=_hip.occupancy_grid(2, [0.0, 0.0], 0.0, (8, 8)), records=good),
    ]
    # nothing is enqueued by a call that fails its checks: the grid keeps the 7s it was filled with
    for kw in bad:
        kw = dict({"D": 2, "g": grid}, **kw)
        assert call(**kw) == -1, kw  # SCP_ERR_INVALID
        assert b"rasterize_shapes" in ctx.lib.scp_last_error(ctx.h), kw
    assert call(2, grid, [(3, 0, 4097, [])]) == -1 and b"4096" in ctx.lib.scp_last_error(ctx.h)
    assert (occ.cpu().numpy() == 7).all()
    assert call(2, grid, good) == 0
    got = occ.cpu().numpy()
    assert set(np.unique(got).tolist()) == {0, 1} and got[0, 4, 4] == 1 and got[0, 7, 7] == 0
    # fields a kind does not read are ignored: a sphere with NaN in the slots of a second point
    assert call(2, grid, [(0, -5, 9999, [2.0, 2.0, nan, nan, nan, nan, 0.5])]) == 0
    with pytest.raises(ValueError):
        from path_planning.scenarios.obstacles import pack_shapes

        ctx.rasterize_shapes(2, grid, pack_shapes(2, discs=[(1.0, 1.0, -1.0)]), 0.25)


class Scene:
    """D = 2, space 10 x 10, T = 8, h = 0.4 (K = 20), R = 0.5, cell 0.2; eight vehicles fly from x = 1.5 to x = 8.5.  An
    oblique wall of two capsules runs from (4.6, 0) to (5.0, 3.0) and from (5.4, 7.0) to (5.8, 10): the gap 3 < y < 7 lies
    between starts and goals, and the outer vehicles' straight lines hit the wall.  A building (a four-sided polygon) stands
    below the lowest goal line.  Why every vehicle can be expected to keep a clearance > 0 although the outer ones fly round
    the wall's ends as tightly as their boxes allow: a state lies at least the shrink 15 h^2 / 8 + 0.02 = 0.32 m inside a box
    of free cells, which is more than one cell of 0.2 m, so a whole free cell lies between the state's cell and any occupied
    one; the 0.12 m to spare cover the sag a h^2 / 8 of a segment between its states up to a = 6 m/s^2.  Measured on an MI355X:
    224 of 2500 cells occupied, largest corridor excess -0.312 m, clearances 0.4, 0.2, 0.63, 1.2, 1.2, 0.6, 0.2, 0.2 m (the
    vehicles that fly round the wall's ends keep exactly the one cell), no touching piece."""
    N, D, T, h, R, K = 8, 2, 8.0, 0.4, 0.5, 20
    space = [0.0, 0.0, 10.0, 10.0]
    cell = 0.2
    capsules = [(4.6, 0.0, 5.0, 3.0, 0.1), (5.4, 7.0, 5.8, 10.0, 0.1)]
    building = np.array([[6.8, 0.2], [8.2, 0.3], [8.0, 1.1], [7.0, 1.0]])
    ys = np.array([2.2, 3.0, 3.8, 4.6, 5.4, 6.2, 7.0, 7.8])
    p0 = np.stack([np.full(8, 1.5), ys], axis=1)
    pf = np.stack([np.full(8, 8.5), ys], axis=1)


def test_end_to_end_around_an_oblique_wall_and_a_building():
    from path_planning.scenarios.obstacles import grid_shape
    from path_planning.solvers.scp import SCP

    import rasterize_ref as rr

    S = Scene
    s = SCP(n_vehicles=S.N, time_horizon=S.T, time_step=S.h, min_distance=S.R, space_dims=S.space, verbose=False)
    assert s.K == S.K and s.obstacle_info is None
    s.set_initial_states(S.p0)
    s.set_final_states(S.pf)
    oi = s.set_obstacle_shapes(S.cell, capsules=S.capsules, polygons=[(S.building,)])
    origin, dims = grid_shape(S.space, S.cell)
    want = rr.rasterize_shapes(S.D, origin, S.cell, dims, capsules=S.capsules, polygons=[(S.building,)], margin=S.R / 2)
    np.testing.assert_array_equal(s._obstacles.occ.cpu().numpy(), want)
    assert oi is s.obstacle_info and oi["n_shapes"] == 3 and oi["counts"] == {"discs": 0, "boxes": 0, "capsules": 2, "polygons": 1}
    assert oi["dims"] == (50, 50) and oi["n_cells"] == 2500 and oi["n_occupied"] == int(want.sum()) and oi["margin"] == S.R / 2
    assert oi["rasterize_ms"] >= 0.0 and oi["prepare_ms"] >= 0.0
    with pytest.raises(ValueError, match="blocked"):  # the wall stands between starts and goals
        s.set_corridors()
    info = s.set_corridors(reference="search")
    assert info["n_blocked"] == 0 and info["n_open"] == 0 and s.last_info["reference"]["n_failed"] == 0
    s.generate_trajectories(max_iterations=15)
    co = s.validate_corridor()
    oc = s.obstacle_clearance()
    print(f"shapes end to end: {oi['n_occupied']} of {oi['n_cells']} cells occupied, rasterised in {oi['rasterize_ms']:.3f} ms; corridor "
          f"max_excess {co['max_excess']:.4e}; clearance per vehicle {oc['vehicles']['clearance'].tolist()}, n_touch {oc['n_touch']}")
    assert co["inside"] and co["n_outside"] == 0 and co["n_blocked"] == 0 and co["max_excess"] <= 0.0
    assert (oc["vehicles"]["clearance"] > 0.0).all() and oc["n_touch"] == 0 and (oc["vehicles"]["n_touch"] == 0).all()
    # a new map by the host's way drops what the device rasteriser reported
    s.set_obstacles(want, origin, S.cell)
    assert s.obstacle_info is None and s._corridor is None and s._boxes is None
    s.close()


def test_the_command_line_plans_the_same_scene(capsys):
    from path_planning.cli import compute_trajectories as ct

    # The command line has no flag for start and goal positions, so it cannot fly Scene's fleet: this is the fleet of the
    # other command-line tests (four vehicles in 20 x 20, K = 20, seed 1) with the same kinds of shape -- an oblique capsule
    # wall across the straight line of vehicle 0, (14.2, 2.4) -> (12.1, 12.2), and a polygon building away from every line.
    solver = ct.main(["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--min-distance", "0.8", "--space", "0", "0",
                      "20", "20", "--seed", "1", "--no-plots", "--corridor-search", "--obstacle-clearance",
                      "--obstacle-capsules", "12.9,6.9,13.9,7.5,0.1", "--obstacle-polygons", "5,2,7,2.5,6,4"])
    out = capsys.readouterr().out
    print(out)
    line = [ln for ln in out.splitlines() if ln.startswith("Obstacles: ")]
    assert len(line) == 1 and line[0].startswith("Obstacles: 2 shapes (1 capsules, 1 polygons) rasterised on the GPU with margin 0.4 m: ")
    assert solver is not None and solver.obstacle_info["n_shapes"] == 2 and solver.obstacle_info["n_occupied"] > 0
    assert "4 of 4 paths found" in out and "Corridors: 2 obstacles on a grid of 100 x 100 x 1 cells of 0.2 m" in out
    assert "every segment stays inside its box" in out and solver.validate_corridor()["inside"]
    assert "Obstacle clearance: at least " in out and "0 pieces touch an occupied cell" in out
