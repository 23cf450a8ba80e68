"""Reference paths by a lattice search on the GPU: scp_lattice_edges and scp_reference_paths against
tests/reference_path_ref.py (integers exactly, the reference points bit for bit), the argument checks, and an end-to-end
solve through a wall with one gap."""
import numpy as np
import pytest

import corridor_ref as cr
import reference_path_cases as rc

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rc.all_cases()}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _grid(c):
    from path_planning import _hip

    return _hip.occupancy_grid(c.D, c.origin, c.cell, c.occ.shape[::-1])


def _run(ctx, c, ref_in, want_path=True, want_dist=True):
    """edges and one search of a case: numpy copies of everything the two calls write"""
    from path_planning import _hip

    g = _grid(c)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    ref = ctx.tensor(ref_in)
    path, info, dist, n_failed = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, ctx.tensor(c.p0), ctx.tensor(c.pf),
                                                     c.max_path, ref, want_path=want_path, want_dist=want_dist)
    return {"edges": edges.cpu().numpy().view(np.uint32), "ref": ref.cpu().numpy(),
            "path": path.cpu().numpy() if want_path else None, "info": info.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:c.N].copy(),
            "dist": dist.cpu().numpy().view(np.uint16) if want_dist else None, "n_failed": int(n_failed.item())}


def _assert_equal(got, want, keys=("edges", "info", "path", "dist", "ref", "n_failed")):
    for k in keys:
        if k == "ref":
            np.testing.assert_array_equal(got[k].view(np.uint64), want[k].view(np.uint64), err_msg=k)
        elif k == "n_failed":
            assert got[k] == want[k]
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_restatement(ctx, name):
    c = CASES[name]
    want = c.want()
    got = _run(ctx, c, c.ref_in())
    _assert_equal(got, want)
    # a second call with the same inputs: the same bytes
    again = _run(ctx, c, c.ref_in())
    _assert_equal(again, got)
    # a failed vehicle's rows of ref keep the bytes they were given, whatever they are
    marked = np.full((c.N, c.K + 1, c.D), -123.456)
    marked.view(np.uint64)[...] ^= np.arange(marked.size, dtype=np.uint64).reshape(marked.shape)
    got = _run(ctx, c, marked, want_path=False, want_dist=False)  # (and without the optional outputs)
    failed = want["info"]["status"] != 0
    np.testing.assert_array_equal(got["ref"][failed].view(np.uint64), marked[failed].view(np.uint64))
    np.testing.assert_array_equal(got["ref"][~failed].view(np.uint64), want["ref"][~failed].view(np.uint64))
    _assert_equal(got, want, keys=("info", "n_failed"))


@pytest.mark.parametrize("name", ["rand2d_50x37_s1_c0", "rand3d_16_s1_c1", "serpentine", "many_vehicles", "status_1_2"])
def test_workgroup_size_does_not_matter(ctx, name):
    c = CASES[name]
    try:
        for threads in (256, 512, 1024):
            ctx.set_option("ref_path_threads", threads)
            _assert_equal(_run(ctx, c, c.ref_in()), c.want())
    finally:
        ctx.set_option("ref_path_threads", 0)


def test_argument_checks(ctx):
    from path_planning import _hip

    c = CASES["rand2d_13x11_s2_c1"]
    g = _grid(c)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    for stride, clearance in ((0, 0), (-1, 0), (12, 0), (1, -1)):  # (12 > ny = 11: L_y = 0)
        with pytest.raises(_hip.HipError):
            ctx.lattice_edges(c.D, g, sat, stride, clearance)
    big = np.zeros((1, 129, 256), dtype=np.uint8)  # 33 024 nodes at stride 1
    gb = _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (256, 129))
    _, sat_big = ctx.occupancy_prepare(2, gb, big)
    with pytest.raises(_hip.HipError, match="nodes"):
        ctx.lattice_edges(2, gb, sat_big, 1, 0)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    p0, pf, ref = ctx.tensor(c.p0), ctx.tensor(c.pf), ctx.tensor(c.ref_in())
    for N, K, stride, max_path in ((0, c.K, c.stride, 5), (c.N, 0, c.stride, 5), (c.N, c.K, 0, 5), (c.N, c.K, c.stride, 0),
                                   (c.N, c.K, c.stride, c.nodes + 1)):
        with pytest.raises(_hip.HipError):
            ctx.reference_paths(N, K, c.D, g, stride, edges, p0, pf, max_path, ref)
    with pytest.raises(_hip.HipError):
        ctx.set_option("ref_path_threads", 128)
    # a clearance beyond the grid is the clearance of the whole grid
    huge = ctx.lattice_edges(c.D, g, sat, c.stride, 2**31 - 1).cpu().numpy()
    np.testing.assert_array_equal(huge, ctx.lattice_edges(c.D, g, sat, c.stride, 13).cpu().numpy())


def test_find_reference_api(ctx):
    from path_planning.solvers.scp import SCP

    W = rc.WallScene
    occ, origin, cell = W.grid()
    s = SCP(n_vehicles=W.N, time_horizon=W.T, time_step=W.h, min_distance=W.R, space_dims=W.space, verbose=False)
    s.set_initial_states(W.p0)
    with pytest.raises(ValueError, match="set_obstacles"):
        s.find_reference()
    s.set_obstacles(occ, origin, cell)
    with pytest.raises(ValueError, match="set_final_states"):
        s.find_reference()
    s.set_final_states(W.pf)
    ref, info = s.find_reference()
    want = CASES["wall_scene"].want()
    np.testing.assert_array_equal(ref.view(np.uint64), want["ref"].view(np.uint64))
    assert info is s.last_info["reference"] and info["n_failed"] == 0 and info["stride"] == 2 and info["clearance"] == 0
    assert info["lattice"] == (20, 20) and info["max_edges"] == int(want["info"]["n_nodes"].max()) + 1 and info["guaranteed"]
    np.testing.assert_array_equal(info["status"], want["info"]["status"])
    np.testing.assert_array_equal(info["n_nodes"], want["info"]["n_nodes"])
    assert info["edges_ms"] > 0 and info["search_ms"] > 0
    assert s.find_reference()[1]["edges_ms"] == 0.0 and list(s._obstacles.edge_masks) == [(2, 0)]  # the masks are cached
    for bad in (dict(stride=0), dict(stride=2.0), dict(clearance=-1), dict(max_path=0), dict(max_path=401), dict(stride=41)):
        with pytest.raises(ValueError):
            s.find_reference(**bad)
    # a clearance that closes the gap (8 cells wide): nobody crosses
    with pytest.raises(ValueError, match="vehicle 0 .*cannot be reached"):
        s.find_reference(stride=1, clearance=4)
    ref, info = s.find_reference(stride=1, clearance=4, allow_unreachable=True)
    assert info["status"].tolist() == [3, 3, 3] and info["n_failed"] == 3 and info["max_edges"] == 0 and info["guaranteed"]
    from path_planning.solvers.scp import straight_reference

    np.testing.assert_array_equal(ref, straight_reference(W.p0, W.pf, W.K))
    # other strides and clearances against the restatement; a short horizon makes E > K, which only clearance makes up for
    for stride, clearance in ((1, 0), (1, 3), (3, 0)):
        ref, info = s.find_reference(stride=stride, clearance=clearance, max_path=100)
        want = rc.Case("x", W.D, occ, origin, cell, stride, clearance, W.K, W.p0, W.pf, max_path=100).want()
        np.testing.assert_array_equal(ref.view(np.uint64), want["ref"].view(np.uint64))
        assert info["max_edges"] == int(want["info"]["n_nodes"].max()) + 1 <= W.K and info["guaranteed"]
    short = SCP(n_vehicles=W.N, time_horizon=4.0, time_step=W.h, min_distance=W.R, space_dims=W.space, verbose=False)
    assert short.K == 20
    short.set_initial_states(W.p0)
    short.set_final_states(W.pf)
    short.set_obstacles(occ, origin, cell)
    assert [short.find_reference(stride=1, clearance=c)[1]["guaranteed"] for c in (0, 1, 3)] == [False, True, True]  # E = 34 .. 39
    assert short.find_reference()[1]["stride"] == 3  # 40 / 3 <= 18
    short.close()
    s.set_obstacles(occ, origin, cell)
    assert not s._obstacles.edge_masks  # a new map drops the cached masks
    s.close()


def test_pool_skips_a_destroyed_context(ctx):
    """An SCP object collected in one cycle with its context pools the context, whose own finaliser then destroys it: the
    next object of that shape must not take it."""
    from path_planning.solvers import scp as scp_mod

    kw = dict(n_vehicles=2, time_horizon=6.0, time_step=0.5, min_distance=0.7, space_dims=[0, 0, 9, 9], device=0, verbose=False)
    p0, pf = np.array([[2.0, 4.0], [6.0, 4.5]]), np.array([[6.0, 4.0], [2.0, 4.5]])  # (4 m in 6 s: well inside the limits)
    first = scp_mod.SCP(**kw)
    first.set_initial_states(p0)
    first.set_final_states(pf)
    first.generate_trajectories(max_iterations=3)
    key, dead = first._pool_key, first._ctx
    first.close()
    assert any(c is dead for c, _ in scp_mod._POOL.get(key, []))  # pooled ...
    dead.close()                                                  # ... and destroyed, as its finaliser would
    second = scp_mod.SCP(**kw)
    assert second._ctx is not dead and second._ctx.h
    second.set_initial_states(p0)
    second.set_final_states(pf)
    second.generate_trajectories(max_iterations=3)
    assert not any(c is dead for c, _ in scp_mod._POOL.get(key, []))
    second.close()


@pytest.mark.parametrize("native", [True, False])
def test_end_to_end_through_the_gap(ctx, native):
    """Three vehicles and a wall with one gap: the straight lines are blocked; with the searched reference every segment stays
    inside its box and the separation checks pass (the expectations and tolerances of test_corridor_gpu's end-to-end test).
    The three meet at the gap, so the SCP loop runs joint QPs with collision rows next to the boxes."""
    from path_planning.solvers.scp import SCP

    W = rc.WallScene
    occ, origin, cell = W.grid()
    s = SCP(n_vehicles=W.N, time_horizon=W.T, time_step=W.h, min_distance=W.R, space_dims=W.space, native=native, verbose=False)
    assert s.K == W.K
    s.set_initial_states(W.p0)
    s.set_final_states(W.pf)
    s.set_obstacles(occ, origin, cell)
    with pytest.raises(ValueError, match="blocked"):
        s.set_corridors()
    info = s.set_corridors(reference="search", max_grow=W.max_grow, pad=W.pad)
    assert info["n_blocked"] == 0 and info["n_open"] == 0
    assert s.last_info["reference"]["n_failed"] == 0 and s.last_info["reference"]["guaranteed"]
    traj = s.generate_trajectories(max_iterations=15)
    statuses = [s.last_info["qp0"]["status_val"]] + [it["status_val"] for it in s.last_info["iterations"]]
    assert set(statuses) <= {1, 2}, statuses
    pipes = {p for it in s.last_info["iterations"] for p in it["pipeline"].split("+")}
    assert len(statuses) > 1 and not pipes & {"persistent16", "persistent8-lean"}, pipes
    rep = s.validate_solution(continuous=True)
    co = rep["corridor"]
    print(f"native={native}: {len(statuses) - 1} SCP iterations, corridor max_excess {co['max_excess']:.4e}, n_outside {co['n_outside']}, min distance "
          f"{rep['min_pair_distance']:.4f} / continuous {rep['min_pair_distance_continuous']:.4f}, pipelines {sorted(pipes)}")
    assert co["inside"] and co["n_outside"] == 0 and co["n_blocked"] == 0 and co["max_excess"] <= 0.0
    assert rep["collision_free"] and rep["collision_free_continuous"]
    out = s.validate_corridor()
    assert out["inside"] and out["n_outside"] == 0
    # every sample keeps the body (radius R / 2) off the wall: it lies in a free cell of the grid rasterised with that margin
    idx = np.floor((traj["positions"] - origin) / cell).astype(int)
    assert (occ[0, idx[..., 1], idx[..., 0]] == 0).all()
    want = cr.check_corridor(W.D, W.h, origin, cell, s._corridor["cells"].cpu().numpy(), traj["positions"], traj["velocities"],
                             traj["accelerations"], 0.0)
    np.testing.assert_array_equal(co["vehicles"]["max_excess"].view(np.uint64), want["max_excess"].view(np.uint64))
    s.close()
