"""Shortened reference paths on the GPU: scp_shorten_paths against tests/shorten_ref.py (the kept lists and the records in
every integer, lengths and reference points bit for bit), per workgroup size, the argument checks, SCP.shorten_reference and
an end-to-end solve through a wall with one gap."""
import numpy as np
import pytest

import corridor_ref as cr
import reference_path_cases as rc
import shorten_cases as sc
import shorten_ref as sr

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sc.all_cases()}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _grid(c):
    from path_planning import _hip

    return _hip.occupancy_grid(c.D, c.origin, c.cell, c.occ.shape[::-1])


def _run(ctx, c, ref_in, want_kept=True):
    """the search and the shortening of a case: numpy copies of what scp_shorten_paths writes.  ref_in: the rows the search
    starts from (those of the vehicles without a path must come back as they are)"""
    from path_planning import _hip

    g = _grid(c)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    ref = ctx.tensor(ref_in)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    path, info, _, _ = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref)
    np.testing.assert_array_equal(path.cpu().numpy(), c.want()["path"])
    kept, out = ctx.shorten_paths(c.N, c.K, c.D, g, sat, c.stride, c.clearance, p0, pf, c.max_path, path, info, ref,
                                  want_kept=want_kept)
    return {"ref": ref.cpu().numpy(), "kept": kept.cpu().numpy() if want_kept else None,
            "out": out.cpu().numpy().view(_hip.SHORTEN_INFO_DTYPE)[:c.N].copy()}


def _assert_equal(got, want, keys=("kept", "out", "ref")):
    for k in keys:
        if k == "ref":
            np.testing.assert_array_equal(got[k].view(np.uint64), want[k].view(np.uint64), err_msg=k)
        elif k == "out":
            for f in ("n_kept", "n_vertices"):
                np.testing.assert_array_equal(got[k][f], want[k][f], err_msg=f)
            for f in ("length", "length_before"):
                np.testing.assert_array_equal(got[k][f].view(np.uint64), want[k][f].view(np.uint64), err_msg=f)
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_restatement(ctx, name):
    c = CASES[name]
    want = sc.want(c)
    got = _run(ctx, c, c.ref_in())
    _assert_equal(got, want)
    # a vehicle without a path keeps the bytes of its rows, whatever they are; without `kept` the same points and records
    marked = np.full((c.N, c.K + 1, c.D), -123.456)
    marked.view(np.uint64)[...] ^= np.arange(marked.size, dtype=np.uint64).reshape(marked.shape)
    got = _run(ctx, c, marked, want_kept=False)
    failed = c.want()["info"]["status"] != 0
    np.testing.assert_array_equal(got["ref"][failed].view(np.uint64), marked[failed].view(np.uint64))
    np.testing.assert_array_equal(got["ref"][~failed].view(np.uint64), want["ref"][~failed].view(np.uint64))
    _assert_equal(got, want, keys=("out",))


@pytest.mark.parametrize("name", ["rand2d_50x37_s1_c0", "rand3d_16_s1_c1", "serpentine", "many_vehicles", "open_40x30"])
def test_workgroup_size_does_not_matter(ctx, name):
    c = CASES[name]
    try:
        for threads in (64, 128, 256):
            ctx.set_option("shorten_threads", threads)
            _assert_equal(_run(ctx, c, c.ref_in()), sc.want(c))
    finally:
        ctx.set_option("shorten_threads", 0)


def test_argument_checks(ctx):
    from path_planning import _hip

    c = CASES["rand2d_13x11_s2_c1"]
    g = _grid(c)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    p0, pf, ref = ctx.tensor(c.p0), ctx.tensor(c.pf), ctx.tensor(c.ref_in())
    path, info, _, _ = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref)
    good = dict(N=c.N, K=c.K, stride=c.stride, clearance=c.clearance, max_path=c.max_path, path=path, info=info)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.shorten_paths(a["N"], a["K"], c.D, g, sat, a["stride"], a["clearance"], p0, pf, a["max_path"], a["path"],
                                 a["info"], ref)

    for bad in (dict(N=0), dict(K=0), dict(stride=0), dict(stride=-1), dict(stride=12), dict(clearance=-1), dict(max_path=0),
                dict(max_path=c.nodes + 1)):
        with pytest.raises(_hip.HipError):
            call(**bad)
    for bad in (dict(path=None), dict(info=None)):
        with pytest.raises(_hip.HipError, match="null pointer"):
            call(**bad)
    for threads in (32, 512, -64):
        with pytest.raises(_hip.HipError):
            ctx.set_option("shorten_threads", threads)
    # a clearance beyond the grid is the clearance of the whole grid (the lattice path was made with c.clearance: where
    # nothing is seen, the next node is taken)
    huge = call(clearance=2**31 - 1)
    whole = call(clearance=13)
    np.testing.assert_array_equal(huge[0].cpu().numpy(), whole[0].cpu().numpy())
    np.testing.assert_array_equal(huge[1].cpu().numpy(), whole[1].cpu().numpy())


def _wall_solver(native=True):
    from path_planning.solvers.scp import SCP

    W = rc.WallScene
    occ, origin, cell = W.grid()
    s = SCP(n_vehicles=W.N, time_horizon=W.T, time_step=W.h, min_distance=W.R, space_dims=W.space, native=native, verbose=False)
    s.set_initial_states(W.p0)
    s.set_final_states(W.pf)
    s.set_obstacles(occ, origin, cell)
    return s


def test_shorten_reference_api(ctx):
    W = rc.WallScene
    occ, origin, cell = W.grid()
    s = _wall_solver()
    for stride, clearance in ((None, None), (None, 1), (1, 0), (3, 1)):
        ref, info = s.shorten_reference(stride=stride, clearance=clearance)
        st = W.stride() if stride is None else stride
        cl = st if clearance is None else clearance
        assert info is s.last_info["reference"] and info["stride"] == st and info["clearance"] == cl and info["n_failed"] == 0
        c = rc.Case(f"wall_s{st}_c{cl}", W.D, occ, origin, cell, st, cl, W.K, W.p0, W.pf, max_path=min((40 // st) ** 2, 8 * W.K))
        want = sc.want(c)
        np.testing.assert_array_equal(ref.view(np.uint64), want["ref"].view(np.uint64))
        np.testing.assert_array_equal(info["n_kept"], want["out"]["n_kept"])
        np.testing.assert_array_equal(info["n_nodes"], c.want()["info"]["n_nodes"])
        for f in ("length", "length_before"):
            np.testing.assert_array_equal(info[f].view(np.uint64), want["out"][f].view(np.uint64))
        delta = sr.delta_of(want["out"]["length"], W.K, cell)
        np.testing.assert_array_equal(info["delta"], delta)
        assert info["guaranteed"] == bool((cl >= delta).all()) and info["shorten_ms"] > 0 and info["search_ms"] > 0
    assert s.shorten_reference()[1]["guaranteed"] and not s.shorten_reference(clearance=0)[1]["guaranteed"]
    assert s.shorten_reference()[1]["edges_ms"] == 0.0  # the masks are cached
    for bad in (dict(stride=0), dict(clearance=-1), dict(clearance=1.0), dict(max_path=0), dict(stride=41)):
        with pytest.raises(ValueError):
            s.shorten_reference(**bad)
    # a clearance that closes the gap: nobody crosses, everybody keeps the straight line
    with pytest.raises(ValueError, match="vehicle 0 .*cannot be reached"):
        s.shorten_reference(stride=1, clearance=4)
    ref, info = s.shorten_reference(stride=1, clearance=4, allow_unreachable=True)
    from path_planning.solvers.scp import straight_reference

    np.testing.assert_array_equal(ref, straight_reference(W.p0, W.pf, W.K))
    assert info["n_kept"].tolist() == [0, 0, 0] and info["length"].tolist() == [0.0, 0.0, 0.0] and info["guaranteed"]
    with pytest.raises(ValueError, match="shortened"):
        s.set_corridors(reference="straight")
    s.close()


@pytest.mark.parametrize("native", [True, False])
def test_end_to_end_through_the_gap(ctx, native):
    """The wall with one gap of tests/test_reference_path_gpu.py, with the shortened reference at clearance 1 (delta = 1: no
    segment can be blocked): every segment stays inside its box and the separation checks pass."""
    W = rc.WallScene
    occ, origin, cell = W.grid()
    s = _wall_solver(native)
    info = s.set_corridors(reference="shortened", max_grow=W.max_grow, pad=W.pad)  # (the defaults: clearance = stride)
    assert info["n_blocked"] == 0 and info["n_open"] == 0 and s.last_info["reference"]["clearance"] == W.stride()
    ref, found = s.shorten_reference(clearance=1)
    assert found["guaranteed"] and found["n_failed"] == 0 and found["n_kept"].tolist() == [4, 4, 4]
    assert (found["length"] < found["length_before"]).all()
    info = s.set_corridors(reference=ref, max_grow=W.max_grow, pad=W.pad)
    assert info["n_blocked"] == 0 and info["n_open"] == 0
    traj = s.generate_trajectories(max_iterations=15)
    statuses = [s.last_info["qp0"]["status_val"]] + [it["status_val"] for it in s.last_info["iterations"]]
    assert set(statuses) <= {1, 2}, statuses
    rep = s.validate_solution(continuous=True)
    co = rep["corridor"]
    print(f"native={native}: {len(statuses) - 1} SCP iterations, corridor max_excess {co['max_excess']:.4e}, n_outside {co['n_outside']}, "
          f"min distance {rep['min_pair_distance']:.4f} / continuous {rep['min_pair_distance_continuous']:.4f}")
    assert co["inside"] and co["n_outside"] == 0 and co["n_blocked"] == 0 and co["max_excess"] <= 0.0
    assert rep["collision_free"] and rep["collision_free_continuous"]
    out = s.validate_corridor()
    assert out["inside"] and out["n_outside"] == 0
    idx = np.floor((traj["positions"] - origin) / cell).astype(int)
    assert (occ[0, idx[..., 1], idx[..., 0]] == 0).all()
    want = cr.check_corridor(W.D, W.h, origin, cell, s._corridor["cells"].cpu().numpy(), traj["positions"], traj["velocities"],
                             traj["accelerations"], 0.0)
    np.testing.assert_array_equal(co["vehicles"]["max_excess"].view(np.uint64), want["max_excess"].view(np.uint64))
    s.close()
