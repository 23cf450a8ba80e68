"""Distance field and clearance on the GPU: scp_obstacle_distance and scp_obstacle_clearance against
tests/obstacle_distance_ref.py (every integer equal), and SCP.obstacle_clearance on the disc scene of tests/corridor_cases.py:
a plan made with searched corridors is clear of the map, the same fleet planned without obstacles is not."""
import numpy as np
import pytest

import corridor_cases as cc
import obstacle_distance_cases as oc
import obstacle_distance_ref as odr

pytestmark = pytest.mark.gpu

FIELD_CASES = {name: (D, occ) for name, D, occ in oc.field_cases()}
PLANS = {p.name: p for p in oc.all_plans()}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def _grid(D, origin, cell, occ):
    from path_planning import _hip

    return _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_equals_the_reference(ctx, name):
    D, occ = FIELD_CASES[name]
    g = _grid(D, [0.0] * D, 1.0, occ)
    d_occ, _ = ctx.occupancy_prepare(D, g, occ)
    for gap in (0, 1):
        got = ctx.obstacle_distance(D, g, d_occ, gap).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, oc.field_want(name, occ, gap), err_msg=f"gap {gap}")
    assert ctx.last_pair_ms() >= 0.0


def test_field_errors(ctx):
    import torch

    from path_planning import _hip

    occ = torch.zeros((1, 4, 4), dtype=torch.uint8, device=ctx.tdev)
    field = torch.zeros((1, 4, 4), dtype=torch.int32, device=ctx.tdev)
    ok = _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (4, 4, 1))
    # nothing is launched by a call that fails its argument checks, so the small buffers are never touched
    for D, g, gap in ((2, _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (32769, 1, 1)), 1), (2, ok, 2), (2, ok, -1), (4, ok, 1),
                      (2, _hip.occupancy_grid(2, [0.0, 0.0], 0.0, (4, 4, 1)), 1)):
        assert ctx.lib.scp_obstacle_distance(ctx.h, D, g, occ.data_ptr(), gap, field.data_ptr()) == -1  # SCP_ERR_INVALID
        assert ctx.lib.scp_last_error(ctx.h)
    assert ctx.lib.scp_obstacle_distance(ctx.h, 2, _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (32769, 1, 1)), occ.data_ptr(), 1,
                                         field.data_ptr()) == -1
    assert b"32768" in ctx.lib.scp_last_error(ctx.h)
    with pytest.raises(ValueError):
        ctx.obstacle_distance(2, _hip.occupancy_grid(2, [0.0, 0.0], 1.0, (5, 4, 1)), occ, 1)
    sat = torch.zeros((1, 4, 4), dtype=torch.int32, device=ctx.tdev)
    x = ctx.tensor(np.full((1, 2, 2), 0.5))
    for bad in (dict(pieces=0), dict(pieces=17), dict(h=0.0), dict(h=np.inf), dict(K=0)):
        with pytest.raises(_hip.HipError) as e:
            ctx.obstacle_clearance(1, bad.get("K", 2), 2, bad.get("h", 0.2), ok, sat, field, bad.get("pieces", 4), x, x, x)
        assert e.value.code == -1


@pytest.mark.parametrize("name", list(PLANS))
def test_clearance_equals_the_reference(ctx, name):
    p = PLANS[name]
    want, want_steps, sat_ref, field_ref = p.want()
    g = _grid(p.D, p.origin, p.cell, p.occ)
    d_occ, sat = ctx.occupancy_prepare(p.D, g, p.occ)
    field = ctx.obstacle_distance(p.D, g, d_occ, 1)
    np.testing.assert_array_equal(field.cpu().numpy().view(np.uint32), field_ref)
    np.testing.assert_array_equal(sat.cpu().numpy(), sat_ref)
    got, steps = ctx.obstacle_clearance(p.N, p.K, p.D, p.h, g, sat, field, p.P, ctx.tensor(p.pos), ctx.tensor(p.vel),
                                        ctx.tensor(p.acc))
    for f in want.dtype.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    np.testing.assert_array_equal(steps, want_steps)
    # the call initialises step_min itself: a second call into the same answers
    again, steps2 = ctx.obstacle_clearance(p.N, p.K, p.D, p.h, g, sat, field, p.P, ctx.tensor(p.pos), ctx.tensor(p.vel),
                                           ctx.tensor(p.acc))
    assert again.tobytes() == got.tobytes() and steps2.tobytes() == steps.tobytes()


def _solver(with_obstacles):
    from path_planning.solvers.scp import SCP

    E = cc.EndToEnd
    s = SCP(n_vehicles=E.N, time_horizon=E.T, time_step=E.h, min_distance=E.R, space_dims=E.space, verbose=False)
    assert s.K == E.K
    s.set_initial_states(E.p0)
    s.set_final_states(E.pf)
    if with_obstacles:
        s.set_obstacles(*E.grid())
    return s


def _check_report(s, rep, pieces):
    """the report's own consistency: the restatement on the same trajectories, steps against vehicles, metres against cells"""
    E = cc.EndToEnd
    occ, origin, cell = E.grid()
    t = s.trajectories
    import corridor_ref as cr

    field = odr.field_brute(occ, 1)
    np.testing.assert_array_equal(s.obstacle_distance_field(), field)
    np.testing.assert_array_equal(s.obstacle_distance_field(gap=0), odr.field_brute(occ, 0))
    want, want_steps = odr.clearance(E.D, E.h, origin, cell, cr.summed_table(occ), field, pieces, t["positions"], t["velocities"],
                                     t["accelerations"])
    ve = rep["vehicles"]
    for f in ("min_sq", "segment", "piece", "cell", "n_touch", "n_off", "n_wide"):
        np.testing.assert_array_equal(ve[f], want[f].astype(np.int64), err_msg=f)
    np.testing.assert_array_equal(ve["clearance"], cell * np.sqrt(want["min_sq"].astype(np.float64)))
    assert (ve["clearance"] >= 0.0).all() and rep["clearance"] == ve["clearance"].min()
    assert ve["clearance"][rep["worst_vehicle"]] == rep["clearance"]
    st = rep["steps"]
    np.testing.assert_array_equal(st["vehicle"], (want_steps & np.uint64(0xFFFFFFFF)).astype(np.int64))
    np.testing.assert_array_equal(st["clearance"], cell * np.sqrt((want_steps >> np.uint64(32)).astype(np.float64)))
    assert st["clearance"].min() == rep["clearance"]  # steps agrees with vehicles: the same minimum ...
    for i in range(E.N):  # ... and no step is closer than the vehicle it names
        mine = st["clearance"][st["vehicle"] == i]
        assert mine.size == 0 or mine.min() >= ve["clearance"][i]
    g_worst = int(ve["segment"][rep["worst_vehicle"]])
    assert st["clearance"][g_worst] == rep["clearance"] and st["vehicle"][g_worst] <= rep["worst_vehicle"]
    assert rep["clear"] == (rep["n_touch"] == 0 and rep["n_wide"] == 0) and rep["n_off"] == 0 and rep["n_wide"] == 0
    assert rep["field_ms"] >= 0.0 and rep["check_ms"] >= 0.0


def test_a_plan_with_searched_corridors_is_clear_of_the_map():
    E = cc.EndToEnd
    s = _solver(True)
    with pytest.raises(ValueError, match="not generated"):
        s.obstacle_clearance()
    info = s.set_corridors(reference="search", max_grow=E.max_grow, pad=E.pad)
    assert info["n_blocked"] == 0 and info["n_open"] == 0
    s.generate_trajectories(max_iterations=15)
    co = s.validate_corridor()
    rep = s.obstacle_clearance()
    print(f"searched corridors: corridor max_excess {co['max_excess']:.4e}; obstacle clearance {rep['clearance']:.4f} m "
          f"(vehicle {rep['worst_vehicle']}), n_touch {rep['n_touch']}, per vehicle {rep['vehicles']['clearance'].tolist()}")
    assert co["inside"] and rep["clear"] and rep["n_touch"] == 0
    _check_report(s, rep, 4)
    assert 1 in s._obstacles.fields
    s.set_obstacles(*E.grid())  # a new map drops the cached field
    assert 1 not in s._obstacles.fields
    s.close()


def test_a_plan_made_without_obstacles_flies_through_the_disc():
    """The same fleet planned without obstacles and judged against the map afterwards: not clear, pieces touch, and the
    report names a vehicle that flies through the rasterised disc.  Its named segment is the FIRST of the vehicle's segments
    whose value is 0 (ties keep the lowest segment) -- the approach, where the samples lie in cells NEXT to the rasterised disc
    (gap-1 field 0), not yet inside it.  So "the sampled positions of the named segment lie inside the rasterised disc" cannot
    hold under the tie rule; what holds, and is asserted: the named vehicle has samples inside the rasterised disc, the named
    segment is no later than the first such segment, a sample of it lies in a cell whose field is 0, and every segment with
    a sample inside counts at least one touching piece.  Measured on an MI355X: vehicle 0, segment 14, samples inside the disc
    in segments 15 .. 24, 68 touching pieces; the field at the nine samples of segment 14 reads 1, 1, 1, 1, 1, 1, 1, 1, 0."""
    E = cc.EndToEnd
    occ, origin, cell = E.grid()
    s = _solver(False)
    traj = s.generate_trajectories(max_iterations=15)
    with pytest.raises(ValueError, match="set_obstacles"):
        s.obstacle_clearance()
    plan = s.trajectories
    s.set_obstacles(occ, origin, cell)  # judging needs the map only: no corridors, no boxes
    assert s.trajectories is plan and s._corridor is None and s._boxes is None
    for pieces in (4, 1):
        rep = s.obstacle_clearance(pieces=pieces)
        assert not rep["clear"] and rep["n_touch"] > 0 and rep["clearance"] == 0.0
        _check_report(s, rep, pieces)
    rep = s.obstacle_clearance()
    i, g = rep["worst_vehicle"], int(rep["vehicles"]["segment"][rep["worst_vehicle"]])
    u = np.linspace(0.0, E.h, 9)[:, None]

    def cells_of(seg):
        pts = traj["positions"][i, seg] + u * traj["velocities"][i, seg] + 0.5 * u * u * traj["accelerations"][i, seg]
        c = np.floor((pts - origin) / cell).astype(int)
        return c[:, 1], c[:, 0]

    field = odr.field_brute(occ, 1)
    inside = [seg for seg in range(E.K) if occ[0][cells_of(seg)].any()]
    print(f"no obstacles in the plan: worst vehicle {i}, segment {g}; its segments with a sample inside the rasterised disc: "
          f"{inside}; n_touch {rep['n_touch']}; field at the samples of segment {g}: {field[0][cells_of(g)].tolist()}")
    assert inside and g <= inside[0] and rep["vehicles"]["n_touch"][i] >= len(inside)
    assert (field[0][cells_of(g)] == 0).any()
    s.close()
