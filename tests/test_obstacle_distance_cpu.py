"""Distance field and clearance, without a GPU: the properties of the restatement (tests/obstacle_distance_ref.py) that the
device code is held to exactly -- brute force and the separable rule give the same field, the gap-1 field is the gap-0 field
of the dilated map, a point keeps at least cell * sqrt(field) from the occupied cells and so does every point of a judged
piece --, the struct layout, the binding's tables and the Python surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import obstacle_distance_cases as oc
import obstacle_distance_ref as odr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scp_hip.h")
FIELD_CASES = {name: (D, occ) for name, D, occ in oc.field_cases()}
PLANS = {p.name: p for p in oc.all_plans()}
ROUNDING = 1e-12  # metres: the float arithmetic of the distances compared below (coordinates of a few metres)


@pytest.mark.parametrize("gap", [0, 1])
@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_brute_force_equals_the_separable_rule(name, gap):
    D, occ = FIELD_CASES[name]
    want = oc.field_want(name, occ, gap)
    np.testing.assert_array_equal(odr.field_separable(occ, gap), want)
    assert want.dtype == np.uint32 and want.shape == occ.shape
    if not occ.any():
        assert (want == odr.NONE).all()
    else:
        assert (want[occ != 0] == 0).all() and want.max() < odr.NONE
    if occ.all():
        assert (want == 0).all()


@pytest.mark.parametrize("name", [n for n, (D, occ) in FIELD_CASES.items() if occ.any()])
def test_dilation_identity_against_scipy(name):
    """gap = 0 is the squared Euclidean transform; gap = 1 is the one of the map dilated by a cell per coordinate"""
    ndi = pytest.importorskip("scipy.ndimage")
    D, occ = FIELD_CASES[name]
    for gap, obstacles in ((0, occ != 0), (1, odr.dilate(occ))):
        edt = ndi.distance_transform_edt(~obstacles)
        np.testing.assert_array_equal(np.rint(edt * edt).astype(np.uint32), oc.field_want(name, occ, gap), err_msg=f"gap {gap}")
    np.testing.assert_array_equal(oc.field_want(name, occ, 1), odr.field_brute(odr.dilate(occ), 0))


def _distances(occ, origin, cell, pts):
    """Euclidean distance of every point (M, D) to the union of the closed occupied cells, metres"""
    D = pts.shape[1]
    lo = np.asarray(origin, dtype=np.float64)[:D] + cell * np.argwhere(occ != 0)[:, ::-1][:, :D].astype(np.float64)
    gap = np.maximum(np.maximum(lo[None] - pts[:, None], pts[:, None] - (lo[None] + cell)), 0.0)
    return np.sqrt((gap * gap).sum(axis=2)).min(axis=1)


@pytest.mark.parametrize("name", ["13x11_one_gap_wall", "40x33_density_0.02", "40x33_density_0.5", "6x5x4", "33x9x5",
                                  "20x20x20_one_cell"])
def test_points_keep_the_distance_of_their_cell(name):
    D, occ = FIELD_CASES[name]
    rng = np.random.default_rng(5)
    origin, cell = [-1.5, 0.25, 2.0][:D], 0.4
    dims = np.array(occ.shape[::-1][:D])
    pts = np.asarray(origin) + cell * dims * rng.uniform(0.0, 1.0, (2000, D))
    c = np.floor((pts - np.asarray(origin)) / cell).astype(int)
    assert (c >= 0).all() and (c < dims).all()
    field = oc.field_want(name, occ, 1)
    sq = field[c[:, 2] if D == 3 else 0, c[:, 1], c[:, 0]].astype(np.float64)
    got = _distances(occ, origin, cell, pts)
    assert (got >= cell * np.sqrt(sq) - ROUNDING).all()
    assert (got[sq == 0] <= cell * np.sqrt(D) + ROUNDING).all()  # a zero says "within a cell per coordinate", no more


@pytest.mark.parametrize("name", ["2d_n1_k50_p3", "2d_n5_k64_p1", "3d_n1_k1_p16", "3d_n3_k65_p1"])
def test_sampled_points_keep_the_guaranteed_distance(name):
    """200 points of every judged piece of vehicle 0 (for the plans with one piece per segment: of the first 20 segments of
    every vehicle but the racing one) keep cell * sqrt(value of the piece) from the occupied cells"""
    p = PLANS[name]
    st, step_min, sat, field = p.want()
    dims = field.shape[::-1]
    who = [(0, g) for g in range(p.K)] if p.N == 1 else [(i, g) for i in range(p.N) if i != 2 for g in range(min(p.K, 20))]
    n_inside = n_judged = 0
    u = np.linspace(0.0, 1.0, 200)
    for i, g in who:
        pos, vel, acc = p.pos[i, g], p.vel[i, g], p.acc[i, g]
        for s in range(p.P):
            t0, t1 = odr.piece_times(p.h, p.P, s)
            r = odr.piece_range(p.D, p.h, p.P, s, p.origin, p.cell, dims, pos, vel, acc)
            if r is None:
                continue
            lo, hi = r
            if (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) > odr.MAX_RANGE:
                continue
            n_judged += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                ts = np.where(acc != 0.0, -vel / acc, np.nan)
            n_inside += bool(((ts > t0) & (ts < t1)).any())
            value = int(field[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].min())
            t = (t0 + (t1 - t0) * u)[:, None]
            pts = pos + t * vel + 0.5 * t * t * acc
            c = np.floor((pts - np.asarray(p.origin)) / p.cell).astype(int)  # every sampled point lies in the piece's range
            assert (c >= np.array(lo[:p.D]) - 1).all() and (c <= np.array(hi[:p.D]) + 1).all()
            if value != odr.NONE:
                assert (_distances(p.occ, p.origin, p.cell, pts) >= p.cell * np.sqrt(float(value)) - ROUNDING).all(), (i, g, s)
    assert n_judged >= 16
    if p.P <= 3:  # about a third of the pieces carry an interior extremum where a piece is a third of a segment or more
        assert 0.12 * n_judged <= n_inside <= 0.7 * n_judged, (n_inside, n_judged)


def test_the_plans_exercise_every_rule():
    """what the GPU test relies on the plans for: pieces off the map, wide pieces, touching pieces, the ties, the empty map"""
    ties = 0
    for p in PLANS.values():
        st, step_min, _, field = p.want()
        assert st["reserved"].sum() == 0 and len(step_min) == p.K
        if p.name == "2d_empty_map":
            assert (st["min_sq"] == odr.NONE).all() and (st["segment"] == odr.NONE).all() and (st["piece"] == odr.NONE).all()
            assert (st["cell"] == -1).all() and st["n_touch"].sum() == 0 and st["n_wide"][2] > 0 and st["n_off"][2] > 0
            assert (step_min >> np.uint64(32) == np.uint64(odr.NONE)).all() and (step_min != np.uint64(odr.NO_STEP)).all()
            continue
        if p.N >= 3:
            assert st["min_sq"][0] == st["min_sq"][1] and st["segment"][0] == st["segment"][1]  # the mirror images
            assert st["cell"][0] != st["cell"][1]
            low = step_min & np.uint64(0xFFFFFFFF)
            ties += int((low == 0).sum())
            assert not (low == 1).any()  # vehicle 1 never beats its mirror image
            assert (st["min_sq"][2], st["segment"][2], st["piece"][2]) == (0, 0, 0)  # hovering: every piece ties, the first wins
            assert st["n_touch"][2] >= 3 * p.P and st["n_wide"][2] > 0 and st["n_off"][2] > 0
        if p.N >= 5:
            assert st["n_off"][3] >= (p.K - p.K // 2) * p.P and st["n_touch"][4] > 0
            assert step_min[p.K - 1] != np.uint64(odr.NO_STEP)
    assert ties >= 10
    one = PLANS["2d_n1_k1_p1"].want()
    assert one[0]["min_sq"][0] not in (0, odr.NONE) and one[1][0] == np.uint64(int(one[0]["min_sq"][0]) << 32)


def test_abi_carries_the_two_functions_and_the_struct():
    from path_planning import _hip

    with open(HEADER) as f:
        text = f.read()
    for name in ("scp_obstacle_distance", "scp_obstacle_clearance"):
        assert f"int {name}(" in text and name in _hip.EXPORTS and name in _hip.PROTOTYPES
        assert hasattr(ctypes.CDLL(_hip.library_path()), name)
    assert "#define SCP_OBSTACLE_MAX_RANGE 4096" in text and "#define SCP_OBSTACLE_MAX_PIECES 16" in text
    assert _hip.STRUCTS["scp_obstacle_stats"] is _hip.ObstacleStats and ctypes.sizeof(_hip.ObstacleStats) == 32
    assert _hip.OBSTACLE_STATS_DTYPE.itemsize == 32 and _hip.OBSTACLE_STATS_DTYPE == odr.OBSTACLE_STATS_DTYPE
    assert (_hip.OBSTACLE_MAX_RANGE, _hip.OBSTACLE_MAX_PIECES, _hip.DIST_NONE) == (odr.MAX_RANGE, odr.MAX_PIECES, odr.NONE)
    assert len(_hip.PROTOTYPES["scp_obstacle_distance"][1]) == 6 and len(_hip.PROTOTYPES["scp_obstacle_clearance"][1]) == 14
    assert callable(_hip.Context.obstacle_distance) and callable(_hip.Context.obstacle_clearance)
    assert list(inspect.signature(_hip.Context.obstacle_distance).parameters)[1:] == ["D", "grid", "occ", "gap"]
    assert list(inspect.signature(_hip.Context.obstacle_clearance).parameters)[1:] == ["N", "K", "D", "h", "grid", "sat", "field",
                                                                                       "pieces", "pos", "vel", "acc"]


def test_python_surface_and_argument_errors():
    from path_planning.cli import compute_trajectories as ct
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.obstacle_clearance)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("pieces", 4), ("dev", None)]
    assert [(k, v.default) for k, v in inspect.signature(SCP.obstacle_distance_field).parameters.items()][1:] == [("gap", 1)]

    class OneRank:
        world = 1

    class TwoRanks:
        world = 2

    s = SCP.__new__(SCP)
    s.shard = OneRank()
    s._obstacles = None
    s.trajectories = None
    for call in (s.obstacle_distance_field, s.obstacle_clearance):
        with pytest.raises(ValueError, match="set_obstacles"):
            call()
    s._obstacles = object()
    with pytest.raises(ValueError, match="not generated"):
        s.obstacle_clearance()
    s.trajectories = {}
    for bad in (0, 17, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="pieces"):
            s.obstacle_clearance(pieces=bad)
    for bad in (2, -1, True, None, 0.5):
        with pytest.raises(ValueError, match="gap"):
            s.obstacle_distance_field(gap=bad)
    s.shard = TwoRanks()
    for call in (s.obstacle_distance_field, s.obstacle_clearance):
        with pytest.raises(ValueError, match="one rank"):
            call()

    parser = ct.build_parser()
    assert parser.parse_args([]).obstacle_clearance is None
    args = parser.parse_args(["--obstacle-discs", "5,5,1", "--obstacle-clearance"])
    assert args.obstacle_clearance == 4 and ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    assert parser.parse_args(["--obstacle-discs", "5,5,1", "--obstacle-clearance", "16"]).obstacle_clearance == 16
    for argv in (["--obstacle-clearance"], ["--obstacle-clearance", "2"], ["--obstacle-discs", "5,5,1", "--obstacle-clearance", "0"],
                 ["--obstacle-discs", "5,5,1", "--obstacle-clearance", "17"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    oc_report = {"worst_vehicle": 1, "clearance": 0.25, "vehicles": {"segment": np.array([3, 7])}, "n_touch": 0, "n_off": 2,
                 "n_wide": 0, "clear": True, "field_ms": 0.5, "check_ms": 0.125}
    assert ct.obstacle_clearance_summary(oc_report, 0.2) == (
        "Obstacle clearance: at least 0.2500 m from the occupied cells (vehicle 1, segment 7, t = 1.40 .. 1.60 s); 0 pieces touch "
        "an occupied cell, 2 off the map, 0 too wide to judge; clear (field 0.500 ms, pass 0.125 ms)")
    oc_report.update(clearance=np.inf, clear=False, n_wide=3)
    assert "no piece judged" in ct.obstacle_clearance_summary(oc_report, 0.2) and "NOT clear" in ct.obstacle_clearance_summary(oc_report, 0.2)
