"""The shape rasteriser, without a GPU: the properties of the restatement (tests/rasterize_ref.py) that the device code is held
to exactly -- it gives the host rasteriser's bits on discs and boxes, its capsule distance is the true one, a degenerate
capsule is a sphere, a polygon's winding does not matter, a rectangle as a polygon is the box, and a point closer than the
reach to a shape lies in an occupied cell --, what pack_shapes rejects, the ABI and the Python surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import rasterize_cases as rc
import rasterize_ref as rr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scp_hip.h")
CASES = {c.name: c for c in rc.all_cases()}


def _space(c):
    """the workspace box whose grid_shape is the case's grid"""
    from path_planning.scenarios.obstacles import grid_shape

    space = list(c.origin) + [c.origin[d] + c.cell * c.dims[d] for d in range(c.D)]
    origin, dims = grid_shape(space, c.cell)
    assert dims == c.dims and origin.tolist() == list(c.origin)
    return space


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.n_shapes and not c.capsules and not c.polygons]
                         + [n for n in CASES if "_mixed_" in n])
def test_discs_and_boxes_give_the_bits_of_the_host_rasteriser(name):
    """margins 0 and > 0, 2-D and 3-D, every grid; of the mixed cases their discs and boxes together"""
    from path_planning.scenarios.obstacles import rasterize

    c = CASES[name]
    occ, origin, cell = rasterize(_space(c), c.cell, discs=c.discs, boxes=c.boxes, margin=c.margin)
    want = c.want() if not (c.capsules or c.polygons) else rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, discs=c.discs,
                                                                               boxes=c.boxes, margin=c.margin)
    assert occ.shape == want.shape and occ.dtype == want.dtype == np.uint8
    np.testing.assert_array_equal(want, occ)


@pytest.mark.parametrize("D", [2, 3])
def test_capsule_distance_against_a_sampled_brute_force(D):
    """g2 never exceeds the minimum over 20 001 samples of the segment (but for the rounding of one evaluation of f) and
    lies below it by no more than the sampling allows: the nearest sample is within delta / 2 = |b - a| / 40 000 of the
    minimiser, so its squared distance exceeds the true one by at most (delta / 2) (2 d + delta / 2).  Rounding: coordinates
    below 16 have an ulp of 1.8e-15, so a gap g < 12 is within 4e-15, its square within 1e-13 and the sum of three within
    1e-12."""
    rng = np.random.default_rng(40 + D)
    worst_below = 0.0
    for trial in range(300):
        lo = rng.uniform(-4.0, 4.0, D)
        hi = lo + rng.uniform(0.05, 2.0, D)
        a, b = rng.uniform(-6.0, 6.0, D), rng.uniform(-6.0, 6.0, D)
        kind = trial % 6
        if kind == 1:  # parallel to an axis
            keep = rng.integers(0, D)
            b = np.where(np.arange(D) == keep, b, a)
        elif kind == 2:  # a point
            b = a.copy()
        elif kind == 3:  # through the middle of the cell
            u = rng.uniform(-3.0, 3.0, D)
            a, b = 0.5 * (lo + hi) - u, 0.5 * (lo + hi) + rng.uniform(0.2, 2.0) * u
        elif kind == 4:  # an end on the cell's boundary plane
            a[0] = lo[0]
        g2 = float(rr.capsule_g2([lo[d:d + 1] for d in range(D)], [hi[d:d + 1] for d in range(D)], a, b)[0])
        brute = rr.segment_distance2_sampled(lo, hi, a, b)
        half = float(np.linalg.norm(b - a)) / 40000.0
        assert g2 <= brute + 1e-12, (trial, g2, brute)
        assert brute - g2 <= half * (2.0 * np.sqrt(g2) + half) + 1e-12, (trial, g2, brute)
        worst_below = max(worst_below, brute - g2)
        if kind == 3:
            assert g2 == 0.0
    print(f"D={D}: the brute force lies above g2 by at most {worst_below:.3e}")


@pytest.mark.parametrize("name", ["130x67_no_shapes", "33x17x9_no_shapes", "65x3_no_shapes"])
def test_a_capsule_of_length_zero_is_the_sphere_bit_for_bit(name):
    c = CASES[name]
    LO, HI, _, _ = rr.cells(c.D, c.origin, c.cell, c.dims)
    rng = np.random.default_rng(3)
    for trial in range(8):
        a = rng.uniform(-5.0, 20.0, c.D)
        if trial == 0:
            a[0] = rc.edge(5)  # on a cell boundary
        sphere = rr.box_g2(LO, HI, a, a)
        capsule = rr.capsule_g2(LO, HI, a, a)
        np.testing.assert_array_equal(capsule.view(np.uint64), sphere.view(np.uint64))
        for r, margin in ((0.7, 0.0), (0.0, 0.4), (1.3, 0.4)):  # (reach > 0: the capsule's touch rule adds no cell)
            np.testing.assert_array_equal(
                rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, capsules=[tuple(a) + tuple(a) + (r,)], margin=margin),
                rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, discs=[tuple(a) + (r,)], margin=margin))


@pytest.mark.parametrize("D", [2, 3])
def test_the_winding_direction_does_not_matter(D):
    tag = "130x67" if D == 2 else "33x17x9"
    for m in ("m0", "m0.4"):
        ccw, cw = CASES[f"{tag}_u_ccw_{m}"], CASES[f"{tag}_u_cw_{m}"]
        assert ccw.want().any() and not ccw.want().all()
        np.testing.assert_array_equal(ccw.want(), cw.want())
    for name in (f"{tag}_polygons_m0", f"{tag}_polygons_m0.4", f"{tag}_vertex_on_centres"):
        c = CASES[name]
        flipped = [(p[0][::-1],) + tuple(p[1:]) for p in c.polygons]
        np.testing.assert_array_equal(rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, polygons=flipped, margin=c.margin), c.want())
    # the "U" is not its convex hull: the cells between its arms are free
    c = CASES[f"{tag}_u_ccw_m0"]
    hull = [(np.array([[0.0, 0.0], [4.1, 0.0], [4.1, 5.2], [0.0, 5.2]]) + (c.polygons[0][0][0]),) + tuple(c.polygons[0][1:])]
    filled = rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, polygons=hull, margin=0.0)
    assert (filled >= c.want()).all() and filled.sum() > c.want().sum() + 10


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("margin", [0.0, 0.1, 0.4, 1.0])
def test_a_rectangle_as_a_polygon_is_the_box(D, margin):
    """corners that are binary fractions, so that a + 1 * (b - a) is b: the two rules then see the same rectangle"""
    dims = rc.LARGE[D]
    origin = [rc.ORIGIN] * D
    for x0, y0, x1, y1, z0, z1 in ((-1.25, -2.5, 3.5, 0.75, -2.75, -1.5), (2.0, -3.0, 2.0, 1.0, -2.0, -2.0), (-8.0, -0.5, 40.0, 0.25, -9.0, 9.0),
                                   (0.5, 0.5, 0.5625, 0.53125, -1.0, -0.96875)):
        rect = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
        poly = (rect, z0, z1) if D == 3 else (rect,)
        box = (x0, y0, z0, x1, y1, z1) if D == 3 else (x0, y0, x1, y1)
        got = rr.rasterize_shapes(D, origin, rc.CELL, dims, polygons=[poly], margin=margin)
        want = rr.rasterize_shapes(D, origin, rc.CELL, dims, boxes=[box], margin=margin)
        np.testing.assert_array_equal(got, want)
        assert want.any()


def _distance_to_segment(pts, a, b):
    e = b - a
    L2 = float(e @ e)
    t = np.clip(((pts - a) @ e) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(pts))
    return np.linalg.norm(pts - (a + t[:, None] * e), axis=1)


def _inside_polygon(pts, verts):
    """even-odd rule in plain floating point, for points that do not lie on an edge"""
    n = len(verts)
    inside = np.zeros(len(pts), dtype=bool)
    for i in range(n):
        p, q = verts[i], verts[(i + 1) % n]
        cond = (p[1] <= pts[:, 1]) != (q[1] <= pts[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            at = p[0] + (pts[:, 1] - p[1]) * (q[0] - p[0]) / (q[1] - p[1])
        inside ^= cond & (pts[:, 0] < at)
    return inside


def _distances(c, pts):
    """(the distance of every point (M, D) to every shape of the case: (n_shapes, M), the reach of every shape)"""
    D = c.D
    out, reach = [], []
    for s in c.discs:
        s = np.asarray(s)
        out.append(np.linalg.norm(pts - s[:D], axis=1))
        reach.append(s[D] + c.margin)
    for s in c.boxes:
        s = np.asarray(s)
        out.append(np.linalg.norm(np.maximum(np.maximum(s[:D] - pts, pts - s[D:]), 0.0), axis=1))
        reach.append(c.margin)
    for s in c.capsules:
        s = np.asarray(s)
        out.append(_distance_to_segment(pts, s[:D], s[D:2 * D]))
        reach.append(s[2 * D] + c.margin)
    for poly in c.polygons:
        verts = np.asarray(poly[0], dtype=np.float64)
        planar = np.min([_distance_to_segment(pts[:, :2], verts[i], verts[(i + 1) % len(verts)]) for i in range(len(verts))], axis=0)
        planar = np.where(_inside_polygon(pts[:, :2], verts), 0.0, planar)
        dz = np.maximum(np.maximum(poly[1] - pts[:, 2], pts[:, 2] - poly[2]), 0.0) if D == 3 else 0.0
        out.append(np.sqrt(planar * planar + dz * dz))
        reach.append(c.margin)
    return np.array(out), np.array(reach)


@pytest.mark.parametrize("name", ["130x67_mixed_m0.4", "130x67_mixed_m0", "33x17x9_mixed_m0.4", "130x67_u_ccw_m0.4", "33x17x9_tall_prisms",
                                  "130x67_sticking_out", "33x17x9_sticking_out", "130x67_axis_capsules_m0.4", "33x17x9_300_random"])
def test_a_point_within_reach_of_a_shape_lies_in_an_occupied_cell(name):
    c = CASES[name]
    rng = np.random.default_rng(9)
    lo, hi = rc.extent(c.D, c.dims)
    pts = rng.uniform(lo, hi, (20000, c.D))
    idx = np.floor((pts - lo) / c.cell).astype(int)
    ok = ((idx >= 0) & (idx < np.asarray(c.dims))).all(axis=1)
    pts, idx = pts[ok], idx[ok]
    dist, reach = _distances(c, pts)
    close = (dist < reach[:, None] - 1e-9).any(axis=0)
    occ = c.want()
    at = occ[idx[:, 2] if c.D == 3 else 0, idx[:, 1], idx[:, 0]]
    assert close.sum() >= 200, close.sum()
    assert (at[close] == 1).all(), int((at[close] == 0).sum())
    # and the grid is no coarser than a cell: an occupied cell's point is within reach + the cell's diagonal of some shape
    assert ((dist - reach[:, None]).min(axis=0)[at == 1] <= c.cell * np.sqrt(c.D) + 1e-9).all()


def test_the_touch_rule_occupies_both_sides_of_a_boundary():
    for name in ("130x67_on_boundary", "33x17x9_on_boundary"):
        c = CASES[name]
        assert c.margin == 0.0 and all(s[-1] == 0.0 for s in c.capsules)
        # the first capsule lies in the plane y = edge(4) between the cells 3 and 4 of y and spans the cells 3 .. 7 of x
        occ = rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, capsules=c.capsules[:1], margin=0.0)
        np.testing.assert_array_equal(occ[:, 3, :], occ[:, 4, :])
        assert occ[:, 3, 3:8].any(axis=0).all() and occ.sum() == 2 * occ[:, 3, :].sum() and not occ[:, :, :3].any() and not occ[:, :, 8:].any()
        if c.D == 2:
            assert occ.sum() == 10
    # a thin oblique segment marks every cell it runs through (r = margin = 0)
    c = CASES["130x67_no_shapes"]
    a, b = np.array([-3.05, -3.17]), np.array([20.3, 11.9])
    occ = rr.rasterize_shapes(2, c.origin, c.cell, c.dims, capsules=[tuple(a) + tuple(b) + (0.0,)], margin=0.0)
    pts = a + np.linspace(0.0, 1.0, 5001)[:, None] * (b - a)
    idx = np.floor((pts - rc.ORIGIN) / rc.CELL).astype(int)
    assert (occ[0, idx[:, 1], idx[:, 0]] == 1).all()


def test_the_half_open_crossing_rule_counts_a_vertex_once():
    c = CASES["130x67_vertex_on_centres"]
    occ = c.want()[0]
    # row 6 holds the kite's left and right vertices exactly on its centres: inside between them, outside beyond them
    assert occ[6, 6:20].all() and not occ[6, :4].any() and not occ[6, 22:24].any()
    LO, HI, CX, CY = rr.cells(2, c.origin, c.cell, c.dims)
    inside = rr.polygon_inside(CX, CY, c.polygons[0][0]).reshape(c.dims[::-1])
    assert inside[6, 6:20].all() and not inside[6, :5].any() and not inside[6, 21:].any()
    assert not inside[1, :].any() and not inside[12, :].any()  # beyond the top and bottom vertices


def test_pack_shapes_packs_and_rejects():
    from path_planning import _hip
    from path_planning.scenarios import obstacles as ob

    assert ob.SHAPE_DTYPE == _hip.OBSTACLE_SHAPE_DTYPE and ob.SHAPE_DTYPE.itemsize == 72
    assert (ob.SHAPE_SPHERE, ob.SHAPE_BOX, ob.SHAPE_CAPSULE, ob.SHAPE_POLYGON) == (rr.SPHERE, rr.BOX, rr.CAPSULE, rr.POLYGON)
    assert (ob.MAX_SHAPES, ob.MAX_VERTICES, ob.MAX_POLYGON) == (_hip.RASTER_MAX_SHAPES, _hip.RASTER_MAX_VERTICES, _hip.RASTER_MAX_POLYGON)
    tri = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    quad = np.array([[2.0, 2.0], [3.0, 2.0], [3.0, 3.0], [2.0, 3.0]])
    pk = ob.pack_shapes(3, discs=[(1, 2, 3, 0.5)], boxes=[(0, 1, 2, 3, 4, 5)], capsules=[(1, 2, 3, 4, 5, 6, 0.25)],
                        polygons=[(tri, -1.0, 2.0), (quad, (0.0, 0.0))])
    s = pk["shapes"]
    assert s["kind"].tolist() == [0, 1, 2, 3, 3] and pk["counts"] == {"discs": 1, "boxes": 1, "capsules": 1, "polygons": 2}
    assert s["p"][0].tolist() == [1, 2, 3, 0, 0, 0, 0.5] and s["p"][1].tolist() == [0, 1, 2, 3, 4, 5, 0]
    assert s["p"][2].tolist() == [1, 2, 3, 4, 5, 6, 0.25] and s["p"][3][:2].tolist() == [-1.0, 2.0]
    assert s["first_vertex"].tolist() == [0, 0, 0, 0, 3] and s["n_vertices"].tolist() == [0, 0, 0, 3, 4]
    assert pk["vertices"].shape == (7, 2) and pk["vertices"][3:].tolist() == quad.tolist()
    pk2 = ob.pack_shapes(2, discs=[(1, 2, 0.5)], boxes=[(0, 1, 3, 4)], capsules=[(1, 2, 4, 5, 0.0)], polygons=[(tri,)])
    assert pk2["shapes"]["p"][1].tolist() == [0, 1, 0, 3, 4, 0, 0] and pk2["shapes"]["p"][2].tolist() == [1, 2, 0, 4, 5, 0, 0]
    empty = ob.pack_shapes(2)
    assert empty["shapes"].size == 0 and empty["vertices"].shape == (0, 2)
    nan, inf = float("nan"), float("inf")
    many = np.zeros((4096, 2))
    many[:, 0] = np.arange(4096)
    bad = [dict(discs=[(1, 2, nan)]), dict(discs=[(inf, 2, 1)]), dict(discs=[(1, 2, -0.1)]), dict(discs=[(1, 2, 3, 1)]),
           dict(boxes=[(0, 0, -1, 1)]), dict(boxes=[(0, nan, 1, 1)]), dict(boxes=[(0, 0, 1)]),
           dict(capsules=[(0, 0, 1, 1, -1e-9)]), dict(capsules=[(0, 0, inf, 1, 1)]), dict(capsules=[(0, 0, 1, 1)]),
           dict(polygons=[(tri[:2],)]), dict(polygons=[(np.zeros((4097, 2)),)]), dict(polygons=[([[0, 0], [1, nan], [0, 1]],)]),
           dict(polygons=[(tri, 0.0, 1.0)]), dict(polygons=[tri]), dict(polygons=[(np.zeros((3, 3)),)]),
           dict(discs=[(0, 0, 1)] * 65537), dict(polygons=[(many,)] * 257)]
    for kw in bad:
        with pytest.raises(ValueError):
            ob.pack_shapes(2, **kw)
    assert ob.pack_shapes(2, discs=[(0, 0, 1)] * 65536)["shapes"].size == 65536
    assert ob.pack_shapes(2, polygons=[(many,)] * 256)["vertices"].shape == (1 << 20, 2)
    for kw in (dict(polygons=[(tri,)]), dict(polygons=[(tri, 1.0, 0.5)]), dict(polygons=[(tri, 0.0, inf)]), dict(discs=[(1, 2, 0.5)]),
               dict(capsules=[(0, 0, 1, 1, 0.1)])):
        with pytest.raises(ValueError):
            ob.pack_shapes(3, **kw)
    with pytest.raises(ValueError):
        ob.pack_shapes(4)


def test_abi_carries_the_function_and_the_struct():
    from path_planning import _hip

    with open(HEADER) as f:
        text = f.read()
    assert "#define SCP_ABI_VERSION 7" in text and _hip.ABI_VERSION == 7
    name = "scp_rasterize_shapes"
    assert f"int {name}(" in text and name in _hip.EXPORTS and name in _hip.PROTOTYPES
    lib = ctypes.CDLL(_hip.library_path())
    assert hasattr(lib, name) and lib.scp_abi_version() == 7
    for define in ("SCP_SHAPE_SPHERE 0", "SCP_SHAPE_BOX 1", "SCP_SHAPE_CAPSULE 2", "SCP_SHAPE_POLYGON 3", "SCP_RASTER_MAX_SHAPES 65536",
                   "SCP_RASTER_MAX_VERTICES 1048576", "SCP_RASTER_MAX_POLYGON 4096"):
        assert "#define " + define in text, define
    assert '"raster_item_cells"' in text
    assert _hip.STRUCTS["scp_obstacle_shape"] is _hip.ObstacleShape and ctypes.sizeof(_hip.ObstacleShape) == 72
    res, args = _hip.PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == 9 and args[4] is ctypes.POINTER(_hip.ObstacleShape)
    assert list(inspect.signature(_hip.Context.rasterize_shapes).parameters)[1:] == ["D", "grid", "packed", "margin"]
    # the whole-ABI checks of tests/test_host_cpu.py see the new symbol and the new struct
    import test_host_cpu as th

    declared = th.header_functions(th.header_text())
    assert declared[name] == ("int", ["scp_ctx*", "int", "scp_occupancy_grid*", "int", "scp_obstacle_shape*", "int", "double*", "double", "uint8_t*"])
    assert th.prototype_errors(_hip.PROTOTYPES, _hip.STRUCTS, declared) == []
    assert th.header_structs(th.header_text())["scp_obstacle_shape"] == ["kind", "first_vertex", "n_vertices", "reserved", "p"]


def test_python_surface_and_argument_errors():
    from path_planning.cli import compute_trajectories as ct
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.set_obstacle_shapes)
    assert [(k, v.default, v.kind) for k, v in sig.parameters.items()][1:] == [
        ("cell", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD)] + [
        (k, d, inspect.Parameter.KEYWORD_ONLY) for k, d in (("discs", ()), ("boxes", ()), ("capsules", ()), ("polygons", ()), ("margin", None))]
    assert SCP.obstacle_info is None

    class TwoRanks:
        world = 2

    class OneRank:
        world = 1

    s = SCP.__new__(SCP)
    s.shard = TwoRanks()
    with pytest.raises(ValueError, match="one rank"):
        s.set_obstacle_shapes(0.25)
    s.shard, s.D, s.space_dims, s.R = OneRank(), 2, [0.0, 0.0, 10.0, 10.0], 0.5
    for kw in (dict(discs=[(1, 1, -1)]), dict(capsules=[(0, 0, 1, 1)]), dict(polygons=[([[0, 0], [1, 1]],)]), dict(margin=-1.0),
               dict(margin=float("nan"))):
        with pytest.raises(ValueError):  # (all before the first device call)
            s.set_obstacle_shapes(0.25, **kw)
    with pytest.raises(ValueError, match="cell"):
        s.set_obstacle_shapes(0.0)

    parser = ct.build_parser()
    args = parser.parse_args(["--obstacle-capsules", "1,2,3,4,0.5", "--obstacle-polygons", "0,0,1,0,0,1", "2,2,3,2,3,3,2,3",
                              "--obstacle-boxes", "0,1,2,3", "--corridor-search", "--obstacle-clearance"])
    assert ct.obstacle_discs(parser, args) is None
    shapes = ct.obstacle_shapes(parser, args)
    assert shapes["capsules"] == [(1.0, 2.0, 3.0, 4.0, 0.5)] and shapes["boxes"] == [(0.0, 1.0, 2.0, 3.0)]
    assert [p[0].tolist() for p in shapes["polygons"]] == [[[0, 0], [1, 0], [0, 1]], [[2, 2], [3, 2], [3, 3], [2, 3]]]
    assert all(len(p) == 1 for p in shapes["polygons"])
    args = parser.parse_args(["--dim", "3", "--obstacle-discs", "1,2,3,1", "--obstacle-polygons", "0,0,1,0,0,1:-1,2.5"])
    assert ct.obstacle_discs(parser, args) == [(1.0, 2.0, 3.0, 1.0)]
    assert ct.obstacle_shapes(parser, args)["polygons"][0][1:] == (-1.0, 2.5)
    args = parser.parse_args(["--obstacle-discs", "5,5,1"])  # the discs alone go the host's way, as before
    assert ct.obstacle_shapes(parser, args) is None and ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    for argv in (["--obstacle-capsules", "1,2,3,4"], ["--obstacle-boxes", "1,2,3"], ["--obstacle-polygons", "0,0,1,0"],
                 ["--obstacle-polygons", "0,0,1,0,0,1:0,1"], ["--obstacle-polygons", "0,0,1,0,0"], ["--obstacle-capsules", "a,2,3,4,1"],
                 ["--dim", "3", "--obstacle-polygons", "0,0,1,0,0,1"]):
        with pytest.raises(SystemExit):
            ct.obstacle_shapes(parser, parser.parse_args(argv))
    for argv in (["--corridor-search"], ["--obstacle-clearance"], ["--corridor-cell", "0.5"]):  # still need an obstacle flag
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    with pytest.raises(SystemExit):  # the range check of --obstacle-clearance holds without discs too
        ct.obstacle_discs(parser, parser.parse_args(["--obstacle-boxes", "0,1,2,3", "--obstacle-clearance", "17"]))
    oi = {"n_shapes": 3, "counts": {"discs": 0, "boxes": 0, "capsules": 2, "polygons": 1}, "margin": 0.25, "n_occupied": 120,
          "n_cells": 1600, "rasterize_ms": 0.0625, "prepare_ms": 0.125}
    assert ct.obstacle_shapes_summary(oi) == ("Obstacles: 3 shapes (2 capsules, 1 polygons) rasterised on the GPU with margin 0.25 m: "
                                              "120 of 1600 cells occupied (0.062 ms, summed table 0.125 ms)")
