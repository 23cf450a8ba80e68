"""Static obstacles as an occupancy grid (numpy only): the input of SCP.set_obstacles.

A cell is the closed cube [origin + cell * c, origin + cell * (c + 1)] per coordinate -- the same two products and sums the
device code uses for a corridor box in metres, so a box of free cells is free of obstacles as a set of points."""
from __future__ import annotations

import numpy as np


def grid_shape(space_dims, cell):
    """(origin (D,), dims (nx, ny[, nz])) of the grid that covers the workspace box space_dims = [min..., max...]"""
    sd = np.asarray(space_dims, dtype=np.float64).reshape(-1)
    if sd.size not in (4, 6):
        raise ValueError("space_dims needs 4 (2-D) or 6 (3-D) entries [min..., max...]")
    D = sd.size // 2
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f"cell={cell!r}: the edge length of a cell is a finite number > 0")
    origin, top = sd[:D], sd[D:]
    if not (np.isfinite(sd).all() and (top > origin).all()):
        raise ValueError("space_dims: every max must exceed its min, all finite")
    dims = np.maximum(np.ceil((top - origin) / cell - 1e-9).astype(np.int64), 1)
    if int(np.prod(dims)) > 1 << 24:
        raise ValueError(f"a grid of {tuple(int(n) for n in dims)} cells exceeds the supported 2^24 cells: use a larger cell")
    return origin.copy(), tuple(int(n) for n in dims)


SEARCH_MAX_NODES = 32768  # SCP_LATTICE_MAX_NODES of include/scp_hip.h


def default_search_stride(dims, K, D):
    """The stride (cells per lattice block) SCP.find_reference uses by default on a grid dims = (nx, ny[, nz]): the smallest
    s >= 1 with at most 32768 lattice nodes (prod(dims_d // s)) and max_d(dims_d) / s <= max(K - 2, 1), so that a path across
    an unobstructed map has no more vertices than the trajectory has states (E <= K: consecutive reference points then lie on
    one lattice edge or two adjacent ones, and no corridor segment is blocked)."""
    dims = [int(n) for n in dims][:D]
    if len(dims) != D or min(dims) < 1 or K < 1:
        raise ValueError(f"dims={dims!r}, K={K!r}: {D} dimensions >= 1 and K >= 1")
    s = 1
    while int(np.prod([n // s for n in dims], dtype=np.int64)) > SEARCH_MAX_NODES or max(dims) > s * max(K - 2, 1):
        s += 1
    return s


def _cell_edges(origin, cell, dims):
    """per coordinate: (lower edges, upper edges) of its cells"""
    out = []
    for d, n in enumerate(dims):
        idx = np.arange(n, dtype=np.float64)
        out.append((origin[d] + cell * idx, origin[d] + cell * (idx + 1.0)))
    return out


def _gap2(edges, lo_pt, hi_pt):
    """squared distance of every closed cell to the closed box [lo_pt, hi_pt] (a point: lo_pt == hi_pt), shape dims reversed
    ([nz][ny][nx])"""
    D = len(edges)
    total = 0.0
    for d, (lo, hi) in enumerate(edges):
        gap = np.maximum(np.maximum(lo - hi_pt[d], lo_pt[d] - hi), 0.0)
        shape = [1] * D
        shape[D - 1 - d] = gap.size
        total = total + (gap * gap).reshape(shape)
    return total


def rasterize(space_dims, cell, discs=(), boxes=(), margin=0.0):
    """Occupancy grid of discs / spheres and axis-aligned boxes inside the workspace box space_dims = [min..., max...].

    discs: (x, y, r) in 2-D, (x, y, z, r) in 3-D; boxes: (min..., max...).  A cell is occupied if the closed cell is closer
    than `margin` to an obstacle: for a disc, dist(centre, cell) < r + margin; for a box, dist(box, cell) < margin or the two
    touch.  This is conservative by construction: a point closer than `margin` to an obstacle always lies in an occupied cell.
    `margin` is the body radius of a vehicle (SCP uses R / 2: two vehicles may come within R of each other).

    Returns (occ uint8 [nz][ny][nx] (nz = 1 in 2-D), origin (D,), cell)."""
    origin, dims = grid_shape(space_dims, cell)
    D = len(dims)
    cell = float(cell)
    margin = float(margin)
    if not (margin >= 0.0 and np.isfinite(margin)):
        raise ValueError(f"margin={margin!r}: a finite number >= 0")
    edges = _cell_edges(origin, cell, dims)
    occ = np.zeros(dims[::-1], dtype=bool)
    for disc in discs:
        disc = np.asarray(disc, dtype=np.float64).reshape(-1)
        if disc.size != D + 1 or not np.isfinite(disc).all() or disc[D] < 0:
            raise ValueError(f"disc {disc.tolist()}: {D} centre coordinates and a radius >= 0")
        reach = disc[D] + margin
        occ |= _gap2(edges, disc[:D], disc[:D]) < reach * reach
    for box in boxes:
        box = np.asarray(box, dtype=np.float64).reshape(-1)
        if box.size != 2 * D or not np.isfinite(box).all() or (box[D:] < box[:D]).any():
            raise ValueError(f"box {box.tolist()}: [min..., max...] with {2 * D} entries")
        g2 = _gap2(edges, box[:D], box[D:])
        occ |= (g2 < margin * margin) | (g2 == 0.0)
    occ = occ.astype(np.uint8)
    if D == 2:
        occ = occ[None]
    return np.ascontiguousarray(occ), origin, cell


# ---- shapes for the device rasteriser (scp_rasterize_shapes of include/scp_hip.h; SCP.set_obstacle_shapes) ----------------
SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_POLYGON = 0, 1, 2, 3  # SCP_SHAPE_*
MAX_SHAPES, MAX_VERTICES, MAX_POLYGON = 65536, 1 << 20, 4096        # SCP_RASTER_MAX_*
# scp_obstacle_shape, 72 bytes: p = SPHERE c, -, r; BOX min, max; CAPSULE a, b, r (three slots per point); POLYGON z0, z1
SHAPE_DTYPE = np.dtype([("kind", "<i4"), ("first_vertex", "<i4"), ("n_vertices", "<i4"), ("reserved", "<i4"), ("p", "<f8", (7,))])


def _numbers(what, values, size, hint):
    try:
        v = np.asarray(values, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        v = np.empty(0)
    if v.size != size or not np.isfinite(v).all():
        raise ValueError(f"{what} {values!r}: {hint}, all finite")
    return v


def pack_shapes(D, *, discs=(), boxes=(), capsules=(), polygons=()):
    """The shapes of one map, checked and packed for the device rasteriser: {"D", "shapes": records of SHAPE_DTYPE in the
    order discs, boxes, capsules, polygons, "vertices": (n, 2) float64 (the polygons' vertices, one after the other),
    "counts": {"discs", "boxes", "capsules", "polygons"}}.

    discs: (x, y[, z], r), r >= 0 (spheres in 3-D); boxes: (min..., max...), axis-aligned, max >= min -- the tuples rasterize
    takes; capsules: (a..., b..., r): the segment from a to b with radius r >= 0 (an oblique wall, a beam, a pipe);
    polygons: (vertices,) in 2-D and (vertices, z0, z1) or (vertices, (z0, z1)) in 3-D: 3 .. 4096 vertices (n, 2) in the xy
    plane, closed by an implied edge, any winding direction, convex or not (even-odd rule), in 3-D the prism over the heights
    z0 <= z1.  ValueError: a parameter that is not finite, a negative radius, max < min, z1 < z0, a vertex count outside
    3 .. 4096, more than 65536 shapes or 2^20 vertices in all."""
    if D not in (2, 3):
        raise ValueError(f"D={D!r}: 2 or 3")
    discs, boxes, capsules, polygons = list(discs), list(boxes), list(capsules), list(polygons)
    n = len(discs) + len(boxes) + len(capsules) + len(polygons)
    if n > MAX_SHAPES:
        raise ValueError(f"{n} shapes: one map takes at most {MAX_SHAPES}")
    rec = np.zeros(n, dtype=SHAPE_DTYPE)
    vertices = []
    n_vertices = i = 0
    for disc in discs:
        v = _numbers("disc", disc, D + 1, f"{D} centre coordinates and a radius")
        if v[D] < 0:
            raise ValueError(f"disc {v.tolist()}: the radius is negative")
        rec["kind"][i] = SHAPE_SPHERE
        rec["p"][i][:D], rec["p"][i][6] = v[:D], v[D]
        i += 1
    for box in boxes:
        v = _numbers("box", box, 2 * D, f"[min..., max...] with {2 * D} entries")
        if (v[D:] < v[:D]).any():
            raise ValueError(f"box {v.tolist()}: a max lies below its min")
        rec["kind"][i] = SHAPE_BOX
        rec["p"][i][:D], rec["p"][i][3:3 + D] = v[:D], v[D:]
        i += 1
    for capsule in capsules:
        v = _numbers("capsule", capsule, 2 * D + 1, f"(a..., b..., r) with {2 * D + 1} entries")
        if v[2 * D] < 0:
            raise ValueError(f"capsule {v.tolist()}: the radius is negative")
        rec["kind"][i] = SHAPE_CAPSULE
        rec["p"][i][:D], rec["p"][i][3:3 + D], rec["p"][i][6] = v[:D], v[D:2 * D], v[2 * D]
        i += 1
    for polygon in polygons:
        if not isinstance(polygon, (tuple, list)) or not 1 <= len(polygon) <= 3:
            raise ValueError("a polygon is (vertices,) or (vertices, z0, z1)")
        heights = list(polygon[1:])
        if len(heights) == 1 and heights[0] is not None and np.ndim(heights[0]) == 1:
            heights = list(heights[0])
        if heights == [None]:
            heights = []
        try:
            verts = np.asarray(polygon[0], dtype=np.float64)
        except (TypeError, ValueError):
            verts = np.empty((0, 0))
        if verts.ndim != 2 or verts.shape[1] != 2:
            raise ValueError(f"polygon: its vertices need shape (n, 2), got {verts.shape}")
        if not 3 <= verts.shape[0] <= MAX_POLYGON:
            raise ValueError(f"polygon: {verts.shape[0]} vertices, supported are 3 .. {MAX_POLYGON}")
        if not np.isfinite(verts).all():
            raise ValueError("polygon: a vertex is not finite")
        if D == 3:
            z = _numbers("polygon heights", heights, 2, "z0 and z1 of the prism")
            if z[1] < z[0]:
                raise ValueError(f"polygon heights {z.tolist()}: z1 lies below z0")
            rec["p"][i][:2] = z
        elif heights:
            raise ValueError("polygon: a height range needs D = 3")
        rec["kind"][i], rec["first_vertex"][i], rec["n_vertices"][i] = SHAPE_POLYGON, n_vertices, verts.shape[0]
        vertices.append(verts)
        n_vertices += verts.shape[0]
        if n_vertices > MAX_VERTICES:
            raise ValueError(f"the polygons have more than {MAX_VERTICES} vertices in all")
        i += 1
    return {"D": D, "shapes": rec, "vertices": np.concatenate(vertices) if vertices else np.zeros((0, 2)),
            "counts": {"discs": len(discs), "boxes": len(boxes), "capsules": len(capsules), "polygons": len(polygons)}}
