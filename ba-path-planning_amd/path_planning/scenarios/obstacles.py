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
