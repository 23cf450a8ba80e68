"""numpy / plain-Python restatement of the rules of include/scp_hip.h, "static obstacles: distance field and clearance": the
squared distance field of an occupancy grid (by brute force over the occupied cells, and by the separable rule) and the
clearance pass.  Integers exactly; the doubles of the clearance pass are numpy float64 scalars, every product, quotient, sum
and difference rounded on its own, in the order the header states."""
import numpy as np

import corridor_ref as cr

NONE = 2**32 - 1       # UINT32_MAX
NO_STEP = 2**64 - 1    # UINT64_MAX
MAX_RANGE = 4096       # SCP_OBSTACLE_MAX_RANGE
MAX_PIECES = 16        # SCP_OBSTACLE_MAX_PIECES
_INF = np.int64(1) << np.int64(40)

OBSTACLE_STATS_DTYPE = np.dtype([("min_sq", np.uint32), ("segment", np.uint32), ("piece", np.uint32), ("cell", np.int32),
                                 ("n_touch", np.uint32), ("n_off", np.uint32), ("n_wide", np.uint32), ("reserved", np.uint32)])


def _penalty(delta, gap):
    """max(delta - gap, 0)^2 of an int64 array of offsets >= 0"""
    e = np.maximum(delta - gap, 0)
    return e * e


def field_brute(occ, gap):
    """occ [nz][ny][nx] (nonzero = occupied) -> field [nz][ny][nx] uint32: min over the occupied cells o of
    sum_q max(|c_q - o_q| - gap, 0)^2; NONE everywhere without an occupied cell"""
    occ = np.asarray(occ) != 0
    cells = np.argwhere(np.ones(occ.shape, dtype=bool)).astype(np.int64)  # (z, y, x) of every cell, in linear order
    obst = np.argwhere(occ).astype(np.int64)
    if len(obst) == 0:
        return np.full(occ.shape, NONE, dtype=np.uint32)
    out = np.empty(len(cells), dtype=np.int64)
    chunk = max(1, (1 << 20) // len(obst))
    for a in range(0, len(cells), chunk):
        diff = np.abs(cells[a:a + chunk, None, :] - obst[None, :, :])
        out[a:a + chunk] = _penalty(diff, gap).sum(axis=2).min(axis=1)
    return out.reshape(occ.shape).astype(np.uint32)


def _envelope(f, axis, gap):
    """out[n] = min over n' of f[n'] + max(|n - n'| - gap, 0)^2 along `axis` (int64, _INF = no occupied cell)"""
    n = f.shape[axis]
    out = np.full(f.shape, _INF, dtype=np.int64)
    idx = np.arange(n, dtype=np.int64)
    shape = [1, 1, 1]
    shape[axis] = n
    for m in range(n):
        pen = _penalty(np.abs(idx - m), gap).reshape(shape)
        out = np.minimum(out, np.take(f, [m], axis=axis) + pen)
    return np.minimum(out, _INF)


def field_separable(occ, gap):
    """the same field by the separable rule: along x the squared gap distance to the nearest occupied cell of the row, then one
    lower-envelope pass along y and one along z"""
    f = np.where(np.asarray(occ) != 0, np.int64(0), _INF)
    for axis in (2, 1, 0):
        f = _envelope(f, axis, gap)
    return np.where(f >= _INF, NONE, f).astype(np.uint32)


def dilate(occ):
    """a cell is occupied if a cell within one step per coordinate is (the map whose gap-0 field is the gap-1 field of occ)"""
    o = np.asarray(occ) != 0
    out = o.copy()
    for axis in range(3):
        grown = out.copy()
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= out[tuple(hi)]
        grown[tuple(hi)] |= out[tuple(lo)]
        out = grown
    return out


def _value(p, v, a, t):
    return p + (t * v + ((np.float64(0.5) * t) * t) * a)


def piece_extremes(p, v, a, t0, t1):
    """(lo_v, hi_v) of one coordinate over [t0, t1]: the candidates t0, t1 and t* = -v / a if a != 0 and t0 < t* < t1, the min
    / max taken in that order (the first operand unless the second is strictly smaller / greater)"""
    lo_v = hi_v = _value(p, v, a, t0)
    cand = [_value(p, v, a, t1)]
    if a != 0.0:
        ts = -v / a
        if ts > t0 and ts < t1:
            cand.append(_value(p, v, a, ts))
    for c in cand:
        if c < lo_v:
            lo_v = c
        if c > hi_v:
            hi_v = c
    return lo_v, hi_v


def piece_times(h, P, s):
    h = np.float64(h)
    return h * (np.float64(s) / np.float64(P)), h * (np.float64(s + 1) / np.float64(P))


def piece_range(D, h, P, s, origin, cell, dims, p, v, a):
    """the inclusive cell range (lo, hi) of piece s, each (x, y, z); None: the piece is off the map"""
    t0, t1 = piece_times(h, P, s)
    lo, hi = [0, 0, 0], [0, 0, 0]
    off = False
    for d in range(D):
        lo_v, hi_v = piece_extremes(np.float64(p[d]), np.float64(v[d]), np.float64(a[d]), t0, t1)
        with np.errstate(invalid="ignore", over="ignore"):
            flo = np.floor((lo_v - np.float64(origin[d])) / np.float64(cell))
            fhi = np.floor((hi_v - np.float64(origin[d])) / np.float64(cell))
        if not np.isfinite(flo) or not np.isfinite(fhi) or fhi < 0.0 or flo >= float(dims[d]):
            off = True
            continue
        lo[d] = int(max(flo, 0.0))
        hi[d] = int(min(fhi, float(dims[d] - 1)))
    return None if off else (lo, hi)


def clearance(D, h, origin, cell, sat, field, pieces, pos, vel, acc):
    """sat / field [nz][ny][nx] (field at gap = 1), pos / vel / acc (N, K, D) -> (OBSTACLE_STATS_DTYPE records (N,), step_min
    uint64 (K,))"""
    nz, ny, nx = field.shape
    dims = (nx, ny, nz)
    N, K = pos.shape[:2]
    out = np.zeros(N, dtype=OBSTACLE_STATS_DTYPE)
    step_min = [NO_STEP] * K
    for i in range(N):
        best = (NONE, NONE, NONE, -1)
        n_touch = n_off = n_wide = 0
        for g in range(K):
            seg_v, judged = NONE, False
            for s in range(pieces):
                r = piece_range(D, h, pieces, s, origin, cell, dims, pos[i, g], vel[i, g], acc[i, g])
                if r is None:
                    n_off += 1
                    continue
                lo, hi = r
                if (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) > MAX_RANGE:
                    n_wide += 1
                    continue
                judged = True
                n_touch += int(cr.occupied_in(sat, lo, hi) != 0)
                sub = field[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
                value = int(sub.min())
                z, y, x = np.unravel_index(int(np.argmin(sub)), sub.shape)  # the first minimum in (z, y, x) order
                where = ((lo[2] + int(z)) * ny + lo[1] + int(y)) * nx + lo[0] + int(x)
                seg_v = min(seg_v, value)
                if value < best[0]:  # (ascending (g, s): a tie keeps the lower; NONE is never attained)
                    best = (value, g, s, where)
            if judged:
                step_min[g] = min(step_min[g], (seg_v << 32) | i)
        out[i] = best + (n_touch, n_off, n_wide, 0)
    return out, np.array(step_min, dtype=np.uint64)


def point_distance(occ, origin, cell, x):
    """the Euclidean distance from the point x (D,) to the union of the closed occupied cells (inf without one), in metres"""
    obst = np.argwhere(np.asarray(occ) != 0)[:, ::-1].astype(np.float64)  # (x, y, z)
    if len(obst) == 0:
        return np.inf
    D = len(x)
    lo = np.asarray(origin, dtype=np.float64)[:D] + cell * obst[:, :D]
    gap = np.maximum(np.maximum(lo - x, x - (lo + cell)), 0.0)
    return float(np.sqrt((gap * gap).sum(axis=1)).min())
