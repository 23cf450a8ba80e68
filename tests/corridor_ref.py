"""numpy restatement of the static-obstacle rules of include/scp_hip.h ("static obstacles"): the summed table, the corridor
boxes, the boxes of the states, the bound overwrite of scp_qp_set_position_boxes and the continuous-time corridor check.
Integers exactly; doubles bit for bit (numpy rounds every product, quotient, sum and difference on its own)."""
import numpy as np

BLOCKED = (0, 0, 0, -1, -1, -1)
NO_SEGMENT = 2**32 - 1

CORRIDOR_STATS_DTYPE = np.dtype([("max_excess", np.float64), ("segment", np.uint32), ("n_blocked", np.uint32),
                                 ("n_outside", np.uint64), ("reserved", np.uint64)])


def summed_table(occ):
    """occ [nz][ny][nx] (nonzero = occupied) -> the inclusive prefix counts, int32, same shape"""
    s = (np.asarray(occ) != 0).astype(np.int64)
    for ax in range(s.ndim):
        s = np.cumsum(s, axis=ax)
    return s.astype(np.int32)


def _sat_at(sat, x, y, z):
    return 0 if x < 0 or y < 0 or z < 0 else int(sat[z, y, x])


def occupied_in(sat, a, b):
    """occupied cells in the inclusive cell range [a, b] (a, b = (x, y, z)): inclusion-exclusion over the table"""
    n = (_sat_at(sat, b[0], b[1], b[2]) - _sat_at(sat, a[0] - 1, b[1], b[2]) - _sat_at(sat, b[0], a[1] - 1, b[2])
         + _sat_at(sat, a[0] - 1, a[1] - 1, b[2]))
    n -= (_sat_at(sat, b[0], b[1], a[2] - 1) - _sat_at(sat, a[0] - 1, b[1], a[2] - 1) - _sat_at(sat, b[0], a[1] - 1, a[2] - 1)
          + _sat_at(sat, a[0] - 1, a[1] - 1, a[2] - 1))
    return n


def cell_of(x, origin_d, cell, dim_d):
    """(inside, cell index) of one coordinate: floor((x - origin) / cell), compared as a double"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.float64(x) - np.float64(origin_d)) / np.float64(cell))
    if not (f >= 0.0 and f < float(dim_d)):
        return False, 0
    return True, int(f)


def corridor_boxes(D, origin, cell, sat, ref, max_grow):
    """sat [nz][ny][nx], ref (N, K+1, D) -> (cells (N, K, 6) int32, n_blocked)"""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    ref = np.asarray(ref, dtype=np.float64)
    N, K = ref.shape[0], ref.shape[1] - 1
    cells = np.zeros((N, K, 6), dtype=np.int32)
    n_blocked = 0
    for i in range(N):
        for g in range(K):
            lo, hi, blocked = [0, 0, 0], [0, 0, 0], False
            for d in range(D):
                in0, c0 = cell_of(ref[i, g, d], origin[d], cell, dims[d])
                in1, c1 = cell_of(ref[i, g + 1, d], origin[d], cell, dims[d])
                blocked |= not (in0 and in1)
                lo[d], hi[d] = min(c0, c1), max(c0, c1)
            if not blocked and occupied_in(sat, lo, hi) != 0:
                blocked = True
            if blocked:
                cells[i, g] = BLOCKED
                n_blocked += 1
                continue
            seed_lo, seed_hi = list(lo), list(hi)
            while True:
                grew = False
                for d in range(D):
                    if seed_lo[d] - lo[d] < max_grow and lo[d] - 1 >= 0:
                        a, b = list(lo), list(hi)
                        a[d] = b[d] = lo[d] - 1
                        if occupied_in(sat, a, b) == 0:
                            lo[d] -= 1
                            grew = True
                    if hi[d] - seed_hi[d] < max_grow and hi[d] + 1 < dims[d]:
                        a, b = list(lo), list(hi)
                        a[d] = b[d] = hi[d] + 1
                        if occupied_in(sat, a, b) == 0:
                            hi[d] += 1
                            grew = True
                if not grew:
                    break
            cells[i, g] = lo + hi
    return cells, n_blocked


def segment_boxes_metres(D, origin, cell, cells):
    """(L, H) of every segment, shape cells.shape[:-1] + (D,): L = origin + cell * lo, H = origin + cell * (hi + 1)"""
    o = np.asarray(origin, dtype=np.float64)[:D]
    c = np.float64(cell)
    L = o + c * cells[..., :D].astype(np.float64)
    H = o + c * (cells[..., 3:3 + D] + 1).astype(np.float64)
    return L, H


def state_boxes(D, origin, cell, cells, shrink):
    """cells (N, K, 6) -> (lo, hi (N, K, D) by state j = 0 .. K-1, n_open)"""
    N, K = cells.shape[:2]
    L, H = segment_boxes_metres(D, origin, cell, cells)
    blocked = cells[..., 3] < cells[..., 0]
    lo = np.full((N, K, D), -np.inf)
    hi = np.full((N, K, D), np.inf)
    s = np.float64(shrink)
    n_open = 0
    for i in range(N):
        for j in range(1, K):
            if blocked[i, j - 1] or blocked[i, j]:
                n_open += 1
                continue
            l = np.where(L[i, j] > L[i, j - 1], L[i, j], L[i, j - 1]) + s
            u = np.where(H[i, j] < H[i, j - 1], H[i, j], H[i, j - 1]) - s
            if (l > u).any():
                n_open += 1
                continue
            lo[i, j], hi[i, j] = l, u
    return lo, hi, n_open


def position_rows(K, h, space, p0, v0, lo, hi):
    """Rows k = 0 .. K-2 of the position block of the QP's bounds after scp_qp_set_position_boxes: (l, u), each (K-1, N*D),
    time-major.  space = [min..., max...], p0 / v0 (N, D), lo / hi (N, K, D) by state."""
    p0 = np.asarray(p0, dtype=np.float64)
    v0 = np.asarray(v0, dtype=np.float64)
    N, D = p0.shape
    smin, smax = np.asarray(space, dtype=np.float64)[:D], np.asarray(space, dtype=np.float64)[D:]
    l = np.empty((K - 1, N * D))
    u = np.empty((K - 1, N * D))
    for k in range(K - 1):
        hk = np.float64(h) * np.float64(k + 1)
        off = p0 + hk * v0
        bl, bu = lo[:, k + 1], hi[:, k + 1]
        l[k] = (np.where(bl > smin, bl, smin) - off).reshape(-1)
        u[k] = (np.where(bu < smax, bu, smax) - off).reshape(-1)
    return l, u


def _value(p, v, a, t):
    return p + (t * v + ((0.5 * t) * t) * a)


def segment_excess(D, h, L, H, p, v, a):
    """excess of ONE segment: L, H, p, v, a are length-D arrays"""
    h = np.float64(h)
    excess = -np.inf
    for d in range(D):
        pd, vd, ad = np.float64(p[d]), np.float64(v[d]), np.float64(a[d])
        vals = [_value(pd, vd, ad, np.float64(0.0)), _value(pd, vd, ad, h)]
        if ad != 0.0:
            ts = -vd / ad
            if ts > 0.0 and ts < h:
                vals.append(_value(pd, vd, ad, ts))
        e = max(L[d] - min(vals), max(vals) - H[d])
        excess = max(excess, e)
    return excess


def check_corridor(D, h, origin, cell, cells, pos, vel, acc, tol):
    """-> a CORRIDOR_STATS_DTYPE array of N records"""
    N, K = cells.shape[:2]
    L, H = segment_boxes_metres(D, origin, cell, cells)
    out = np.zeros(N, dtype=CORRIDOR_STATS_DTYPE)
    for i in range(N):
        best, best_g, n_blocked, n_outside = -np.inf, NO_SEGMENT, 0, 0
        for g in range(K):
            if cells[i, g, 3] < cells[i, g, 0]:
                n_blocked += 1
                continue
            e = segment_excess(D, h, L[i, g], H[i, g], pos[i, g], vel[i, g], acc[i, g])
            n_outside += int(e > tol)
            if best_g == NO_SEGMENT or e > best:
                best, best_g = e, g
        out[i] = (best, best_g, n_blocked, n_outside, 0)
    return out
