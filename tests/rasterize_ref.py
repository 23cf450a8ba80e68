"""The rules of scp_rasterize_shapes (include/scp_hip.h, "static obstacles: shapes into an occupancy grid"), restated in numpy
over ALL cells of the grid: no cell ranges, no work items.  Every product, quotient, sum and difference below is one numpy
operation, so it is rounded on its own like the device code's (compiled without contraction); the device grid is held to this
one with array_equal."""
import numpy as np

SPHERE, BOX, CAPSULE, POLYGON = 0, 1, 2, 3


def cells(D, origin, cell, dims):
    """(LO, HI, CX, CY): per coordinate d < D the lower and upper edges of every cell, flattened in the order of occ
    ([nz][ny][nx], x fastest), and the x / y coordinates of the cells' centres"""
    dims = [int(n) for n in dims] + [1] * (3 - len(dims))
    cell = np.float64(cell)
    idx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims[::-1]), indexing="ij")[::-1]  # idx[d]: [nz][ny][nx]
    LO = [(np.float64(origin[d]) + cell * idx[d]).reshape(-1) for d in range(D)]
    HI = [(np.float64(origin[d]) + cell * (idx[d] + 1.0)).reshape(-1) for d in range(D)]
    CX, CY = ((np.float64(origin[d]) + cell * (idx[d] + 0.5)).reshape(-1) for d in range(2))
    return LO, HI, CX, CY


def box_g2(LO, HI, lo_pt, hi_pt):
    """squared distance of every closed cell to the closed box [lo_pt, hi_pt] (a point: lo_pt == hi_pt)"""
    total = np.zeros(LO[0].shape)
    for d in range(len(LO)):
        g = np.maximum(np.maximum(LO[d] - np.float64(hi_pt[d]), np.float64(lo_pt[d]) - HI[d]), 0.0)
        total = total + g * g
    return total


def segment_f(LO, HI, a, e, t):
    """f(t): the squared distance of the point a + t e to every closed cell"""
    total = np.zeros(LO[0].shape)
    for d in range(len(LO)):
        x = a[d] + t * e[d]
        g = np.maximum(np.maximum(LO[d] - x, x - HI[d]), 0.0)
        total = total + g * g
    return total


def capsule_g2(LO, HI, a, b):
    """squared distance of the segment a -> b to every closed cell: the minimum of f over the rule's finite set of t"""
    D = len(LO)
    a = [np.float64(v) for v in a]
    e = [np.float64(b[d]) - a[d] for d in range(D)]
    n = LO[0].size
    cands = [np.zeros(n), np.ones(n)]
    for d in range(D):
        if e[d] != 0.0:
            for edge in (LO[d], HI[d]):
                with np.errstate(over="ignore"):
                    t = (edge - a[d]) / e[d]
                cands.append(np.where((t > 0.0) & (t < 1.0), t, 1.0))  # (a member twice is a member once)
    T = np.sort(np.stack(cands), axis=0)
    g2 = np.full(n, np.inf)
    for t in T:
        v = segment_f(LO, HI, a, e, t)
        g2 = np.where(v < g2, v, g2)
    for k in range(len(T) - 1):
        t0, t1 = T[k], T[k + 1]
        tm = 0.5 * (t0 + t1)
        num, den = np.zeros(n), np.zeros(n)
        for d in range(D):
            x = a[d] + tm * e[d]
            below, above = x < LO[d], x > HI[d]
            c = np.where(below, a[d] - LO[d], a[d] - HI[d])
            num = num + np.where(below | above, c * e[d], 0.0)
            den = den + np.where(below | above, e[d] * e[d], 0.0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ts = -num / den
        ts = np.where(ts < t0, t0, ts)
        ts = np.where(ts > t1, t1, ts)
        ts = np.where(den == 0.0, tm, ts)  # (f is constant on the interval: its value at the middle carries no rounding of a breakpoint)
        with np.errstate(invalid="ignore"):
            v = segment_f(LO, HI, a, e, ts)
            g2 = np.where((t0 < t1) & (v < g2), v, g2)
    return g2


def polygon_inside(CX, CY, verts):
    """even-odd rule at the cells' centres: the integer count of crossed edges is odd"""
    verts = np.asarray(verts, dtype=np.float64)
    count = np.zeros(CX.shape, dtype=np.int64)
    for i in range(len(verts)):
        p, q = verts[i], verts[(i + 1) % len(verts)]
        straddles = (p[1] <= CY) != (q[1] <= CY)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            at = p[0] + ((CY - p[1]) * (q[0] - p[0])) / (q[1] - p[1])
            count += straddles & (CX < at)
    return count % 2 == 1


def polygon_occupied(D, LO, HI, CX, CY, verts, z0, z1, margin):
    verts = np.asarray(verts, dtype=np.float64)
    margin = np.float64(margin)
    if D == 3:
        gz = np.maximum(np.maximum(LO[2] - np.float64(z1), np.float64(z0) - HI[2]), 0.0)
    else:
        gz = np.zeros(CX.shape)
    gz2, m2 = gz * gz, margin * margin
    hit = np.zeros(CX.shape, dtype=bool)
    for i in range(len(verts)):
        g2 = capsule_g2(LO[:2], HI[:2], verts[i], verts[(i + 1) % len(verts)]) + gz2
        hit |= (g2 < m2) | (g2 == 0.0)
    return hit | (polygon_inside(CX, CY, verts) & ((gz2 < m2) | (gz == 0.0)))


def rasterize_shapes(D, origin, cell, dims, discs=(), boxes=(), capsules=(), polygons=(), margin=0.0):
    """occ uint8 [nz][ny][nx] (nz = 1 in 2-D) of the shapes: discs (c..., r), boxes (min..., max...), capsules (a..., b..., r),
    polygons (vertices (n, 2), z0, z1) -- in 2-D (vertices,) or (vertices, anything)"""
    dims3 = [int(n) for n in dims] + [1] * (3 - len(dims))
    LO, HI, CX, CY = cells(D, origin, cell, dims3)
    margin = np.float64(margin)
    occ = np.zeros(LO[0].shape, dtype=bool)
    for s in discs:
        s = np.asarray(s, dtype=np.float64)
        reach = s[D] + margin
        occ |= box_g2(LO, HI, s[:D], s[:D]) < reach * reach
    for s in boxes:
        s = np.asarray(s, dtype=np.float64)
        g2 = box_g2(LO, HI, s[:D], s[D:])
        occ |= (g2 < margin * margin) | (g2 == 0.0)
    for s in capsules:
        s = np.asarray(s, dtype=np.float64)
        reach = s[2 * D] + margin
        g2 = capsule_g2(LO, HI, s[:D], s[D:2 * D])
        occ |= (g2 < reach * reach) | (g2 == 0.0)
    for poly in polygons:
        verts = poly[0]
        z0, z1 = (poly[1], poly[2]) if D == 3 else (0.0, 0.0)
        occ |= polygon_occupied(D, LO, HI, CX, CY, verts, z0, z1, margin)
    return occ.astype(np.uint8).reshape(dims3[::-1])


def segment_distance2_sampled(lo, hi, a, b, samples=20001):
    """brute force for one cell [lo, hi] (D,): min over `samples` points of the segment; its error is at most the sampling's"""
    lo, hi, a, b = (np.asarray(v, dtype=np.float64) for v in (lo, hi, a, b))
    t = np.linspace(0.0, 1.0, samples)[:, None]
    x = a + t * (b - a)
    g = np.maximum(np.maximum(lo - x, x - hi), 0.0)
    return float((g * g).sum(axis=1).min())
