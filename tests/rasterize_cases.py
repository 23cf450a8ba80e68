"""The maps the rasteriser tests share: small grids on which rounding matters (cell = 0.3 and origin = -3.3 are not
representable), every kind of shape alone and mixed, shapes outside the grid and sticking out of it, the empty list, capsules
along an axis and exactly on a cell boundary, a non-convex polygon, a vertex on a row of cell centres, a prism taller than
the grid, 300 random shapes, and one polygon over a whole 256 x 256 grid.  The reference grid of a case (tests/rasterize_ref.py
over all cells) is computed once per process."""
import functools

import numpy as np

import rasterize_ref as rr

CELL, ORIGIN = 0.3, -3.3
GRIDS = {2: [(1, 1), (1, 7), (65, 3), (130, 67)], 3: [(5, 4, 3), (33, 17, 9)]}
LARGE = {2: (130, 67), 3: (33, 17, 9)}
BODY = 0.4  # a margin > 0: the body radius of a vehicle with min_distance 0.8


class Case:
    def __init__(self, name, D, dims, margin, discs=(), boxes=(), capsules=(), polygons=()):
        self.name, self.D, self.dims, self.margin = name, D, tuple(dims), float(margin)
        self.origin, self.cell = [ORIGIN] * D, CELL
        self.discs, self.boxes, self.capsules, self.polygons = list(discs), list(boxes), list(capsules), list(polygons)

    @property
    def n_shapes(self):
        return len(self.discs) + len(self.boxes) + len(self.capsules) + len(self.polygons)

    def shapes(self):
        return {"discs": self.discs, "boxes": self.boxes, "capsules": self.capsules, "polygons": self.polygons}

    def want(self):
        return _want(self.name)


def edge(k):
    """the k-th cell boundary of a coordinate, as the grid computes it"""
    return float(np.float64(ORIGIN) + np.float64(CELL) * np.float64(k))


def centre(k):
    """the centre of cell k of a coordinate, as the rule computes it"""
    return float(np.float64(ORIGIN) + np.float64(CELL) * (np.float64(k) + 0.5))


def extent(D, dims):
    lo = np.full(D, ORIGIN)
    return lo, lo + CELL * np.asarray(dims, dtype=np.float64)


def random_shapes(D, dims, rng, n_each, max_vertices=7, scale=1.0):
    """n_each shapes of every kind around the grid: about a third of them reach beyond it or lie outside"""
    lo, hi = extent(D, dims)
    span = hi - lo
    a, b = lo - 0.3 * span - 0.5, hi + 0.3 * span + 0.5
    size = scale * max(float(span.max()), 1.0)

    def point():
        return rng.uniform(a, b)

    discs = [tuple(point()) + (float(rng.uniform(0.0, 0.15 * size)),) for _ in range(n_each)]
    boxes = []
    for _ in range(n_each):
        p = point()
        boxes.append(tuple(p) + tuple(p + rng.uniform(0.0, 0.2 * size, D) * (rng.random(D) > 0.15)))  # (some sides of width 0)
    capsules = []
    for _ in range(n_each):
        p, q = point(), point()
        q = np.where(rng.random(D) < 0.2, p, q)  # (parallel to an axis, or a point)
        capsules.append(tuple(p) + tuple(q) + (float(rng.uniform(0.0, 0.08 * size)) * (rng.random() > 0.25),))
    polygons = []
    for _ in range(n_each):
        n = int(rng.integers(3, max_vertices + 1))
        c, rad = point()[:2], rng.uniform(0.05, 0.3) * size
        ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
        verts = c + (rad * rng.uniform(0.3, 1.0, n))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)  # (a star: non-convex)
        if rng.random() < 0.5:
            verts = verts[::-1]
        if D == 3:
            z = np.sort(rng.uniform(a[2], b[2], 2))
            polygons.append((verts, float(z[0]), float(z[1] if rng.random() > 0.2 else z[0])))
        else:
            polygons.append((verts,))
    return discs, boxes, capsules, polygons


def _heights(D, z0, z1):
    return (z0, z1) if D == 3 else ()


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    for D in (2, 3):
        for dims in GRIDS[D]:
            tag = "x".join(str(n) for n in dims)
            rng = np.random.default_rng(1000 * D + int(np.prod(dims)))
            discs, boxes, capsules, polygons = random_shapes(D, dims, rng, 6)
            for margin in (0.0, BODY):
                m = f"m{margin:g}"
                cases.append(Case(f"{tag}_discs_{m}", D, dims, margin, discs=discs))
                cases.append(Case(f"{tag}_boxes_{m}", D, dims, margin, boxes=boxes))
                cases.append(Case(f"{tag}_capsules_{m}", D, dims, margin, capsules=capsules))
                cases.append(Case(f"{tag}_polygons_{m}", D, dims, margin, polygons=polygons))
                cases.append(Case(f"{tag}_mixed_{m}", D, dims, margin, discs, boxes, capsules, polygons))
            cases.append(Case(f"{tag}_no_shapes", D, dims, BODY))
        dims = LARGE[D]
        tag = "x".join(str(n) for n in dims)
        lo, hi = extent(D, dims)
        far = [100.0] * D
        tri = np.array([[90.0, 90.0], [95.0, 90.0], [92.0, 97.0]])
        cases.append(Case(f"{tag}_outside", D, dims, BODY, discs=[tuple(far) + (2.0,)], boxes=[tuple(far) + tuple(far)],
                          capsules=[tuple(far) + tuple([-100.0] + far[1:]) + (0.5,), tuple([-50.0] * D) + tuple([-60.0] * D) + (1.0,)],
                          polygons=[(tri,) + _heights(D, -1.0, 1.0), (tri - 200.0,) + _heights(D, 90.0, 95.0)]))
        mid = [0.5 * (lo[d] + hi[d]) for d in range(D)]
        cases.append(Case(f"{tag}_sticking_out", D, dims, BODY, discs=[tuple(lo) + (1.0,), tuple(hi) + (0.7,)],
                          boxes=[tuple(lo - 5.0) + tuple(lo + 0.45), tuple(mid[:1] + list(hi[1:] - 0.2)) + tuple(hi + 3.0)],
                          capsules=[tuple(lo - 2.0) + tuple(hi + 2.0) + (0.1,)],
                          polygons=[(np.array([[lo[0] - 3.0, mid[1]], [mid[0], lo[1] - 3.0], [mid[0] + 0.2, mid[1] + 0.1]]),)
                                    + _heights(D, lo[2] - 1.0 if D == 3 else 0.0, mid[2] if D == 3 else 0.0)]))
        # along an axis: with a radius, without one, and through cell interiors
        axis = []
        for d in range(D):
            p, q = list(mid), list(mid)
            p[d], q[d] = lo[d] + 0.17, hi[d] - 0.41
            axis += [tuple(p) + tuple(q) + (0.25,), tuple(q) + tuple(p) + (0.0,)]
            p2 = [v + 0.6 for v in p]
            q2 = list(p2)
            q2[d] = p2[d] + 1.1
            axis.append(tuple(p2) + tuple(q2) + (0.05,))
        for margin in (0.0, BODY):
            cases.append(Case(f"{tag}_axis_capsules_m{margin:g}", D, dims, margin, capsules=axis))
        # exactly on a cell boundary, r = margin = 0: the touch rule occupies the cells on both sides
        on_edge = []
        for d in range(D):
            p = [edge(3) + 0.1] * D
            q = [edge(7) + 0.2] * D
            other = (d + 1) % D
            p[other] = q[other] = edge(4)
            on_edge.append(tuple(p) + tuple(q) + (0.0,))
        cases.append(Case(f"{tag}_on_boundary", D, dims, 0.0, capsules=on_edge))
        # a non-convex "U", counter-clockwise and clockwise, and one with a vertex on a row of cell centres
        u = np.array([[0.0, 0.0], [4.1, 0.0], [4.1, 5.2], [2.9, 5.2], [2.9, 1.3], [1.2, 1.3], [1.2, 5.2], [0.0, 5.2]]) + ([1.05, 2.13] if D == 2 else [-2.9, -3.1])
        z = _heights(D, -2.0, -1.45)
        for margin in (0.0, BODY):
            cases.append(Case(f"{tag}_u_ccw_m{margin:g}", D, dims, margin, polygons=[(u,) + z]))
            cases.append(Case(f"{tag}_u_cw_m{margin:g}", D, dims, margin, polygons=[(u[::-1],) + z]))
        kite = np.array([[centre(5) - 0.01, centre(6)], [centre(12), centre(2)], [centre(20) + 0.02, centre(6)], [centre(12), centre(11)]])
        cases.append(Case(f"{tag}_vertex_on_centres", D, dims, 0.0, polygons=[(kite,) + z, (kite + [6.0, CELL], ) + z]))
        if D == 3:  # the height range leaves the grid: both ways, upwards only, a flat one above it
            square = np.array([[-1.0, -1.0], [0.7, -1.2], [1.1, 0.9], [-0.8, 0.6]])
            cases.append(Case(f"{tag}_tall_prisms", D, dims, BODY, polygons=[(square, lo[2] - 4.0, hi[2] + 4.0), (square + 3.0, mid[2], hi[2] + 9.0),
                                                                            (square - 1.5, hi[2] + 0.2, hi[2] + 0.2)]))
        rng = np.random.default_rng(77 + D)
        cases.append(Case(f"{tag}_300_random", D, dims, BODY, *random_shapes(D, dims, rng, 75, scale=0.12)))
    big = np.array([[-9.0, -9.0], [90.0, -8.0], [91.0, 88.0], [-7.0, 90.0]])  # 256 x 0.3 = 76.8 metres a side
    cases.append(Case("256x256_one_polygon", 2, (256, 256), BODY, polygons=[(big,)]))
    ring = np.array([[-3.0, -3.0], [73.0, -3.0], [73.0, 73.0], [-3.0, 73.0], [-3.0, 20.0], [30.0, 20.0], [30.0, 50.0], [-3.0, 50.0]])
    cases.append(Case("256x256_notched_polygon", 2, (256, 256), 0.0, polygons=[(ring,)], discs=[(40.0, 35.0, 3.0)]))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def _want(name):
    c = by_name(name)
    occ = rr.rasterize_shapes(c.D, c.origin, c.cell, c.dims, margin=c.margin, **c.shapes())
    occ.setflags(write=False)
    return occ


MIXED = [c.name for c in all_cases() if "_mixed_" in c.name or "_300_random" in c.name or c.name.startswith("256x256")]
