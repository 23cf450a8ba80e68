"""Inputs shared by tests/test_corridor_cpu.py and tests/test_corridor_gpu.py: random occupancy grids with reference paths
through free cells, and the end-to-end scene (one disc obstacle, three vehicles)."""
import numpy as np


def random_grid(rng, dims, density=0.08):
    """occ uint8 [nz][ny][nx] with about `density` occupied cells; dims = (nx, ny[, nz])"""
    shape = tuple(dims[::-1]) if len(dims) == 3 else (1, dims[1], dims[0])
    return (rng.random(shape) < density).astype(np.uint8)


def random_walk_reference(rng, occ, D, origin, cell, N, K):
    """(N, K + 1, D) reference points: a random walk over free cells (steps of at most one cell per coordinate), every point
    somewhere inside its cell"""
    nz, ny, nx = occ.shape
    dims = (nx, ny, nz)[:D]
    free = np.argwhere(occ == 0)  # (z, y, x)
    ref = np.empty((N, K + 1, D))
    for i in range(N):
        z, y, x = free[rng.integers(len(free))]
        c = [int(x), int(y), int(z)][:D]
        for j in range(K + 1):
            ref[i, j] = [origin[d] + cell * (c[d] + rng.uniform(0.05, 0.95)) for d in range(D)]
            for _ in range(20):
                n = [min(max(c[d] + int(rng.integers(-1, 2)), 0), dims[d] - 1) for d in range(D)]
                idx = (n[2] if D == 3 else 0, n[1], n[0])
                if occ[idx] == 0:
                    c = n
                    break
    return ref


def polyline(points, n):
    """n points uniform in arc length along the polyline through `points`"""
    pts = np.asarray(points, dtype=np.float64)
    seg = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    s = np.concatenate([[0.0], np.cumsum(seg)])
    at = np.linspace(0.0, s[-1], n)
    return np.stack([np.interp(at, s, pts[:, d]) for d in range(pts.shape[1])], axis=1)


class EndToEnd:
    """D = 2, space 10 x 10, T = 8, h = 0.2 (K = 40), R = 0.5; one disc of radius 1 at (5, 5), cell 0.25, margin R / 2.
    Vehicle 0 flies (1,5) -> (9,5) over (5, 7.2), vehicle 1 (9,5) -> (1,5) under (5, 2.8), vehicle 2 (1,8) -> (9,8) straight."""
    N, D, T, h, R = 3, 2, 8.0, 0.2, 0.5
    K = 40
    space = [0.0, 0.0, 10.0, 10.0]
    disc = (5.0, 5.0, 1.0)
    cell = 0.25
    max_grow = 8
    pad = 0.02
    p0 = np.array([[1.0, 5.0], [9.0, 5.0], [1.0, 8.0]])
    pf = np.array([[9.0, 5.0], [1.0, 5.0], [9.0, 8.0]])

    @classmethod
    def reference(cls):
        n = cls.K + 1
        return np.stack([polyline([cls.p0[0], (5.0, 7.2), cls.pf[0]], n), polyline([cls.p0[1], (5.0, 2.8), cls.pf[1]], n),
                         polyline([cls.p0[2], cls.pf[2]], n)])

    @classmethod
    def grid(cls):
        from path_planning.scenarios.obstacles import rasterize

        return rasterize(cls.space, cls.cell, discs=[cls.disc], margin=cls.R / 2)
