"""Inputs shared by tests/test_obstacle_distance_cpu.py and tests/test_obstacle_distance_gpu.py: the maps of the distance
field (the smallest shapes at which each pass can go wrong) and the plans of the clearance pass.  Expected outputs come from
tests/obstacle_distance_ref.py, computed once per process and never changed."""
import numpy as np

import corridor_cases as cc
import corridor_ref as cr
import obstacle_distance_ref as odr


def _grid2(nx, ny):
    return np.zeros((1, ny, nx), dtype=np.uint8)


def _one_gap_wall():
    """13 x 11: a wall across x = 6 with its gap at y = 7, 8"""
    occ = _grid2(13, 11)
    occ[0, :, 6] = 1
    occ[0, 7:9, 6] = 0
    return occ


def _three_cells(nx, ny):
    """three occupied cells along the long side: the first cell, one just beyond 4096 and one in between"""
    occ = _grid2(nx, ny)
    long_x = nx > ny
    for at, across in ((0, 0), (2500, 1), (4097, 2)):
        occ[0, across if long_x else at, at if long_x else across] = 1
    return occ


def field_cases():
    """[(name, D, occ [nz][ny][nx])], in a fixed order"""
    rng = np.random.default_rng(2024)
    out = [("1x1_occupied", 2, np.ones((1, 1, 1), dtype=np.uint8)), ("1x1_free", 2, _grid2(1, 1))]
    for nx, ny in ((70, 1), (1, 70)):  # a row longer than a wave; x-only and y-only work
        occ = _grid2(nx, ny)
        occ.reshape(-1)[[3, 4, 40]] = 1
        out.append((f"{nx}x{ny}", 2, occ))
    corner = _grid2(65, 67)
    corner[0, 0, 0] = 1  # the longest expansions
    out.append(("65x67_corner", 2, corner))
    out.append(("13x11_one_gap_wall", 2, _one_gap_wall()))
    for density in (0.0, 0.02, 0.5, 1.0):
        out.append((f"40x33_density_{density:g}", 2, cc.random_grid(rng, (40, 33), density)))
    out.append(("4100x3", 2, _three_cells(4100, 3)))
    out.append(("3x4100", 2, _three_cells(3, 4100)))
    out.append(("6x5x4", 3, cc.random_grid(rng, (6, 5, 4), 0.1)))
    out.append(("33x9x5", 3, cc.random_grid(rng, (33, 9, 5), 0.03)))
    z_only = np.zeros((70, 1, 1), dtype=np.uint8)
    z_only[[5, 66]] = 1
    out.append(("1x1x70", 3, z_only))
    one = np.zeros((20, 20, 20), dtype=np.uint8)
    one[13, 2, 7] = 1
    out.append(("20x20x20_one_cell", 3, one))
    assert len({n for n, _, _ in out}) == len(out)
    return out


_FIELDS = {}


def field_want(name, occ, gap):
    """the reference field of a case (brute force), computed once"""
    if (name, gap) not in _FIELDS:
        _FIELDS[name, gap] = odr.field_brute(occ, gap)
    return _FIELDS[name, gap]


class Plan:
    """One input of the clearance pass: a map that is symmetric under x -> nx - 1 - x, its origin placed so that the mirror
    line is x = 0, and N random quadratic trajectories (p, v, a drawn so that about a third of the pieces have t* inside)
    with the special vehicles below, as far as N has room for them.
      vehicles 0 and 1 (N >= 3): mirror images of each other -- equal values in every step, so step_min's tie goes to vehicle 0
      vehicle 2 (N >= 3): hovers over an occupied cell for three segments (n_touch; every piece of them ties, the lowest
        (segment, piece) wins); its last three segments race across the map: wide pieces (n_wide) and pieces off the map (n_off)
      vehicle 3 (N >= 5): leaves the grid half way (n_off)
      vehicle 4 (N >= 5): starts beside an occupied cell and crosses it (n_touch)"""

    def __init__(self, name, D, N, K, P, seed, empty=False):
        self.name, self.D, self.N, self.K, self.P, self.h = name, D, N, K, P, 0.2
        rng = np.random.default_rng(seed)
        dims = (96, 80) if D == 2 else (40, 36, 30)
        self.cell = 0.125 if D == 2 else 0.25
        half = cc.random_grid(rng, (dims[0] // 2,) + dims[1:], 0.004 if D == 2 else 0.001)
        occ = np.concatenate([half, half[:, :, ::-1]], axis=2)
        occ[:, 10:14, 20:24] = 1
        occ[:, 10:14, dims[0] - 24:dims[0] - 20] = 1
        if empty:
            occ[:] = 0
        self.occ = occ
        self.origin = [-0.5 * dims[0] * self.cell, 0.25, 2.0][:D]
        width = np.array(dims, dtype=np.float64) * self.cell
        o = np.array(self.origin)
        pos = o + width * rng.uniform(0.15, 0.85, (N, 1, D)) + rng.normal(0.0, 3.0 * self.cell, (N, K, D))  # around a home point
        vel = rng.normal(0.0, 1.5, (N, K, D))
        acc = rng.uniform(-15.0, 15.0, (N, K, D))
        if N >= 3:
            pos[1], vel[1], acc[1] = pos[0], vel[0], acc[0]
            for arr in (pos, vel, acc):
                arr[1, :, 0] = -arr[0, :, 0]
            solid = o + self.cell * (np.array([21.5, 11.5, 0.5 * dims[2] if D == 3 else 0.0])[:D])
            pos[2, :3], vel[2, :3], acc[2, :3] = solid, 0.0, 0.0
            fast = max(K - 3, 0)
            pos[2, fast:], acc[2, fast:] = o + 0.6 * self.cell, 0.0
            vel[2, fast:] = (45.0 if D == 2 else 25.0) * P  # 72 (20) cells per piece and coordinate: 73^2, 21^3 > 4096
            pos[2, K - 1], vel[2, K - 1] = o - 1.0, -vel[2, K - 1]  # (the last one starts outside and flies away)
        if N >= 5:
            pos[3, K // 2:] = o + width + 3.0 * self.cell
            pos[3, K // 2:, 0] = o[0] - 7.0
            beside = solid.copy()
            beside[0] -= 3.0 * self.cell
            pos[4, 0], vel[4, 0], acc[4, 0] = beside, 0.0, 0.0
            vel[4, 0, 0] = 5.0 * self.cell / self.h
        self.pos, self.vel, self.acc = pos, vel, acc
        self._want = None

    def want(self):
        """(records, step_min, sat, field) of the restatement, computed once"""
        if self._want is None:
            sat = cr.summed_table(self.occ)
            field = odr.field_brute(self.occ, 1)
            st, step_min = odr.clearance(self.D, self.h, self.origin, self.cell, sat, field, self.P, self.pos, self.vel, self.acc)
            self._want = (st, step_min, sat, field)
        return self._want


def plans():
    """every N of 1, 3, 5 (five vehicles cross a workgroup of four waves), every K of 1, 50, 64, 65, 130 (below, at and beyond
    one wave's lanes), every P of 1, 3, 16, in 2-D and 3-D, and one empty map"""
    out = [Plan("2d_n5_k130_p3", 2, 5, 130, 3, 1), Plan("2d_n3_k65_p16", 2, 3, 65, 16, 2), Plan("2d_n5_k64_p1", 2, 5, 64, 1, 3),
           Plan("2d_n1_k1_p1", 2, 1, 1, 1, 4), Plan("2d_n1_k50_p3", 2, 1, 50, 3, 5), Plan("3d_n5_k50_p3", 3, 5, 50, 3, 6),
           Plan("3d_n3_k65_p1", 3, 3, 65, 1, 7), Plan("3d_n5_k130_p16", 3, 5, 130, 16, 8), Plan("3d_n1_k1_p16", 3, 1, 1, 16, 9),
           Plan("2d_empty_map", 2, 3, 5, 3, 10, empty=True)]
    assert len({p.name for p in out}) == len(out)
    return out


_PLANS = None


def all_plans():
    """plans(), built once per process (their expected outputs are memoised inside)"""
    global _PLANS
    if _PLANS is None:
        _PLANS = plans()
    return _PLANS
