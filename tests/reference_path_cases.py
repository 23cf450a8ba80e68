"""Inputs shared by tests/test_reference_path_cpu.py and tests/test_reference_path_gpu.py: occupancy grids with starts and
goals for the lattice search, what tests/reference_path_ref.py makes of them (computed once per case), and the end-to-end
scene (a wall with one gap, three vehicles)."""
import numpy as np

import corridor_cases as cc
import corridor_ref as cr
import reference_path_ref as rr


def block_points(rng, D, origin, cell, stride, L, nodes):
    """one point inside the block of every given node (never on its boundary)"""
    pts = np.empty((len(nodes), D))
    for k, node in enumerate(nodes):
        X = rr.node_coords(L, int(node))
        pts[k] = [origin[d] + cell * stride * (X[d] + rng.uniform(0.05, 0.95)) for d in range(D)]
    return pts


class Case:
    """One call of scp_lattice_edges + scp_reference_paths: occ [nz][ny][nx], origin, cell, stride, clearance, K, max_path
    (None: every node), p0 / pf (N, D)"""

    def __init__(self, name, D, occ, origin, cell, stride, clearance, K, p0, pf, max_path=None):
        self.name, self.D, self.occ, self.origin, self.cell = name, D, occ, list(origin), float(cell)
        self.stride, self.clearance, self.K = stride, clearance, K
        self.p0, self.pf = np.ascontiguousarray(p0, dtype=np.float64), np.ascontiguousarray(pf, dtype=np.float64)
        nz, ny, nx = occ.shape
        self.dims = (nx, ny, nz)
        self.L = rr.lattice(D, self.dims, stride)
        self.nodes = self.L[0] * self.L[1] * self.L[2]
        self.max_path = self.nodes if max_path is None else max_path
        self.N = self.p0.shape[0]
        self._want = None

    def ref_in(self):
        """the caller's pre-filled reference: the straight lines"""
        s = (np.arange(self.K + 1, dtype=np.float64) / float(self.K))[None, :, None]
        return self.p0[:, None, :] + s * (self.pf - self.p0)[:, None, :]

    def want(self):
        """{"sat", "edges", "ref", "path", "info", "dist", "n_failed"} of the restatement (computed once, never changed)"""
        if self._want is None:
            sat = cr.summed_table(self.occ)
            edges = rr.lattice_edges(self.D, sat, self.stride, self.clearance)
            ref, path, info, dist, n_failed = rr.reference_paths(self.D, self.origin, self.cell, sat, self.stride, edges, self.p0,
                                                                 self.pf, self.K, self.max_path, self.ref_in())
            self._want = {"sat": sat, "edges": edges, "ref": ref, "path": path, "info": info, "dist": dist, "n_failed": n_failed}
            for v in self._want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._want


def _random_case(name, seed, dims, D, stride, clearance, N, K, density):
    """a random map; starts and goals inside passable blocks (among them the corner blocks where they are passable, so that
    the clipping of the grown range matters), one vehicle whose goal lies in its start block, two arbitrary points"""
    rng = np.random.default_rng(seed)
    occ = cc.random_grid(rng, dims, density)
    origin, cell = [-1.5, 0.25, 2.0][:D], 0.4
    edges = rr.lattice_edges(D, cr.summed_table(occ), stride, clearance)
    L = rr.lattice(D, (list(dims) + [1])[:3], stride)
    passable = np.nonzero(edges >> np.uint32(rr.SELF) & np.uint32(1))[0]
    if passable.size == 0:
        passable = np.array([0])
    border = [n for n in passable if any(x in (0, L[d] - 1) for d, x in enumerate(rr.node_coords(L, int(n))[:D]))]
    starts = rng.choice(passable, N)
    goals = rng.choice(passable, N)
    if border:
        starts[0], goals[1 % N] = border[0], border[-1]
    goals[2 % N] = starts[2 % N]
    p0 = block_points(rng, D, origin, cell, stride, L, starts)
    pf = block_points(rng, D, origin, cell, stride, L, goals)
    top = [origin[d] + cell * dims[d] for d in range(D)]
    if N > 4:
        p0[3] = rng.uniform(origin, top)  # anywhere in the grid: maybe on an occupied block, maybe beyond the lattice
        pf[4] = rng.uniform(origin, top)
    return Case(name, D, occ, origin, cell, stride, clearance, K, p0, pf)


def _grid2(nx, ny):
    return np.zeros((1, ny, nx), dtype=np.uint8)


def _centre(x, y, cell=1.0):
    return [cell * (x + 0.5), cell * (y + 0.5)]


def _forced_cases():
    out = []
    # one node: a 5 x 4 grid at stride 4; cell (4, .) belongs to no node
    occ = _grid2(5, 4)
    out.append(Case("one_node", 2, occ, [0.0, 0.0], 1.0, 4, 0, 5, [[0.5, 0.5], [3.5, 3.5], [4.5, 1.0], [1.0, 1.0]],
                    [[3.2, 2.1], [0.1, 0.2], [1.0, 1.0], [4.2, 1.0]]))
    # status 1: the start on an occupied block / outside the grid / NaN; status 2: the goal beyond the lattice (13 = 4 * 3 + 1)
    # / outside the grid / on an occupied block
    occ = _grid2(13, 11)
    occ[0, 4, 6] = 1
    out.append(Case("status_1_2", 2, occ, [0.0, 0.0], 1.0, 3, 0, 6,
                    [_centre(6, 4), [-0.5, 2.0], [np.nan, 2.0], _centre(1, 1), _centre(1, 1), _centre(1, 1), _centre(7, 5), _centre(1, 1)],
                    [_centre(1, 1), _centre(1, 1), _centre(1, 1), _centre(12, 2), [5.0, 11.0], _centre(7, 3), _centre(1, 1), _centre(10, 8)]))
    # status 3: a closed wall across x = 6
    occ = _grid2(12, 9)
    occ[0, :, 6] = 1
    out.append(Case("closed_wall", 2, occ, [0.0, 0.0], 1.0, 1, 0, 8, [_centre(1, 1), _centre(9, 7), _centre(2, 8)],
                    [_centre(10, 4), _centre(8, 0), _centre(5, 0)]))
    # status 4: the diagonal of an open 12 x 12 map has 12 nodes
    p0, pf = [_centre(0, 0), _centre(0, 0), _centre(3, 3)], [_centre(11, 11), _centre(10, 11), _centre(3, 9)]
    out.append(Case("max_path_short", 2, _grid2(12, 12), [0.0, 0.0], 1.0, 1, 0, 9, p0, pf, max_path=11))
    out.append(Case("max_path_exact", 2, _grid2(12, 12), [0.0, 0.0], 1.0, 1, 0, 9, p0, pf, max_path=12))
    # K = 1, 2, 3 on a long path (E > K): around a wall with its gap at the top
    occ = _grid2(20, 15)
    occ[0, :13, 10] = 1
    for K in (1, 2, 3):
        out.append(Case(f"long_path_K{K}", 2, occ, [0.5, -0.5], 0.5, 1, 0, K, [[1.0, 0.0], [9.0, 6.0]], [[10.0, 0.0], [1.0, 0.2]]))
    return out


def serpentine():
    """64 x 64: a wall on every other row with its gap alternating between the two ends: about 2 000 levels"""
    occ = _grid2(64, 64)
    for k, y in enumerate(range(1, 64, 2)):
        occ[0, y, :] = 1
        occ[0, y, 63 if k % 2 == 0 else 0] = 0
    return Case("serpentine", 2, occ, [0.0, 0.0], 1.0, 1, 0, 40, [_centre(0, 0), _centre(30, 32), _centre(5, 62)],
                [_centre(0, 62), _centre(3, 0), _centre(5, 62)])


def node_cap():
    """an open 256 x 128 map at stride 1: exactly SCP_LATTICE_MAX_NODES nodes"""
    return Case("node_cap", 2, _grid2(256, 128), [0.0, 0.0], 0.5, 1, 0, 50, [_centre(0, 0, 0.5), _centre(255, 127, 0.5)],
                [_centre(255, 127, 0.5), _centre(17, 3, 0.5)])


def many_vehicles():
    """N = 600 on a 20 x 20 map: more workgroups than the chip holds at once"""
    return _random_case("many_vehicles", 600, (20, 20), 2, 1, 0, 600, 5, 0.1)


def cases():
    """every case, in a fixed order (names are unique)"""
    out = []
    for dims in ((13, 11), (50, 37)):
        for stride in (1, 2, 3):
            for clearance in (0, 1, 2):
                out.append(_random_case(f"rand2d_{dims[0]}x{dims[1]}_s{stride}_c{clearance}", 7 * dims[0] + stride, dims, 2, stride,
                                        clearance, 7, 9, 0.06))
    for dims, strides, N in (((5, 4, 3), (1,), 6), ((16, 16, 16), (1, 2), 7)):
        for stride in strides:
            for clearance in (0, 1):
                out.append(_random_case(f"rand3d_{dims[0]}_s{stride}_c{clearance}", 31 * dims[0] + stride, dims, 3, stride,
                                        clearance, N, 8, 0.03))
    out += _forced_cases()
    out += [serpentine(), node_cap(), many_vehicles(), WallScene.case()]
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def all_cases():
    """cases(), built once per process (their expected outputs are memoised inside)"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


class WallScene:
    """The space of corridor_cases.EndToEnd (10 x 10, cell 0.25, K = 40, h = 0.2, R = 0.5) with a wall of two boxes across
    x = 5 that leaves the gap 4 < y < 6.5 (about 2 m after the margin R / 2).  Vehicles 0 and 2 cross from the left, vehicle 1
    from the right, all three through the gap at about the same time: every straight line hits the wall, and the joint QPs
    carry collision rows next to the corridor boxes."""
    N, D, T, h, R = 3, 2, 8.0, 0.2, 0.5
    K = 40
    space = [0.0, 0.0, 10.0, 10.0]
    cell = 0.25
    boxes = [(4.8, 0.0, 5.2, 4.0), (4.8, 6.5, 5.2, 10.0)]
    max_grow = 8
    pad = 0.02
    p0 = np.array([[1.0, 4.0], [9.0, 6.5], [1.0, 8.0]])
    pf = np.array([[9.0, 4.0], [1.0, 6.5], [9.0, 8.0]])

    @classmethod
    def grid(cls):
        from path_planning.scenarios.obstacles import rasterize

        return rasterize(cls.space, cls.cell, boxes=cls.boxes, margin=cls.R / 2)

    @classmethod
    def stride(cls):
        from path_planning.scenarios.obstacles import default_search_stride

        return default_search_stride((40, 40), cls.K, cls.D)

    @classmethod
    def case(cls):
        occ, origin, cell = cls.grid()
        return Case("wall_scene", cls.D, occ, origin, cell, cls.stride(), 0, cls.K, cls.p0, cls.pf,
                    max_path=min((40 // cls.stride()) ** 2, 8 * cls.K))  # (the default of SCP.find_reference)
