"""Inputs shared by tests/test_weighted_path_cpu.py and tests/test_weighted_path_gpu.py: the cases of the weighted lattice
search (a case of tests/reference_path_cases.py plus `prefer` and `weight`), what tests/weighted_path_ref.py makes of them
(computed once per case), and the end-to-end scene with a narrow near gap and a wide far one.  Each case is the smallest one
that can expose the mistake its name stands for."""
import numpy as np

import corridor_ref as cr
import obstacle_distance_ref as od
import reference_path_cases as rc
import reference_path_ref as rr
import weighted_path_ref as wr


class WCase:
    """One call of scp_lattice_penalties + scp_reference_paths_weighted on a reference_path_cases.Case: prefer / weight of the
    penalties (weight None: pen = NULL)"""

    def __init__(self, base, prefer=0, weight=None):
        self.base, self.name, self.prefer, self.weight = base, base.name, prefer, weight
        self._want = None

    def __getattr__(self, key):  # (D, occ, origin, cell, stride, clearance, K, p0, pf, dims, L, nodes, max_path, N)
        return getattr(self.base, key)

    def ref_in(self):
        """the caller's pre-filled reference: marked, so that a row that must stay untouched is recognised"""
        marked = np.full((self.N, self.K + 1, self.D), -123.456)
        marked.view(np.uint64)[...] ^= np.arange(marked.size, dtype=np.uint64).reshape(marked.shape)
        return marked

    def want(self):
        """{"sat", "edges", "field", "pen", "rho", "ref", "path", "info", "path_cost", "cost", "n_failed"} of the restatement
        (computed once, never changed); field / pen / rho are None where weight is None"""
        if self._want is None:
            sat = cr.summed_table(self.occ)
            edges = rr.lattice_edges(self.D, sat, self.stride, self.clearance)
            field = pen = rho = None
            if self.weight is not None:
                field = od.field_separable(self.occ, 1)
                pen, rho = wr.penalties(self.D, field, self.stride, self.prefer, self.weight)
            ref, path, info, path_cost, cost, n_failed = wr.reference_paths_weighted(
                self.D, self.origin, self.cell, sat, self.stride, edges, pen, self.p0, self.pf, self.K, self.max_path, self.ref_in())
            self._want = {"sat": sat, "edges": edges, "field": field, "pen": pen, "rho": rho, "ref": ref, "path": path,
                          "info": info, "path_cost": path_cost, "cost": cost, "n_failed": n_failed}
            for v in self._want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._want


def _case2(name, occ, p0, pf, K=6, stride=1, max_path=None, cell=1.0, **kw):
    return WCase(rc.Case(name, 2, occ, [0.0, 0.0], cell, stride, 0, K, p0, pf, max_path=max_path), **kw)


def detour():
    """9 x 5, one obstacle cell under the straight line from (0, 1) to (7, 1): the cheapest path arches away from it and has
    MORE moves than the fewest-move path -- a search that stops when the start is first reached returns the wrong field"""
    occ = rc._grid2(9, 5)
    occ[0, 0, 4] = 1
    return _case2("detour", occ, [rc._centre(0, 1)], [rc._centre(7, 1)], prefer=2, weight=70)


def improve_late():
    """9 x 6: a tunnel one block high between the wall along the bottom row and a wall over x = 2 .. 5, vehicle 0 at its two
    ends.  Through the tunnel it is 5 moves beside walls; the open route over the upper wall has 13 and is cheaper.  The
    start's first finite cost (6300) comes through the tunnel and is lowered rounds later (5528) -- a sweep that relaxes a node
    once and skips it afterwards, as the level sweep does, keeps the first cost"""
    occ = rc._grid2(9, 6)
    occ[0, 0, :] = 1
    occ[0, 2, 2:6] = 1
    return _case2("improve_late", occ, [rc._centre(6, 1), rc._centre(8, 5)], [rc._centre(1, 1), rc._centre(1, 1)], prefer=2,
                  weight=280)


def ties():
    """open 6 x 6, no penalties: many paths of equal cost; direction order decides, the cost is the octile formula"""
    p0 = [rc._centre(0, 0), rc._centre(0, 1), rc._centre(5, 2), rc._centre(1, 4)]
    pf = [rc._centre(5, 5), rc._centre(5, 3), rc._centre(0, 0), rc._centre(4, 4)]
    return _case2("ties", rc._grid2(6, 6), p0, pf)


def _forced():
    base = {c.name: c for c in rc._forced_cases()}
    out = [WCase(base["one_node"], prefer=1, weight=70), WCase(base["status_1_2"], prefer=2, weight=35)]
    out.append(_case2("start_is_goal", rc._grid2(7, 5), [rc._centre(3, 2), [3.1, 2.2]], [[3.9, 2.9], rc._centre(4, 2)], prefer=1,
                      weight=70))
    # status 3: a sealed room around the start of vehicle 0; vehicle 1 stays outside, vehicle 2 moves inside the room
    occ = rc._grid2(11, 9)
    occ[0, 2, 2:7] = occ[0, 6, 2:7] = 1
    occ[0, 2:7, 2] = occ[0, 2:7, 6] = 1
    out.append(_case2("status_3", occ, [rc._centre(4, 4), rc._centre(0, 0), rc._centre(3, 3)],
                      [rc._centre(9, 7), rc._centre(9, 7), rc._centre(5, 5)], prefer=1, weight=70))
    # status 4: the weighted diagonal of an open 12 x 12 map has 12 nodes; max_path is one short of it
    m = base["max_path_short"]
    out.append(WCase(rc.Case("status_4", 2, m.occ, m.origin, m.cell, 1, 0, m.K, m.p0, m.pf, max_path=11), prefer=0, weight=0))
    return out


def limit():
    """weight * prefer = 32768 on the serpentine (every free cell touches a wall: every node pays the whole product, over
    thousands of moves): the largest costs the call supports"""
    s = rc.serpentine()
    return WCase(rc.Case("limit", 2, s.occ, s.origin, s.cell, 1, 0, s.K, s.p0, s.pf), prefer=2, weight=16384)


def cap_8192_8193():
    """two open lattices on either side of the boundary between the two LDS instantiations: 128 x 64 and 8193 x 1"""
    return [_case2("cap_8192", rc._grid2(128, 64), [rc._centre(0, 0)], [rc._centre(127, 63)], K=20),
            _case2("cap_8193", rc._grid2(8193, 1), [rc._centre(8192, 0)], [rc._centre(0, 0)], K=20)]


def node_cap():
    """the open 256 x 128 map: exactly SCP_LATTICE_MAX_NODES nodes, the full 128 KiB field; one vehicle"""
    c = rc.node_cap()
    return WCase(rc.Case("node_cap", 2, c.occ, c.origin, c.cell, 1, 0, c.K, c.p0[:1], c.pf[:1]))


def block_min():
    """stride 3 on 9 x 9 with one occupied cell at (4, 7): the block (1, 1) holds cells 3 .. 5 x 3 .. 5, its centre cell (4, 4)
    has the field 2^2 = 4 (rho 2), its minimum is at (4, 5): 1 (rho 1) -- a kernel that reads the centre cell is found out"""
    occ = rc._grid2(9, 9)
    occ[0, 7, 4] = 1
    return _case2("block_min", occ, [[1.5, 1.5]], [[7.5, 4.5]], stride=3, prefer=3, weight=50)


def _block_cell(stride, off):
    """the index c = x + s y + s^2 z of a cell within its block, as the penalties kernel counts the cells (a wave's lane c mod
    64 reads it in pass c div 64)"""
    return off[0] + stride * off[1] + stride * stride * off[2]


def wave2d_s9():
    """2-D, stride 9 on 27 x 27 (3 x 3 nodes, 81 cells per block: one wave per node, two passes).  The occupied cell (12, 19)
    lies in block (1, 2); the minimum of block (1, 1) is 1 on its top row of cells (cells 72 .. 80 of the block: the SECOND
    pass of the wave, lanes 8 .. 16) while its centre cell reads 25 -- a lost second pass or a wrong lane of the wave minimum
    shows in pen, and the search runs over that pen: vehicle 0 crosses from block (0, 1) to block (2, 1) and goes around block
    (1, 1), which it would cross if that block's penalty came from its centre cell"""
    occ = rc._grid2(27, 27)
    occ[0, 19, 12] = 1
    return _case2("wave2d_s9", occ, [[4.5, 13.5], [22.5, 4.0]], [[22.5, 13.5], [3.0, 22.0]], stride=9, prefer=4, weight=30)


def wave3d_s5():
    """3-D, stride 5 on 10^3 (2 x 2 x 2 nodes, 125 cells per block: one wave per node, two passes).  The occupied cell
    (1, 3, 6) lies in block (0, 0, 1); the minimum of block (0, 0, 0) is 1 on its top layer z = 4 (cells 100 .. 124: the second
    pass), its centre cell reads 9 -- the 3-D block indexing of the wave form"""
    occ = np.zeros((10, 10, 10), dtype=np.uint8)
    occ[6, 3, 1] = 1
    base = rc.Case("wave3d_s5", 3, occ, [0.0, 0.0, 0.0], 1.0, 5, 0, 6, [[2.5, 2.5, 2.5], [7.5, 2.0, 7.0]],
                   [[7.5, 7.5, 7.5], [2.0, 2.0, 2.0]])
    return WCase(base, prefer=4, weight=30)


def thread3d_s3():
    """3-D, stride 3 on 9^3 (27 nodes, 27 cells per block: one thread per node).  The occupied cell (4, 4, 7) lies in block
    (1, 1, 2); the minimum of block (1, 1, 1) is 1 at z offset 2, its centre cell reads 4 -- the 3-D block indexing of the
    thread form"""
    occ = np.zeros((9, 9, 9), dtype=np.uint8)
    occ[7, 4, 4] = 1
    base = rc.Case("thread3d_s3", 3, occ, [0.0, 0.0, 0.0], 1.0, 3, 0, 6, [[1.5, 1.5, 1.5], [7.5, 4.5, 1.0]],
                   [[7.5, 7.5, 7.5], [1.0, 4.0, 4.0]])
    return WCase(base, prefer=3, weight=50)


def cases():
    out = [detour(), improve_late(), ties()] + _forced()
    out.append(WCase(rc._random_case("rand2d_13x11_s2", 93, (13, 11), 2, 2, 0, 5, 9, 0.06), prefer=2, weight=35))
    out.append(WCase(rc._random_case("rand3d_7_s1", 218, (7, 7, 7), 3, 1, 0, 5, 8, 0.03), prefer=2, weight=70))
    out.append(_case2("empty_map", rc._grid2(10, 7), [rc._centre(0, 0), rc._centre(9, 6)], [rc._centre(9, 3), rc._centre(2, 0)],
                      prefer=3, weight=70))
    out += [limit()] + cap_8192_8193() + [node_cap(), block_min(), wave2d_s9(), wave3d_s5(), thread3d_s3()]
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def all_cases():
    """cases(), built once per process (their expected outputs are memoised inside)"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def octile(L, a, b):
    """the cost between two nodes of an open 2-D map without penalties: 140 (max - min) + 198 min of |dx|, |dy|"""
    A, B = rr.node_coords(L, int(a)), rr.node_coords(L, int(b))
    dx, dy = abs(A[0] - B[0]), abs(A[1] - B[1])
    return 140 * (max(dx, dy) - min(dx, dy)) + 198 * min(dx, dy)


class TwoGaps:
    """The space of reference_path_cases.WallScene (10 x 10, cell 0.25, K = 40) with a wall across x = 5 that leaves a NARROW
    gap near the vehicles' line (4.5 < y < 5.5) and a WIDE gap far from it (7 < y < 10).  The fewest-move path takes the near
    gap, whose blocks touch the wall; with keep_clear = 2 the weighted path takes the far one."""
    N, D, T, h, R = 2, 2, 8.0, 0.2, 0.5
    K = 40
    space = [0.0, 0.0, 10.0, 10.0]
    cell = 0.25
    boxes = [(4.8, 0.0, 5.2, 4.5), (4.8, 5.5, 5.2, 7.0)]
    p0 = np.array([[1.0, 5.0], [9.0, 3.0]])
    pf = np.array([[9.0, 5.0], [1.0, 3.0]])
    stride = 2
    keep_clear = 2

    @classmethod
    def grid(cls):
        from path_planning.scenarios.obstacles import rasterize

        return rasterize(cls.space, cls.cell, boxes=cls.boxes, margin=cls.R / 2)

    @classmethod
    def case(cls):
        occ, origin, cell = cls.grid()
        base = rc.Case("two_gaps", cls.D, occ, origin, cell, cls.stride, 0, cls.K, cls.p0, cls.pf,
                       max_path=min((40 // cls.stride) ** 2, 8 * cls.K))
        return WCase(base, prefer=cls.keep_clear, weight=70)


class AssignScene:
    """The map of TwoGaps with three vehicles and three goals anywhere on it, found by a seeded search on the CPU: the pairing
    by weighted length and clearance (keep_clear = 2) costs 6518 against 6552 for the pairing by hop counts, which in turn
    has 39 moves against 40 -- the two costs truly disagree, no tie decides."""
    N, D, T, h, R = 3, 2, 8.0, 0.2, 0.5
    K = 40
    space, cell, boxes, stride, keep_clear = TwoGaps.space, TwoGaps.cell, TwoGaps.boxes, TwoGaps.stride, TwoGaps.keep_clear
    seed = 25
    grid = TwoGaps.grid
    _want = None

    @classmethod
    def points(cls, seed):
        rng = np.random.default_rng(seed)
        p0, pf = rng.uniform(0.8, 9.2, (cls.N, 2)), rng.uniform(0.8, 9.2, (cls.N, 2))
        return p0, pf

    @classmethod
    def pairings(cls, p0, pf):
        """{"hops", "lengths", "by_path", "by_length"} of the two restatements (power = 1)"""
        import assign_paths_ref as ar
        from path_planning.scenarios.assignment import length_costs, path_costs

        occ, origin, cell = cls.grid()
        hops, _, _, _, edges = ar.hop_matrix(cls.D, origin, cell, occ, cls.stride, 0, p0, pf)
        diff = p0[:, None, :] - pf[None, :, :]
        by_path = ar.auction_costs(path_costs(hops, (diff * diff).sum(-1), 1)[0])["goal_of"]
        pen, _ = wr.penalties(cls.D, od.field_separable(occ, 1), cls.stride, cls.keep_clear, 70)
        nz, ny, nx = occ.shape
        lengths = wr.cost_matrix(cls.D, origin, cell, (nx, ny, nz), cls.stride, edges, pen, p0, pf)[0]
        by_length = ar.auction_costs(length_costs(lengths, 1)[0])["goal_of"]
        return {"hops": hops, "lengths": lengths, "by_path": by_path, "by_length": by_length}

    @classmethod
    def want(cls):
        if cls._want is None:
            cls.p0, cls.pf = cls.points(cls.seed)
            cls._want = cls.pairings(cls.p0, cls.pf)
        return cls._want
