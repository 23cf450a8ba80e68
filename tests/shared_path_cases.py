"""Inputs shared by tests/test_shared_paths_cpu.py and tests/test_shared_paths_gpu.py: the cases of the negotiated routing (a
case of tests/reference_path_cases.py -- a wall with doors and a fleet that has to cross it -- plus the penalties and the
sharing parameters), what tests/shared_path_ref.py makes of them (computed once per case), and the two-door scene for the
planner.  Each case is a few vehicles on the smallest lattice that can still go wrong."""
import numpy as np

import corridor_ref as cr
import obstacle_distance_ref as od
import reference_path_cases as rc
import reference_path_ref as rr
import shared_path_ref as sp
import weighted_path_ref as wr

COST_SENTINEL = 0xA5A5A5A5  # what a row of cost_out holds that no call has written


class SCase:
    """One scp_negotiate_paths on a reference_path_cases.Case: prefer / weight of the node penalties (weight None: pen = NULL),
    share_weight, capacity, groups, rounds"""

    def __init__(self, base, share_weight, capacity, groups, rounds, prefer=0, weight=None):
        self.base, self.name, self.prefer, self.weight = base, base.name, prefer, weight
        self.share_weight, self.capacity, self.groups, self.rounds = share_weight, capacity, groups, rounds
        self._map = self._want = None

    def __getattr__(self, key):  # (D, occ, origin, cell, stride, clearance, K, p0, pf, dims, L, nodes, max_path, N)
        return getattr(self.base, key)

    def ref_in(self):
        """the caller's pre-filled reference: marked, so that a row that must stay untouched is recognised"""
        marked = np.full((self.N, self.K + 1, self.D), -123.456)
        marked.view(np.uint64)[...] ^= np.arange(marked.size, dtype=np.uint64).reshape(marked.shape)
        return marked

    def map(self):
        """{"sat", "edges", "pen"} of the restatements (pen None where weight is None)"""
        if self._map is None:
            sat = cr.summed_table(self.occ)
            edges = rr.lattice_edges(self.D, sat, self.stride, self.clearance)
            pen = None
            if self.weight is not None:
                pen, _ = wr.penalties(self.D, od.field_separable(self.occ, 1), self.stride, self.prefer, self.weight)
            self._map = {"sat": sat, "edges": edges, "pen": pen}
        return self._map

    def negotiate(self, **changed):
        """shared_path_ref.negotiate of the case with some of share_weight / capacity / groups / rounds replaced"""
        m = self.map()
        kw = dict(share_weight=self.share_weight, capacity=self.capacity, groups=self.groups, rounds=self.rounds)
        kw.update(changed)
        return sp.negotiate(self.D, self.origin, self.cell, m["sat"], self.stride, m["edges"], m["pen"], self.p0, self.pf, self.K,
                            self.max_path, self.ref_in(), **kw)

    def want(self):
        """what shared_path_ref.negotiate returns for the case, and "costs": for every round r >= 1 the cost_out of its
        re-routing, rows nobody wrote holding COST_SENTINEL (computed once, never changed)"""
        if self._want is None:
            w = self.negotiate()
            m = self.map()
            costs = []
            for r in range(self.rounds):
                blank = np.full((self.N, self.nodes), COST_SENTINEL, dtype=np.uint32)
                *new, cost, _ = sp.reroute(self.D, self.origin, self.cell, self.dims, self.stride, m["edges"], m["pen"], self.p0,
                                           self.pf, self.K, self.max_path, *w["sets"][r], w["loads"][r], self.share_weight,
                                           self.capacity, self.groups, r % self.groups, cost=blank)
                for a, b in zip(new, w["sets"][r + 1]):
                    assert a.tobytes() == b.tobytes()
                costs.append(cost)
            w["costs"] = costs
            for v in [a for s in w["sets"] for a in s] + w["loads"] + costs:
                v.setflags(write=False)
            self._want = w
        return self._want


def wall2(nx, ny, x, doors):
    """an nx x ny map with a wall along column x, open at the rows of `doors`"""
    occ = rc._grid2(nx, ny)
    occ[0, :, x] = 1
    for y in doors:
        occ[0, y, x] = 0
    return occ


def _fleet(rows, x0, x1, cell=1.0):
    """vehicles from column x0 to column x1, one per row of `rows`"""
    return [rc._centre(x0, y, cell) for y in rows], [rc._centre(x1, y, cell) for y in rows]


def _case2(name, occ, p0, pf, K=30, stride=1, max_path=None, **kw):
    return SCase(rc.Case(name, 2, occ, [0.0, 0.0], 1.0, stride, 0, K, p0, pf, max_path=max_path), **kw)


ROWS8 = (8, 9, 10, 11, 12, 13, 14, 15)


def two_doors(name="two_doors", groups=4, rounds=8, share_weight=70, **kw):
    """24 x 24, a wall along x = 12 with one-cell doors at y = 6 and y = 17, eight vehicles from the left to the right between
    them: alone, each takes the door nearer to it, four through each"""
    p0, pf = _fleet(ROWS8, 2, 21)
    return _case2(name, wall2(24, 24, 12, (6, 17)), p0, pf, share_weight=share_weight, capacity=1, groups=groups, rounds=rounds, **kw)


def wide_doors(name="wide_doors", groups=4, rounds=8):
    """the same wall with three-cell doors, four vehicles each way, capacity 2, node penalties from the distance field.  With
    groups = 1 the whole fleet re-routes at once and swings between the doors: the overuse goes 12, 24, 14, 22, 14 and round 0
    stays the best"""
    a0, af = _fleet(ROWS8[::2], 2, 21)
    b0, bf = _fleet(ROWS8[1::2], 21, 2)
    return _case2(name, wall2(24, 24, 12, (5, 6, 7, 16, 17, 18)), a0 + b0, af + bf, share_weight=70, capacity=2, groups=groups,
                  rounds=rounds, prefer=2, weight=35)


def stride_2():
    """48 x 48 cells at stride 2: the lattice of two_doors, every door two cells wide"""
    p0, pf = _fleet(ROWS8, 2, 21, cell=2.0)
    occ = wall2(48, 48, 24, (12, 13, 34, 35))
    occ[0, :, 25] = occ[0, :, 24]
    return _case2("stride_2", occ, p0, pf, stride=2, share_weight=70, capacity=1, groups=4, rounds=4)


def slab_3d():
    """3-D, 10 x 10 x 3: a wall across x = 5 over all three layers with two holes, six vehicles"""
    occ = np.zeros((3, 10, 10), dtype=np.uint8)
    occ[:, :, 5] = 1
    occ[1, 2, 5] = occ[1, 7, 5] = 0
    p0 = [[1.5, y + 0.5, 1.5] for y in (2, 3, 4, 5, 6, 7)]
    pf = [[8.5, y + 0.5, 1.5] for y in (2, 3, 4, 5, 6, 7)]
    base = rc.Case("slab_3d", 3, occ, [0.0, 0.0, 0.0], 1.0, 1, 0, 20, p0, pf)
    return SCase(base, share_weight=70, capacity=1, groups=3, rounds=6)


def large():
    """96 x 96 (9216 nodes: the instantiation with the 128 KiB field), a wall with two doors, six vehicles, groups 2, rounds 2"""
    rows = (40, 44, 48, 52, 56, 60)
    p0, pf = _fleet(rows, 8, 88)
    return _case2("large", wall2(96, 96, 48, (30, 70)), p0, pf, K=60, max_path=400, share_weight=70, capacity=1, groups=2, rounds=2)


def clamp():
    """two_doors with share_weight at its limit and node penalties: pen + 32768 others is clamped at 32768"""
    return two_doors("clamp", share_weight=32768, rounds=4, prefer=2, weight=70)


def short_max_path():
    """two_doors with max_path = 21: every path of round 0 has 20 nodes; a re-routed vehicle whose way round the others has
    more than 21 keeps its path (four of them over the four rounds)"""
    p0, pf = _fleet(ROWS8, 2, 21)
    return _case2("short_max_path", wall2(24, 24, 12, (6, 17)), p0, pf, max_path=21, share_weight=280, capacity=1, groups=4, rounds=4)


def statuses():
    """two_doors' map with a sealed room; vehicle 1 starts on the wall (status 1), vehicle 3 ends off the grid (status 2),
    vehicle 5 ends in the sealed room (status 3), vehicle 6 ends in its start block; the others cross the wall"""
    occ = wall2(24, 24, 12, (6, 17))
    occ[0, 0:4, 16] = occ[0, 3, 16:24] = 1  # the room x = 17 .. 23, y = 0 .. 2
    p0, pf = _fleet(ROWS8, 2, 21)
    p0[1] = rc._centre(12, 9)
    pf[3] = [30.0, 11.5]
    pf[5] = rc._centre(20, 1)
    pf[6] = [2.2, 14.8]
    return _case2("statuses", occ, p0, pf, share_weight=70, capacity=1, groups=4, rounds=4, prefer=1, weight=70)


def cases():
    out = [two_doors(), wide_doors(), wide_doors("groups_1", groups=1, rounds=4), two_doors("groups_3", groups=3, rounds=6),
           stride_2(), slab_3d(), large(), clamp(), short_max_path(), statuses()]
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def all_cases():
    """cases(), built once per process (their expected outputs are memoised inside)"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


DOOR_CASES = ("two_doors", "wide_doors", "groups_3", "stride_2", "slab_3d", "large")  # overuse[best] < overuse[0]


class TwoDoorScene:
    """The planner's scene: 12 x 12 m at cell 0.5 (the lattice of two_doors at stride 1), a wall across x = 6 with two doors one
    cell wide, eight vehicles from the left to the right, all of them nearer to the door at y = 6: alone, every one takes it.
    Negotiated (share 1, capacity 1, groups 4, rounds 8) the overuse goes 70, 66, 55, 40, 34, 28, 27, 28, 27 -- round 6 is
    kept -- and two vehicles take the other door.  K = 40 >= every E.  The time step is short enough that the boxes of
    set_corridors, shrunk by max|a| h^2 / 8 + pad (about a tenth of a cell), still meet inside a door one cell wide: no state is
    open."""
    N, D, T, h, R = 8, 2, 5.0, 0.125, 0.4
    K = 40
    space = [0.0, 0.0, 12.0, 12.0]
    cell = 0.5
    stride = 1
    rows = (3, 4, 5, 6, 7, 8, 9, 10)
    doors = (6, 17)
    p0 = np.array([rc._centre(2, y, 0.5) for y in rows])
    pf = np.array([rc._centre(21, y, 0.5) for y in rows])
    _case = None

    @classmethod
    def grid(cls):
        return wall2(24, 24, 12, cls.doors), [0.0, 0.0], cls.cell

    @classmethod
    def case(cls):
        """the scene as a case at cell 1: the same lattice and the same blocks, so the same integers"""
        if cls._case is None:
            p0, pf = _fleet(cls.rows, 2, 21)
            cls._case = _case2("two_door_scene", wall2(24, 24, 12, cls.doors), p0, pf, max_path=8 * cls.K, share_weight=70,
                               capacity=1, groups=4, rounds=8)
        return cls._case
