"""The entry tables a persistent ADMM workgroup builds for itself (build_entry_tables, csrc/scp_qp_persist_device.h), stated
in numpy and checked on the CPU against a host restatement of the global build (the csr_* kernels of csrc/scp_qp_rows.hip)
and of the in-kernel build, for the working sets tests/test_persist_lists_gpu.py runs.

expected_tables() is the statement: for the block of agents [a0, a1), the entries (row n, side) whose agent lies in the
block, ordered by cell (local agent, time step) and by code 2 n + side inside a cell, and the exclusive cell offsets.  The
GPU test's assertions on its inputs (a cell with >= 3 entries, a row inside one block, a row across blocks) are checked here
too, so they are not the only check of what that test compares."""
import dataclasses

import numpy as np
import pytest

import persist_cases as pc
from oracle import qp_oracle as qo


# ---- the working sets ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class ListCase:
    scen: pc.Scenario
    kernels: tuple        # settings.persistent values of the scenario's row in pc's table
    rows: int             # what the issue's table states, checked below
    max_cell: int
    cells_ge3: int = -1   # (-1: not stated)
    inside8: int = -1
    across8: int = -1
    per_block8: tuple = ()


CASES = [
    ListCase(pc.Scenario("near", 116, 17, 16, 2), (4, 3, 2), 523, 7, 234, 327, 196, (490, 514, 42)),
    ListCase(pc.Scenario("circle", 1, 33, 50, 2), (4, 3, 2), 689, 5, 81, 143, 546, (382, 313, 291, 320, 72)),
    ListCase(pc.Scenario("near", 3161, 9, 16, 3), (4, 3), 194, 5),
    ListCase(pc.Scenario("near", 3501, 17, 50, 3, 0.05), (3,), 342, 3),
]
N33 = CASES[1]
OVERFLOW = pc.Scenario("circle", 2, 16, 50, 2)  # every one of its 6000 rows goes into the working set


def rows_of(prob, W):
    """(w_k, w_i, w_j) of the working rows in the order the solver holds them (row n = W[n])"""
    k, i, j = qo.working_rows(prob, np.asarray(W, dtype=np.int64))
    return np.asarray(k, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)


def without_agents(prob, W, lo, hi):
    """W without the rows that touch an agent in [lo, hi)"""
    _, i, j = rows_of(prob, W)
    keep = ~(((i >= lo) & (i < hi)) | ((j >= lo) & (j < hi)))
    return np.asarray(W)[keep]


def halves_high_first(W):
    """the set in two batches, the higher row ids first: row n of the solver is no longer ascending in the row id"""
    W = np.sort(np.asarray(W))
    return [W[W.size // 2:], W[: W.size // 2]]


def set_labels(case):
    """the labels of working_sets(case), without running the oracle"""
    return ["all", "high-ids-first"] + (["no-rows-at-agents-8..15"] if case is N33 else [])


def working_sets(case):
    """[(label, [batches of row ids in the order they are added])] of a case"""
    prob, _, _, _, _, W = pc.setup(case.scen)
    sets = [("all", [W]), ("high-ids-first", halves_high_first(W))]
    if case is N33:
        sets.append(("no-rows-at-agents-8..15", [without_agents(prob, W, 8, 16)]))
    assert [label for label, _ in sets] == set_labels(case)
    return sets


# ---- the statement -------------------------------------------------------------------------------------------------------
def cell_stats(K, N, wk, wi, wj):
    return np.bincount(np.concatenate([wi * K + wk, wj * K + wk]), minlength=N * K)


def expected_tables(K, wk, wi, wj, a0, a1):
    """(cptr [(a1 - a0) K + 1], codes [entries of the block]) of the block of agents [a0, a1)"""
    n = np.arange(wk.size, dtype=np.int64)
    code = np.concatenate([2 * n, 2 * n + 1])
    agent = np.concatenate([wi, wj])
    kk = np.concatenate([wk, wk])
    own = (agent >= a0) & (agent < a1)
    cell = (agent[own] - a0) * K + kk[own]
    code = code[own]
    order = np.lexsort((code, cell))  # by cell, ascending code inside a cell
    cptr = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=(a1 - a0) * K))])
    return cptr.astype(np.int64), code[order]


def block_counts(N, per, wi, wj):
    nb = (N + per - 1) // per
    return np.bincount(wi // per, minlength=nb) + np.bincount(wj // per, minlength=nb)


def assert_inputs_detect_order(K, N, wk, wi, wj, per):
    """what the GPU comparison needs of its input: two entries of a cell commute in every sum, only a cell with >= 3 detects a
    wrong order; rows with both ends in one block and rows across blocks take different paths through the exchange"""
    assert cell_stats(K, N, wk, wi, wj).max() >= 3
    same = (wi // per) == (wj // per)
    if N > per:
        assert same.any() and (~same).any()


# ---- host restatements of the two builds ---------------------------------------------------------------------------------
def insertion_sort(a):
    a = list(a)
    for i in range(1, len(a)):
        v, j = a[i], i - 1
        while j >= 0 and a[j] > v:
            a[j + 1] = a[j]
            j -= 1
        a[j + 1] = v
    return a


def global_build(N, K, wk, wi, wj, rng):
    """csr_count / scan / fill (the atomics in an arbitrary order) / sort: (cell_ptr [N K + 1], ent_code [2 nW])"""
    ncell = N * K
    cnt = np.zeros(ncell, dtype=np.int64)
    for n in rng.permutation(wk.size):
        cnt[wi[n] * K + wk[n]] += 1
        cnt[wj[n] * K + wk[n]] += 1
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    cur = ptr[:-1].copy()
    ent = np.full(2 * wk.size, -1, dtype=np.int64)
    for n in rng.permutation(wk.size):
        for side, ag in ((0, wi[n]), (1, wj[n])):
            c = ag * K + wk[n]
            ent[cur[c]] = 2 * n + side
            cur[c] += 1
    for c in range(ncell):
        ent[ptr[c]:ptr[c + 1]] = insertion_sort(ent[ptr[c]:ptr[c + 1]])
    return ptr, ent


def kernel_build(N, K, per, block, wk, wi, wj, rng):
    """build_entry_tables as one workgroup runs it: block counters, own hits appended in an arbitrary order, scan, scatter
    (the cursors in an arbitrary order), insertion sort per cell: (cptr, codes, entry count of every block)"""
    a0, a1 = block * per, min(block * per + per, N)
    ncell = (a1 - a0) * K
    blk = np.zeros((N + per - 1) // per, dtype=np.int64)
    cnt = np.zeros(ncell + 1, dtype=np.int64)
    hits = []
    for n in rng.permutation(wk.size):
        for side, ag in ((0, wi[n]), (1, wj[n])):
            blk[ag // per] += 1
            if ag // per == block:
                cell = (ag - a0) * K + wk[n]
                cnt[cell] += 1
                hits.append((2 * n + side, cell))
    cptr = np.concatenate([[0], np.cumsum(cnt[:ncell])])
    cur = np.zeros(ncell, dtype=np.int64)
    codes = np.full(len(hits), -1, dtype=np.int64)
    for t in rng.permutation(len(hits)):
        code, cell = hits[t]
        codes[cptr[cell] + cur[cell]] = code
        cur[cell] += 1
    for c in range(ncell):
        codes[cptr[c]:cptr[c + 1]] = insertion_sort(codes[cptr[c]:cptr[c + 1]])
    return cptr, codes, blk


# ---- the checks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.scen.label)
def test_working_sets_are_what_the_table_states(case):
    prob, _, _, _, _, W = pc.setup(case.scen)
    wk, wi, wj = rows_of(prob, W)
    cnt = cell_stats(prob.K, prob.N, wk, wi, wj)
    assert (W.size, cnt.max()) == (case.rows, case.max_cell)
    if case.cells_ge3 >= 0:
        same = (wi // 8) == (wj // 8)
        assert (int((cnt >= 3).sum()), int(same.sum()), int((~same).sum())) == (case.cells_ge3, case.inside8, case.across8)
        assert tuple(block_counts(prob.N, 8, wi, wj)) == case.per_block8
    for kernel in case.kernels:
        per = pc.apb(kernel, prob.D)
        assert block_counts(prob.N, per, wi, wj).max() <= pc.entry_cap(kernel, prob.N, prob.K, prob.D)
        for label, batches in working_sets(case):
            k2, i2, j2 = rows_of(prob, np.concatenate(batches))
            assert_inputs_detect_order(prob.K, prob.N, k2, i2, j2, per)
            if label.startswith("no-rows") and per <= 8:  # a block without any incident row
                assert block_counts(prob.N, per, i2, j2)[8 // per] == 0
            if label == "high-ids-first":
                assert np.any(np.diff(np.concatenate(batches)) < 0)


def test_overflow_set_is_beyond_every_capacity():
    prob = pc.make_problem(OVERFLOW)
    assert prob.m_col == 6000
    wk, wi, wj = rows_of(prob, np.arange(prob.m_col))
    for kernel, worst in ((4, 6000), (3, 6000), (2, 12000)):
        per = pc.apb(kernel, 2)
        assert block_counts(prob.N, per, wi, wj).max() == worst > 4 * pc.entry_cap(kernel, prob.N, prob.K, 2)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.scen.label)
def test_expected_tables_equal_both_host_builds(case):
    prob, _, _, _, _, _ = pc.setup(case.scen)
    N, K = prob.N, prob.K
    rng = np.random.default_rng(7)
    for label, batches in working_sets(case):
        wk, wi, wj = rows_of(prob, np.concatenate(batches))
        ptr, ent = global_build(N, K, wk, wi, wj, rng)
        assert ptr[-1] == 2 * wk.size and np.array_equal(np.sort(ent), np.arange(2 * wk.size))
        for per in sorted({pc.apb(kernel, prob.D) for kernel in case.kernels}):
            counts = block_counts(N, per, wi, wj)
            for b in range((N + per - 1) // per):
                a0, a1 = b * per, min(b * per + per, N)
                cptr, codes = expected_tables(K, wk, wi, wj, a0, a1)
                what = (case.scen.label, label, per, b)
                # the slice of the global lists the kernels copy when the host builds them
                e0, e1 = ptr[a0 * K], ptr[a1 * K]
                assert np.array_equal(cptr, ptr[a0 * K:a1 * K + 1] - e0), what
                assert np.array_equal(codes, ent[e0:e1]), what
                # the in-kernel build
                cptr_k, codes_k, blk = kernel_build(N, K, per, b, wk, wi, wj, rng)
                assert np.array_equal(cptr, cptr_k) and np.array_equal(codes, codes_k), what
                assert np.array_equal(blk, counts) and codes.size == counts[b], what
