"""Working sets for the r phase's gather g = sum_e c_e g_e of the lean persistent ADMM kernels (csrc/scp_qp_persist16.hip),
the per-cell loop over the rows incident to a cell (agent, time step).  A gather that keeps the loads of U entries in
flight per wait -- indices past the cell's end clamped into it, their contributions masked -- can go wrong only by the
number of rows of a cell: none (no trip), 1 (U - 1 masked slots), U (a full trip, nothing masked), U + 1 (a second trip
for one entry) and at least 2 U + 1 (three trips).  Depths U = 2, 3 and 4 were built and measured (all slower than one
entry per trip at 1024 x 50, DESIGN.md 3.3: the kernel keeps the plain loop); the table below -- modelled on
tests/persist_cases.py, chosen with the oracle -- has all five counts for each of them in every case, so that the loop as it
is and any deeper form of it meet cells of every kind.  tests/test_lean_gather_depth_gpu.py runs the table on the kernels."""
import numpy as np
import pytest

import persist_cases as pc
from oracle import qp_oracle as qo

DEPTHS = (2, 3, 4)
STEPS = (1, 2, 7)  # the first step, a plain one, the step after a check (pc.CHECK = 6)

# (scenario with the working-set margin, kernels): a tight crossing on a circle in 2-D, a jittered lattice in 3-D
TABLE = [
    (pc.Scenario("circle", 17, 17, 17, 2, 2.0), (3, 2)),
    (pc.Scenario("circle", 2, 13, 16, 2, 3.0), (3, 2)),
    (pc.Scenario("near", 3103, 17, 17, 3, 0.6), (3,)),
]
CASES = [pc.Case(sc, kern, sc.N % pc.apb(kern, sc.dim), sc.K % 16, STEPS) for sc, kerns in TABLE for kern in kerns]


def incident_rows(prob, W):
    """[N][K] rows of the working set at every cell (a row joins two agents: it counts at both)"""
    k, i, j = qo.working_rows(prob, np.asarray(W, dtype=np.int64))
    cnt = np.zeros((prob.N, prob.K), dtype=np.int64)
    np.add.at(cnt, (i, k), 1)
    np.add.at(cnt, (j, k), 1)
    return cnt


def test_table_shape():
    assert {(c.scen.dim, c.kernel) for c in CASES} == {(2, 3), (2, 2), (3, 3)}
    assert sum(c.scen.dim == 3 for c in CASES) == 1
    for c in CASES:
        assert c.scen.K <= 17 and (c.scen.dim == 3 or c.scen.N <= 17), c.id


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_cells_with_0_1_U_U1_and_2U1_rows(case):
    """... and every block of agents within the kernel's LDS entry capacity (else: EXIT_OVERFLOW, three-launch pipeline)"""
    sc = case.scen
    prob, x0, eta, l_col, dist, W = pc.setup(sc)
    assert (prob.N, prob.K, prob.D) == (sc.N, sc.K, sc.dim)
    cnt = incident_rows(prob, W)
    assert cnt.sum() == 2 * W.size
    have = set(np.unique(cnt).tolist())
    for U in DEPTHS:
        assert {0, 1, U, U + 1} <= have, (case.id, U, sorted(have))
        assert cnt.max() >= 2 * U + 1, (case.id, U, int(cnt.max()))
    per = pc.apb(case.kernel, sc.dim)
    assert pc.block_entries(prob, W, per).max() <= pc.entry_cap(case.kernel, sc.N, sc.K, sc.dim), case.id
