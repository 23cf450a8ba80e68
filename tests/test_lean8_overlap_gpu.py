"""The bench-shaped problem (1024 agents x 50 steps, 2-D, grid-swap seed 1 024 000) on the lean 8-agent kernel with S0 p = T r
on its idle matrix waves: the QP of the first SCP iteration runs on that kernel alone, never gives up or overflows, and takes
the ADMM steps, working rows and rounds that the build before this change recorded (bench.py's cpu_baseline.sample: 230
iterations, 12 583 rows, 2 rounds)."""
import pytest
import torch

from path_planning.scenarios.position_generator import generate_grid_swap
from path_planning.solvers.scp import SCP


@pytest.mark.gpu
def test_bench_shape_runs_on_the_lean8_kernel_with_the_recorded_counts():
    N, K, D, h, R = 1024, 50, 2, 0.2, 0.8
    p0, pf, space = generate_grid_swap(N, seed=1000 * N, dim=D)
    solver = SCP(N, K * h + 1e-9, h, R, space, dim=D, device=0, verbose=False)
    assert solver.K == K
    solver.set_initial_states(p0)
    solver.set_final_states(pf)
    solver._precompute_constraint_matrices()
    acc0 = solver._solve_initial_trajectory()
    _, info = solver.scp_iteration(acc0)
    torch.cuda.synchronize()
    assert info["pipeline"] == "persistent8-lean", info  # no EXIT_OVERFLOW, no three-launch fallback
    assert info["persist_gave_up"] == 0, info
    assert info["status"] == "solved", info
    assert (info["iter"], info["working_rows"], info["rounds"]) == (230, 12583, 2), info
