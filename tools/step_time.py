"""Developer tool: device time per ADMM step of the joint QP for a few shapes (N, dim) -- QP#0, then one SCP iteration from
its solution through scp_solver_step; prints solve_ms / ADMM iterations of both."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ba-path-planning_amd"))
from path_planning.scenarios.position_generator import generate_grid_swap  # noqa: E402
from path_planning.solvers.scp import SCP  # noqa: E402

shapes = [(64, 2), (64, 3), (125, 3), (128, 2), (512, 2), (512, 3), (1024, 2)]
if len(sys.argv) > 1:  # NxD, NxDxP (P = settings.persistent: 2 lean 16-agent kernel, 3 lean 8-agent kernel, 0 three launches)
    # or NxDxPxK (K time steps of 0.2 s instead of 50)
    shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
for shape in shapes:
    n, dim = shape[:2]
    qp = {"persistent": shape[2]} if len(shape) > 2 else None
    p0, pf, space = generate_grid_swap(n, seed=1000 * n, dim=dim)
    s = SCP(n, shape[3] * 0.2 + 1e-9 if len(shape) > 3 else 10.0, 0.2, 0.8, space, dim=dim, verbose=False, qp_settings=qp)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s._precompute_constraint_matrices()
    for _ in range(2):
        acc0 = s._solve_initial_trajectory()
    q0 = s._last_qp_info
    print(f"N={n} D={dim} K={s.K} QP#0 [{q0['pipeline']}]: {q0['iter']} ADMM steps, solve {q0['solve_ms']:.3f} ms = "
          f"{q0['solve_ms']*1e3/max(q0['iter'],1):.2f} us/step")
    for _ in range(2):
        _, info = s.scp_iteration(acc0)
    print(f"N={n} D={dim} K={s.K} [{info['pipeline']}]: {info['iter']} ADMM steps, {info['working_rows']} rows, {info['rounds']} rounds, "
          f"solve {info['solve_ms']:.3f} ms = {info['solve_ms']*1e3/max(info['iter'],1):.2f} us/step, "
          f"iteration wall {info['time_sec']*1e3:.2f} ms")
