"""Goal assignment for interchangeable vehicles (scp_assign_goals): which vehicle flies to which goal.

The planner takes "vehicle i flies to goal i" as given; for a fleet whose vehicles are interchangeable the pairing is free.
The assignment that minimises the sum of squared start-goal distances has (s_i - s_j).(g_i - g_j) >= 0 for every pair, so no
two equal-time straight-line motions are opposed and none come closer than min(|s_i - s_j|, |g_i - g_j|) / sqrt(2): head-on
swaps, the instances on which the first linearised QP of the SCP is infeasible, cannot occur.  The auction runs on the GPU,
one workgroup per scenario or, for large single scenarios, on the whole chip (scp_assign_goals_wide; include/scp_hip.h
states the rule, both forms write the same bytes); there is no CPU path: without a GPU these functions raise
``_hip.HipError`` like ``SCP``.
"""
import numpy as np

from .grid_swap_device import _context

_ASSIGN_KEYS = ("cost_q", "cost_q_identity", "quantum", "rounds", "bids", "phases", "status")
_LINE_KEYS = ("min_approach", "arg_i", "arg_j", "n_close", "n_opposed")

METHODS = ("auto", "single", "wide")
SINGLE_MAX_N = 4096  # scp_assign_goals keeps a scenario's whole state in one workgroup's LDS
# Up to 4096 vehicles "auto" takes the wide form where profiles/assign_wide_times.txt shows it faster: a single scenario
# (B = 1) of 1024 vehicles or more (uniform points 43.8 against 56.9 ms at 1024 and 0.56 against 1.52 s at 4096; grid-swap
# 1.4 against 7.6 ms and 2.1 against 112 ms).  At N = 128 the one-workgroup form is faster alone (4.8 against 7.0 ms) and in
# a batch of 4096 (16.4 against 26.8 ms); nothing between those shapes was measured, so nothing between them moves.
AUTO_WIDE_MIN_N = 1024
AUTO_WIDE_MAX_B = 1


def assign_method(ctx, method, N, B=1):
    """The bound call of ``ctx`` behind ``method`` for B scenarios of N vehicles: "single" is scp_assign_goals (one workgroup
    per scenario, N <= 4096), "wide" scp_assign_goals_wide (N <= 65536), "auto" is wide beyond 4096 vehicles and, up to
    there, for a single scenario of at least AUTO_WIDE_MIN_N vehicles.  Both write the same bytes, so the choice never shows
    in a result."""
    if method not in METHODS:
        raise ValueError(f"method {method!r}: need one of {METHODS}")
    if method == "wide" or (method == "auto" and (N > SINGLE_MAX_N or (N >= AUTO_WIDE_MIN_N and B <= AUTO_WIDE_MAX_B))):
        return ctx.assign_goals_wide
    return ctx.assign_goals


def assign_goals_batch(init, goal, device=0, min_sep=0.0, max_rounds_per_phase=0, method="auto"):
    """B scenarios in one call.  init / goal: (B, N, D) arrays or device tensors.  method: see assign_method.

    Returns (goal_of, info): goal_of (B, N) int32 device tensor -- vehicle i of scenario b flies to ``goal[b, goal_of[b, i]]``
    -- and info, a dict of numpy arrays of length B: ``cost_q`` / ``cost_q_identity`` (sum of the quantised squared
    distances with the assignment / with the given pairing; times ``quantum`` they are m^2), ``rounds``, ``bids``, ``phases``,
    ``status`` (0 ok, 1: the round limit was hit and goal_of is the identity), and ``line_before`` / ``line_after``: dicts of
    the straight-line check (``min_approach``, ``arg_i``, ``arg_j``, ``n_close`` = pairs closer than min_sep, ``n_opposed``)
    with the given pairing and with the assignment."""
    ctx = _context(device)
    start, target = ctx._scenario_points(init, goal)
    assign = assign_method(ctx, method, int(start.shape[1]), int(start.shape[0]))
    goal_of, st, _ = assign(start, target, max_rounds_per_phase=max_rounds_per_phase)
    before = ctx.straight_line_check(start, target, None, min_sep)
    after = ctx.straight_line_check(start, target, goal_of, min_sep)
    info = {k: st[k].copy() for k in _ASSIGN_KEYS}
    info["line_before"] = {k: before[k].copy() for k in _LINE_KEYS}
    info["line_after"] = {k: after[k].copy() for k in _LINE_KEYS}
    return goal_of, info


def assign_goals(init, goal, device=0, min_sep=0.0, max_rounds_per_phase=0, method="auto"):
    """One scenario: init / goal (N, D).  Returns (goal_of, info): goal_of a numpy int array of length N (vehicle i flies to
    ``goal[goal_of[i]]``), info as assign_goals_batch's with scalars in place of the arrays."""
    init, goal = np.asarray(init, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    if init.ndim != 2 or init.shape != goal.shape:
        raise ValueError(f"init {init.shape} and goal {goal.shape} must both be (N, D)")
    goal_of, info = assign_goals_batch(init[None], goal[None], device=device, min_sep=min_sep,
                                       max_rounds_per_phase=max_rounds_per_phase, method=method)
    one = {k: (v[0].item() if isinstance(v, np.ndarray) else {kk: vv[0].item() for kk, vv in v.items()})
           for k, v in info.items()}
    return goal_of[0].cpu().numpy().astype(np.int64), one


def describe(info):
    """one line for the CLIs: cost (m^2), straight-line closest approach and opposed pairs, before -> after"""
    q, lb, la = info["quantum"], info["line_before"], info["line_after"]
    note = "" if info["status"] == 0 else " [round limit: pairing kept]"
    return (f"Goal assignment: cost {info['cost_q_identity'] * q:.3f} -> {info['cost_q'] * q:.3f} m^2, straight-line minimum "
            f"approach {lb['min_approach']:.4f} -> {la['min_approach']:.4f} m, opposed pairs {lb['n_opposed']} -> "
            f"{la['n_opposed']} ({info['phases']} phases, {info['rounds']} rounds){note}")
