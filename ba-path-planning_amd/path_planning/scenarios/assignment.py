"""Goal assignment for interchangeable vehicles (scp_assign_goals): which vehicle flies to which goal.

The planner takes "vehicle i flies to goal i" as given; for a fleet whose vehicles are interchangeable the pairing is free.
The assignment that minimises the sum of squared start-goal distances has (s_i - s_j).(g_i - g_j) >= 0 for every pair, so no
two equal-time straight-line motions are opposed and none come closer than min(|s_i - s_j|, |g_i - g_j|) / sqrt(2): head-on
swaps, the instances on which the first linearised QP of the SCP is infeasible, cannot occur.  The auction runs on the GPU,
one workgroup per scenario or, for large single scenarios, on the whole chip (scp_assign_goals_wide; include/scp_hip.h
states the rule, both forms write the same bytes); there is no CPU path: without a GPU these functions raise
``_hip.HipError`` like ``SCP``.

Straight-line distance does not see walls.  assign_goals_costs runs the same auction on a matrix of the caller's own costs
(scp_assign_costs), and path_costs builds such a matrix from the hop counts of the lattice search (scp_lattice_distances):
SCP.assign_goals(cost="path") joins the two.
"""
import numpy as np

from .. import _hip
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


HOPS_UNREACHED = 0xFFFF  # scp_lattice_distances: no path between the two nodes, or a point without a node
MAX_COST = 2 ** 31 - 1   # SCP_ASSIGN_MAX_COST
MAX_TIE_BITS = 12


def path_costs(hops, d2, power=2):
    """Costs for assign_goals_costs from the hop counts of the lattice search: hops decide, the straight-line distance only
    breaks ties among equal hops, and one unreachable pair costs more than any assignment without one.

    hops: (N, N) whole numbers, hops[i][j] lattice moves from start i to goal j, HOPS_UNREACHED (0xFFFF, or -1 as the int16
    view of it) where there is no path.  d2: (N, N) squared straight-line distances (>= 0).  power: 1 or 2 -- hops^2 prefers
    even detours to one long one, as the squared distances of assign_goals do.  numpy arrays or torch tensors.
      Hmax = the largest finite hop count;  b = the largest whole number in 0 .. 12 with N (Hmax^power + 1) 2^b <= 2^31 - 1;
      finite pairs:      c = hops^power 2^b + floor(d2 / max d2 (2^b - 1))   (the second term 0 if max d2 == 0);
      unreachable pairs: c = U = N (largest finite c) + 1   (<= 2^31 - 1 by the choice of b).
    Raises ValueError if not even b = 0 fits.  Returns (cost (N, N) int64 ndarray, {"tie_bits": b, "unreachable_cost": U,
    "max_hops": Hmax})."""
    to_numpy = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    hops, d2 = to_numpy(hops), np.asarray(to_numpy(d2), dtype=np.float64)
    if hops.dtype.kind not in "iu":
        raise ValueError(f"hops of dtype {hops.dtype}: need whole numbers")
    hops = hops.astype(np.int64) & 0xFFFF if hops.dtype.itemsize == 2 else hops.astype(np.int64)
    if hops.ndim != 2 or hops.shape[0] != hops.shape[1] or d2.shape != hops.shape:
        raise ValueError(f"hops {hops.shape} and d2 {d2.shape} must both be (N, N)")
    if isinstance(power, bool) or power not in (1, 2):
        raise ValueError(f"power={power!r}: 1 or 2")
    if ((hops < 0) | (hops > HOPS_UNREACHED)).any() or not (d2 >= 0).all():
        raise ValueError("hops must lie in [0, 0xFFFF] and d2 must be >= 0")
    N = hops.shape[0]
    finite = hops != HOPS_UNREACHED
    Hmax = int(hops[finite].max()) if finite.any() else 0
    fits = [b for b in range(MAX_TIE_BITS + 1) if N * (Hmax ** power + 1) * 2 ** b <= MAX_COST]
    if not fits:
        raise ValueError(f"path costs: {N} vehicles and paths of up to {Hmax} hops do not fit 31 bits with power={power} "
                         f"(N (Hmax^power + 1) = {N * (Hmax ** power + 1)}): use power=1 or a larger stride")
    b = fits[-1]
    top = float(d2.max()) if d2.size else 0.0
    tie = np.floor(d2 / top * float(2 ** b - 1)).astype(np.int64) if top > 0.0 else np.zeros(hops.shape, dtype=np.int64)
    cost = np.where(finite, hops, 0) ** power * 2 ** b + tie
    U = N * (int(cost[finite].max()) if finite.any() else 0) + 1
    cost = np.where(finite, cost, U)
    return cost, {"tie_bits": b, "unreachable_cost": U, "max_hops": Hmax}


COST_UNREACHED = _hip.COST_UNREACHED  # scp_lattice_costs: no path between the two nodes, or a point without a node


def length_costs(costs, power=1):
    """Costs for assign_goals_costs from the weighted lattice costs of scp_lattice_costs: length decides (it already separates
    what equal hop counts lump together, so there are no tie bits), and one unreachable pair costs more than any assignment
    without one.

    costs: (N, N) whole numbers, costs[i][j] the lattice cost from start i to goal j, COST_UNREACHED (0xFFFFFFFF, or -1 as
    the int32 view of it) where there is no path.  power: 1 or 2.  numpy arrays or torch tensors.
      Lmax = the largest finite cost;  t = the smallest shift >= 0 with N ((Lmax >> t)^power + 1) <= 2^31 - 1;
      finite pairs:      c = (L >> t)^power;
      unreachable pairs: c = U = N (largest finite c) + 1   (<= 2^31 - 1 by the choice of t).
    Returns (cost (N, N) int64 ndarray, {"shift": t, "unreachable_cost": U, "max_cost": Lmax})."""
    to_numpy = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    L = to_numpy(costs)
    if L.dtype.kind not in "iu":
        raise ValueError(f"costs of dtype {L.dtype}: need whole numbers")
    L = L.astype(np.int64) & 0xFFFFFFFF if L.dtype.itemsize == 4 else L.astype(np.int64)
    if L.ndim != 2 or L.shape[0] != L.shape[1]:
        raise ValueError(f"costs {L.shape} must be (N, N)")
    if isinstance(power, bool) or power not in (1, 2):
        raise ValueError(f"power={power!r}: 1 or 2")
    if ((L < 0) | (L > COST_UNREACHED)).any():
        raise ValueError("costs must lie in [0, 0xFFFFFFFF]")
    N = L.shape[0]
    finite = L != COST_UNREACHED
    Lmax = int(L[finite].max()) if finite.any() else 0
    t = next(t for t in range(33) if N * ((Lmax >> t) ** power + 1) <= MAX_COST)
    cost = (np.where(finite, L, 0) >> t) ** power
    U = N * (int(cost[finite].max()) if finite.any() else 0) + 1
    return np.where(finite, cost, U), {"shift": t, "unreachable_cost": U, "max_cost": Lmax}


def assign_goals_costs(cost, device=0, max_rounds_per_phase=0):
    """The assignment that minimises sum_i cost[i][goal_of[i]] for the caller's own costs (scp_assign_costs: the auction of
    assign_goals on a matrix, exact).  cost: (N, N) or (B, N, N) whole numbers in [0, 2^31 - 1], N <= 4096; cost[i][j] is what
    vehicle i pays for goal j.

    Returns (goal_of, info).  (N, N): goal_of a numpy int array of length N and info a dict of scalars -- ``cost_q`` /
    ``cost_q_identity`` (the sum with the assignment / with the given pairing), ``quantum`` (1.0), ``rounds``, ``bids``,
    ``phases``, ``status`` (0 ok, 1: the round limit was hit and goal_of is the identity), ``assign_ms`` (device
    milliseconds).  (B, N, N): goal_of a (B, N) int32 device tensor and arrays of length B (assign_ms one number)."""
    ctx = _context(device)
    single = getattr(cost, "ndim", None) == 2 or (not hasattr(cost, "ndim") and np.ndim(cost) == 2)
    goal_of, st, _ = ctx.assign_costs(cost, max_rounds_per_phase=max_rounds_per_phase)
    ms = ctx.last_pair_ms()
    if single:
        info = {k: st[k][0].item() for k in _ASSIGN_KEYS}
        info["assign_ms"] = ms
        return goal_of[0].cpu().numpy().astype(np.int64), info
    info = {k: st[k].copy() for k in _ASSIGN_KEYS}
    info["assign_ms"] = ms
    return goal_of, info


def pairing_totals(matrix, goal_of, unreached):
    """{"sum", "max", "n_unreachable"} of matrix[i][goal_of[i]] (goal_of None: the identity); sum and max over the pairs whose
    entry is not `unreached`"""
    m = np.asarray(matrix)
    h = m[np.arange(m.shape[0]), np.arange(m.shape[0]) if goal_of is None else np.asarray(goal_of)].astype(np.int64)
    ok = h != unreached
    return {"sum": int(h[ok].sum()), "max": int(h[ok].max()) if ok.any() else 0, "n_unreachable": int((~ok).sum())}


def hop_totals(hops, goal_of=None):
    """pairing_totals of the hop counts of scp_lattice_distances"""
    return pairing_totals(hops, goal_of, HOPS_UNREACHED)


def length_totals(costs, goal_of=None):
    """pairing_totals of the lattice costs of scp_lattice_costs"""
    return pairing_totals(costs, goal_of, COST_UNREACHED)


def describe(info):
    """one line for the CLIs: cost (m^2), straight-line closest approach and opposed pairs, before -> after; with path costs
    the hop totals before -> after come first"""
    q, lb, la = info["quantum"], info["line_before"], info["line_after"]
    note = "" if info["status"] == 0 else " [round limit: pairing kept]"
    if "length_assigned" in info:
        li, la_ = info["length_identity"], info["length_assigned"]
        return (f"Goal assignment by weighted path length: {li['sum']} -> {la_['sum']} in lattice costs (a straight move is 140; "
                f"largest {li['max']} -> {la_['max']}), pairs without a path {info['n_unreachable_identity']} -> "
                f"{info['n_unreachable_assigned']}, straight-line minimum approach {lb['min_approach']:.4f} -> "
                f"{la['min_approach']:.4f} m, opposed pairs {lb['n_opposed']} -> {la['n_opposed']} ({info['phases']} phases, "
                f"{info['rounds']} rounds, {info['distances_ms'] + info['assign_ms']:.3f} ms){note}")
    if "hops_assigned" in info:
        hi, ha = info["hops_identity"], info["hops_assigned"]
        return (f"Goal assignment by path length: {hi['sum']} -> {ha['sum']} lattice moves in all (longest {hi['max']} -> "
                f"{ha['max']}), pairs without a path {info['n_unreachable_identity']} -> {info['n_unreachable_assigned']}, "
                f"straight-line minimum approach {lb['min_approach']:.4f} -> {la['min_approach']:.4f} m, opposed pairs "
                f"{lb['n_opposed']} -> {la['n_opposed']} ({info['phases']} phases, {info['rounds']} rounds, "
                f"{info['distances_ms'] + info['assign_ms']:.3f} ms){note}")
    return (f"Goal assignment: cost {info['cost_q_identity'] * q:.3f} -> {info['cost_q'] * q:.3f} m^2, straight-line minimum "
            f"approach {lb['min_approach']:.4f} -> {la['min_approach']:.4f} m, opposed pairs {lb['n_opposed']} -> "
            f"{la['n_opposed']} ({info['phases']} phases, {info['rounds']} rounds){note}")
