"""Fleet-level steps around the solve (not in the reference): goal assignment for interchangeable
vehicles, repair of between-sample conflicts by holds, staggered starts.  FleetMethods is a state-free base of solvers.scp.SCP.
It reads ``N``, ``K``, ``D``, ``h``, ``R``, ``convergence_tolerance``, ``initial_positions``, ``_obstacles``, ``_pairs``,
``_last_qp_info``, ``_metric`` and ``_ctx`` and calls ``_require`` / ``_device_trajectories`` / ``_lattice_edges`` / ``_states`` / ``_limits`` /
``_space`` / ``_ensure_qp`` / ``_apply_boxes`` / ``_solve_with_avoidance_constraints`` / ``_kinematics``; it writes
``final_positions`` / ``final_velocities``, ``_final_given``, ``goal_assignment``, ``assignment_info``, ``_dev`` (assign_goals),
``trajectories``, ``_holds``, ``_rho_start``, ``last_info["repair"]`` (repair_conflicts), ``staggered``, ``last_info["stagger"]``
(stagger_starts)."""
import time

import numpy as np

from .. import _hip
from ._obstacles import whole_number
from .stagger import candidate_orders, refined_orders, schedule_key, staggered_fleet


class FleetMethods:
    def assign_goals(self, min_sep=None, method="auto", cost="line", stride=None, clearance=0, power=2,
                     allow_unreachable=False):
        """Interchangeable vehicles: re-pair vehicles and goals so that the sum of squared start-goal distances is minimal
        (scp_assign_goals).  Call it after set_initial_states and set_final_states; the final positions AND velocities are
        permuted, so vehicle i then flies to the goal given as number ``goal_assignment[i]``.  ``goal_assignment`` always
        refers to the order handed to set_final_states: a second call recomputes from those originals, it does not compose.
        ``assignment_info`` holds the auction's statistics and the straight-line checks before / after (min_sep, default the
        minimum distance, is their "close" threshold).  ``method``: "single" (scp_assign_goals, up to 4096 vehicles), "wide"
        (scp_assign_goals_wide, up to 65536) or "auto" (wide from 1024 vehicles, where it is faster); the result does not
        depend on it.

        ``cost``: "line" pairs by squared straight-line distance, which does not see walls; "path" (after set_obstacles) by
        the number of moves of find_reference's lattice search between every start and every goal (scp_lattice_distances on
        the lattice of ``stride`` / ``clearance``, the edge masks shared with find_reference), raised to ``power`` (1 or 2),
        the straight-line distance only breaking ties (scenarios.assignment.path_costs), through the same auction on that
        matrix (scp_assign_costs; up to 4096 vehicles, ``method`` is not used).  ``assignment_info`` then also holds
        ``hops_identity`` / ``hops_assigned`` ({"sum", "max"} over the pairs that have a path), ``n_unreachable_identity`` /
        ``n_unreachable_assigned``, ``tie_bits``, ``unreachable_cost``, ``max_hops``, ``stride``, ``clearance``, ``lattice``
        and the device milliseconds ``edges_ms``, ``distances_ms``, ``assign_ms``.  If even the best pairing leaves a vehicle
        without a path, no pairing connects every vehicle: ValueError naming one, unless ``allow_unreachable``.

        ``cost="length"`` pairs by the weighted length of the paths between every start and every goal (scp_lattice_costs: a
        diagonal move costs more than a straight one, with the node penalties of set_search_metric's ``keep_clear`` /
        ``clear_weight``; the setting's metric itself is not consulted), raised to ``power`` and shifted right until it fits 31 bits (scenarios.assignment.length_costs; no tie bits: length already separates what equal hop
        counts lump together), through the same auction.  ``assignment_info`` then holds ``length_identity`` /
        ``length_assigned`` ({"sum", "max"} of the lattice costs over the pairs that have a path), the unreachable counts,
        ``shift``, ``unreachable_cost``, ``max_cost``, ``keep_clear``, ``stride``, ``clearance``, ``lattice`` and the device
        milliseconds ``edges_ms``, ``penalties_ms``, ``distances_ms``, ``assign_ms``.

        Returns goal_assignment."""
        from ..scenarios.assignment import (COST_UNREACHED, _ASSIGN_KEYS, _LINE_KEYS, assign_method, hop_totals, length_costs,
                                            length_totals, path_costs)
        if cost not in ("line", "path", "length"):
            raise ValueError(f"cost={cost!r}: \"line\", \"path\" or \"length\"")
        _, prefer, weight = self._metric
        if cost != "line":
            if self.N > _hip.ASSIGN_COSTS_MAX_N:
                raise ValueError(f"assign_goals(cost=\"{cost}\") supports up to {_hip.ASSIGN_COSTS_MAX_N} vehicles (one N x N cost "
                                 f"matrix in one workgroup), not {self.N}; cost=\"line\" goes up to 65536")
            stride, clearance, lattice, edges, edges_ms = self._lattice_edges(f"assign_goals(cost=\"{cost}\")", stride, clearance)
        else:
            assign = assign_method(self._ctx, method, self.N)
        self._require("assign_goals", states=True)
        if self._final_given is None:
            self._final_given = (self.final_positions.copy(), self.final_velocities.copy())
        pf, vf = (a.reshape(self.N, self.D) for a in self._final_given)
        start = self.initial_positions.reshape(1, self.N, self.D)
        sep = float(self.R if min_sep is None else min_sep)
        if cost == "path":
            c, s0 = self._ctx, start[0]
            hops, _, _, _ = c.lattice_distances(self.D, self._obstacles.grid, stride, edges, c.tensor(s0), c.tensor(pf))
            distances_ms = c.last_pair_ms()
            hops = hops.cpu().numpy().view(np.uint16)
            diff = s0[:, None, :] - pf[None, :, :]
            costs, how = path_costs(hops, (diff * diff).sum(-1), power)
            goal_of, st, _ = c.assign_costs(costs[None])
            assign_ms = c.last_pair_ms()
        elif cost == "length":
            c, s0 = self._ctx, start[0]
            pen, penalties_ms = self._obstacles.penalties(stride, prefer, weight) if prefer > 0 and weight > 0 else (None, 0.0)
            lengths, _, _, _ = c.lattice_costs(self.D, self._obstacles.grid, stride, edges, c.tensor(s0), c.tensor(pf), pen=pen)
            distances_ms = c.last_pair_ms()
            lengths = lengths.cpu().numpy().view(np.uint32)
            costs, how = length_costs(lengths, power)
            goal_of, st, _ = c.assign_costs(costs[None])
            assign_ms = c.last_pair_ms()
        else:
            goal_of, st, _ = assign(start, pf[None])
        before = self._ctx.straight_line_check(start, pf[None], None, sep)
        after = self._ctx.straight_line_check(start, pf[None], goal_of, sep)
        info = {k: st[k][0].item() for k in _ASSIGN_KEYS}
        info["line_before"] = {k: before[k][0].item() for k in _LINE_KEYS}
        info["line_after"] = {k: after[k][0].item() for k in _LINE_KEYS}
        perm = goal_of[0].cpu().numpy().astype(np.int64)
        if cost == "path":
            hi, ha = hop_totals(hops), hop_totals(hops, perm)
            info.update(how, hops_identity={k: hi[k] for k in ("sum", "max")}, hops_assigned={k: ha[k] for k in ("sum", "max")},
                        n_unreachable_identity=hi["n_unreachable"], n_unreachable_assigned=ha["n_unreachable"], stride=stride,
                        clearance=clearance, lattice=lattice[:self.D], edges_ms=edges_ms, distances_ms=distances_ms,
                        assign_ms=assign_ms)
            if ha["n_unreachable"] and not allow_unreachable:
                i = int(np.flatnonzero(hops[np.arange(self.N), perm] == 0xFFFF)[0])
                raise ValueError(f"assign_goals(cost=\"path\"): no pairing connects every vehicle -- in the best one "
                                 f"{ha['n_unreachable']} vehicles have no path, vehicle {i} among them (stride {stride}, "
                                 f"clearance {clearance}, lattice {lattice[:self.D]}); allow_unreachable=True pairs the rest")
        if cost == "length":
            li, la = length_totals(lengths), length_totals(lengths, perm)
            info.update(how, length_identity={k: li[k] for k in ("sum", "max")}, length_assigned={k: la[k] for k in ("sum", "max")},
                        n_unreachable_identity=li["n_unreachable"], n_unreachable_assigned=la["n_unreachable"], stride=stride,
                        clearance=clearance, lattice=lattice[:self.D], keep_clear=prefer, edges_ms=edges_ms,
                        penalties_ms=penalties_ms, distances_ms=distances_ms, assign_ms=assign_ms)
            if la["n_unreachable"] and not allow_unreachable:
                i = int(np.flatnonzero(lengths[np.arange(self.N), perm] == COST_UNREACHED)[0])
                raise ValueError(f"assign_goals(cost=\"length\"): no pairing connects every vehicle -- in the best one "
                                 f"{la['n_unreachable']} vehicles have no path, vehicle {i} among them (stride {stride}, "
                                 f"clearance {clearance}, lattice {lattice[:self.D]}); allow_unreachable=True pairs the rest")
        self.final_positions = pf[perm].flatten()
        self.final_velocities = vf[perm].flatten()
        self._dev.pop("p0", None)
        self.trajectories = None
        self.goal_assignment = perm
        self.assignment_info = info
        return perm

    def repair_conflicts(self, max_passes=6, pad=0.02, max_iterations=15):
        """Remove the between-sample conflicts of the stored trajectories (what validate_solution(continuous=True,
        conflicts=True) lists) by HOLDS: for every conflicting segment the two collision rows at its ends are replaced by one
        fixed half-plane eta . (p_i - p_j) >= R + margin, eta the direction of the closest approach, which keeps the pair
        apart over the whole segment (include/scp_hip.h, scp_update_holds).  A PASS lists the conflicts, updates the table
        of holds (a conflict that persists raises its margin by its shortfall + pad), re-runs the SCP loop from the stored
        accelerations (at most max_iterations iterations, to the usual relative-step tolerance) and lists again.  Passes
        repeat until no conflict is left, max_passes have run, or a QP of the pass ends with a status other than solved /
        solved inaccurate -- then the trajectories from before that pass are kept.

        Always the Python-driven, row-writing loop (the planes of all rows, 24 B per row, are allocated), whatever `native` /
        `row_free` say; one rank only.  ``self.trajectories`` becomes the last accepted pass.  Returns (and stores in
        ``last_info["repair"]``) a dictionary: ``conflicts_before`` and ``conflicts_per_pass`` (violating segments, the records
        of scp_list_conflicts), ``passes``, ``holds``, ``repaired`` (no conflict left), ``stopped_by`` ("clean", "max_passes"
        or "qp_status"), ``cost_ratio`` (sum of squared accelerations after / before), ``time_sec``; per pass also
        ``iterations_per_pass``, ``admm_steps_per_pass``, ``update_holds_ms`` and ``apply_holds_ms`` (device time of the
        table update and of the pass's last plane overwrite).  Without a conflict it returns at once with passes = 0 and
        leaves the trajectories untouched."""
        self._require("repair_conflicts", trajectories=True)  # (asked before the ranks, unlike the obstacle calls)
        self._require("repair_conflicts", one_rank=True)
        t_start = time.perf_counter()
        N, K, D, h, c = self.N, self.K, self.D, self.h, self._ctx
        p0, v0, pf, vf = self._states()
        dev = self._device_trajectories()
        acc = dev[2]
        cost_before = float(np.sum(self.trajectories["accelerations"] ** 2))
        found = c.list_conflicts(N, K, D, h, self.R, *dev)
        info = {"conflicts_before": int(found.size), "conflicts_per_pass": [], "passes": 0, "holds": 0, "repaired": found.size == 0,
                "stopped_by": "clean" if found.size == 0 else "max_passes", "cost_ratio": 1.0, "iterations_per_pass": [],
                "admm_steps_per_pass": [], "update_holds_ms": [], "apply_holds_ms": []}
        if found.size and max_passes > 0:
            self._ensure_qp().set_problem(self._limits(), self._space(), p0, v0, pf, vf)
            self._apply_boxes(self._qp)
            self._rho_start = 0.0
            table, n_holds = c.hold_table(capacity=max(1024, 4 * found.size))
        try:
            while found.size and info["passes"] < max_passes:
                table, n_holds, info["holds"] = c.update_holds(N, K, D, h, self.R, *dev, found, table, n_holds, pad)
                info["update_holds_ms"].append(c.last_pair_ms())
                self._holds = (table, n_holds)
                x, iterations, steps, ok = acc, 0, 0, True
                while iterations < max_iterations:
                    new = self._solve_with_avoidance_constraints(x)
                    iterations += 1
                    steps += int(self._last_qp_info["iter"])
                    ok = self._last_qp_info["status_val"] in (1, 2)
                    if not ok:
                        break
                    _, _, rel = c.rel_step(new, x)
                    x = new
                    if rel <= self.convergence_tolerance:
                        break
                info["passes"] += 1
                info["iterations_per_pass"].append(iterations)
                info["admm_steps_per_pass"].append(steps)
                info["apply_holds_ms"].append(float(self._pairs.last_holds_ms))
                if not ok:
                    info["stopped_by"] = "qp_status"
                    break
                pos, vel = self._kinematics(x)
                acc, dev = x, (pos, vel, x)
                found = c.list_conflicts(N, K, D, h, self.R, *dev)
                info["conflicts_per_pass"].append(int(found.size))
                self.trajectories = {"positions": pos.cpu().numpy(), "velocities": vel.cpu().numpy(),
                                     "accelerations": x.cpu().numpy()}
                if found.size == 0:
                    info["repaired"], info["stopped_by"] = True, "clean"
        finally:
            self._holds = None
        info["cost_ratio"] = float(np.sum(self.trajectories["accelerations"] ** 2)) / cost_before if cost_before > 0 else 1.0
        info["time_sec"] = time.perf_counter() - t_start
        self.last_info["repair"] = info
        return info

    def stagger_starts(self, max_delay, order=None, *, search=0, rounds=1, seed=0, objective="makespan"):
        """Remove the between-sample conflicts of the stored trajectories WITHOUT changing a plan: some vehicles start a few
        whole steps later, at most ``max_delay`` (an int in [0, min(K, 63)]).  One device pass computes, for every ordered pair
        and every lag, whether the pair conflicts when the first vehicle starts that many steps after the second
        (scp_lag_conflicts); a greedy schedule then takes the vehicles in ``order`` (a permutation of 0 .. N-1; None: by
        index) and gives each the smallest delay that conflicts with nobody placed before it (scp_schedule_starts), -1 if
        there is none -- such a vehicle is unplaced, flies undelayed and is reported.  No QP is solved, so this also serves
        plans of ``generate_trajectories(max_iterations=0)`` and fleets whose joint QP fails.  One rank only.

        ``self.trajectories`` is left untouched; the staggered fleet -- arrays (N, K + Dmax, D), Dmax the largest delay, every
        vehicle held at its start before it leaves and parked at its goal after it has arrived -- is stored as
        ``self.staggered`` ({"positions", "velocities", "accelerations", "delays"}) and judged by the continuous-time check.
        Returns (and stores in ``last_info["stagger"]``) a dictionary: ``delays`` (int array, -1: unplaced), ``scheduled`` (every
        vehicle placed), ``n_delayed``, ``n_unplaced``, ``max_delay``, ``total_delay``, ``conflicts_before`` /
        ``conflicts_after`` (violating segments of the stored and of the staggered fleet, scp_check_separation),
        ``min_distance_after``, ``horizon_steps`` (K + Dmax), ``lag_conflicts_ms`` / ``schedule_ms`` (device time of the two
        calls) and ``time_sec``.

        The greedy schedule depends on the order it takes the vehicles in.  ``search=B`` (an int in [1, 65535]; 0: the one order
        above) schedules B candidate orders per round in one launch each (scp_schedule_starts_batch) and keeps the best under
        ``objective`` -- "makespan": fewest unplaced vehicles, then the smallest largest delay, then the smallest total delay;
        "total": fewest unplaced, then total, then largest.  Round 0 takes ``candidate_orders(N, B, default_rng(seed),
        base=order)``, every later one of ``rounds`` takes ``refined_orders`` of the best so far; a later round replaces the
        best only by a strictly smaller key, and the search stops when nobody is unplaced or delayed.  Candidate 0 of round 0 is
        ``order`` itself, so the result is never worse than without the search.  The masks are computed once.  The info then
        also has ``search``: ``candidates``, ``rounds_run``, ``best_round``, ``best_candidate``, ``best_order``, ``baseline``
        (``n_unplaced`` / ``max_delay`` / ``total_delay`` / ``n_delayed`` of ``order``), ``improved`` and ``objective``;
        ``schedule_ms`` is the sum over the rounds."""
        self._require("stagger_starts", trajectories=True)  # (asked before the ranks, unlike the obstacle calls)
        self._require("stagger_starts", one_rank=True)
        top = min(self.K, _hip.MAX_LAG)
        whole_number(max_delay, 0, top,
                     f"max_delay={max_delay!r}: the largest delay is a whole number of steps in [0, min(K, 63) = {top}]")
        if self.N > _hip.SCHEDULE_MAX_N:
            raise ValueError(f"stagger_starts schedules at most {_hip.SCHEDULE_MAX_N} vehicles")
        if order is not None:
            order = np.asarray(order, dtype=np.int64).reshape(-1)
            if order.size != self.N or not np.array_equal(np.sort(order), np.arange(self.N)):
                raise ValueError("order must be a permutation of 0 .. N-1")
        whole_number(search, 0, _hip.SCHEDULE_MAX_BATCH,
                     f"search={search!r}: the candidate orders per round are an int in [0, {_hip.SCHEDULE_MAX_BATCH}]")
        whole_number(rounds, 1, None, f"rounds={rounds!r}: an int >= 1")
        if objective not in _hip.SCHEDULE_OBJECTIVES:
            raise ValueError(f"objective={objective!r}: one of {sorted(_hip.SCHEDULE_OBJECTIVES)}")
        t_start = time.perf_counter()
        N, K, D, h, c = self.N, self.K, self.D, self.h, self._ctx
        S = int(max_delay)
        dev = self._device_trajectories()
        before = c.check_separation(N, K, D, h, self.R, *dev)
        mask = c.lag_conflicts(N, K, D, h, self.R, *dev, S, device=True)
        lag_ms = c.last_pair_ms()
        if search:
            delays, st, schedule_ms, found = self._search_start_orders(mask, S, order, int(search), int(rounds), seed, objective)
        else:
            delays, st = c.schedule_starts(mask, S, order)
            schedule_ms = c.last_pair_ms()
        traj = self.trajectories
        pos, vel, acc = staggered_fleet(traj["positions"], traj["velocities"], traj["accelerations"], h, delays)
        horizon = pos.shape[1]
        after = c.check_separation(N, horizon, D, h, self.R, c.tensor(pos), c.tensor(vel), c.tensor(acc))
        self.staggered = {"positions": pos, "velocities": vel, "accelerations": acc, "delays": delays.astype(np.int64)}
        info = {"delays": delays.astype(np.int64), "scheduled": st["n_unplaced"] == 0, "n_delayed": st["n_delayed"],
                "n_unplaced": st["n_unplaced"], "max_delay": st["max_delay"], "total_delay": st["total_delay"],
                "conflicts_before": int(before["n_violating"]), "conflicts_after": int(after["n_violating"]),
                "min_distance_after": float(after["min_dist"]), "horizon_steps": int(horizon), "lag_conflicts_ms": lag_ms,
                "schedule_ms": schedule_ms, "time_sec": time.perf_counter() - t_start}
        if search:
            info["search"] = found
        self.last_info["stagger"] = info
        return info

    def _search_start_orders(self, mask, S, order, B, rounds, seed, objective):
        """the order search of stagger_starts on the device masks: (delays, stats, device ms, the info's "search" entry)"""
        c, N = self._ctx, self.N
        rng = np.random.default_rng(seed)
        fields = ("n_delayed", "n_unplaced", "max_delay", "first_unplaced", "total_delay")
        best = None  # (key, order, delays, stats, round, candidate)
        ms = 0.0
        for r in range(rounds):
            orders = candidate_orders(N, B, rng, base=order) if r == 0 else refined_orders(best[1], best[2], B, rng)
            delays, stats, b = c.schedule_starts_batch(mask, S, orders, objective)
            ms += c.last_pair_ms()
            st = {f: int(stats[f][b]) for f in fields}
            key = schedule_key(st["n_unplaced"], st["max_delay"], st["total_delay"], objective)
            if r == 0:
                baseline = {f: int(stats[f][0]) for f in ("n_unplaced", "max_delay", "total_delay", "n_delayed")}
                base_key = schedule_key(baseline["n_unplaced"], baseline["max_delay"], baseline["total_delay"], objective)
            if best is None or key < best[0]:
                best = (key, orders[b].copy(), delays[b].copy(), st, r, b)
            if best[0] == (0, 0, 0):
                break
        found = {"candidates": B, "rounds_run": r + 1, "best_round": best[4], "best_candidate": best[5],
                 "best_order": best[1].astype(np.int64), "baseline": baseline, "improved": best[0] < base_key,
                 "objective": objective}
        return best[2], best[3], ms, found
