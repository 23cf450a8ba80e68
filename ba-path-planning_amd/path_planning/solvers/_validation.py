"""Post-solve validation: one device pass over all pairs and the fixed rows on the host copy, and what the
samples cannot show -- the continuous-time separation, its conflicts, the clearance profiles and the delay margins.
ValidationMethods is a state-free base of solvers.scp.SCP.  It reads ``N``, ``K``, ``D``, ``h``, ``R``, ``shard``, the ``*_min`` /
``*_max`` limits, ``final_positions`` / ``final_velocities``, ``trajectories``, ``_corridor`` and ``_ctx`` and calls ``_require`` /
``_device_trajectories`` / ``validate_corridor``; it writes no attribute."""
import numpy as np

from .. import _hip
from ._obstacles import whole_number
from .conflicts import conflict_windows, pair_from_index, pairs_from_index


def gather_delay_blocks(shard, mine, a0):
    """The ranks' blocks of delay margins (DELAY_DTYPE, (vehicles of the rank, S + 1), the rank's first vehicle a0) concatenated
    in vehicle order, flat: the records travel through Shard.allgather_records under the row id a (S + 1) + s, as their bytes."""
    lags = mine.shape[1]
    rec = np.empty(mine.size, dtype=[("row", np.uint64)] + _hip.DELAY_DTYPE.descr)
    rec["row"] = a0 * lags + np.arange(mine.size)
    for f in _hip.DELAY_DTYPE.names:
        rec[f] = mine.reshape(-1)[f]
    return shard.allgather_records(rec)[list(_hip.DELAY_DTYPE.names)]


def segment_min_distance(d, w, b, h):
    """Minimum over t in [0, h] of ||d + t w + t^2/2 b|| for ONE pair and segment, and the t it is attained at (host helper
    of validate_solution(continuous=True): the report's details for a row the device pass has already picked).  The squared
    distance is a quartic; its minimum is at 0, at h or at a real root of its derivative inside (0, h)."""
    d, w, b = (np.asarray(x, dtype=np.float64) for x in (d, w, b))
    c = [d @ d, 2.0 * (d @ w), w @ w + d @ b, w @ b, 0.25 * (b @ b)]
    f = lambda t: c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4])))  # noqa: E731
    cand = [0.0, float(h)]
    der = np.trim_zeros([4.0 * c[4], 3.0 * c[3], 2.0 * c[2], c[1]], "f")
    if len(der) > 1:
        # the real part of every root, clipped: a point of [0, h] can only over-estimate the minimum, a real root is kept as it is
        cand += [float(min(max(r.real, 0.0), h)) for r in np.roots(der)]
    vals = [f(t) for t in cand]
    m = int(np.argmin(vals))
    return float(np.sqrt(max(vals[m], 0.0))), cand[m]


class ValidationMethods:
    def validate_solution(self, continuous=False, conflicts=False, clearance=False, delay=None):
        """Feasibility report of the stored trajectories: minimum pair distance over all stored samples and its
        first violation of R - 0.01 (device reduction, generalises scp.py:597-615), worst violation of every bound
        the reference imposes (scp.py:182-257) and of the final-state equalities (state K).

        continuous=True adds what the samples cannot show: ``min_pair_distance_continuous`` (minimum over every segment,
        not only its end points), ``collision_free_continuous`` (no segment below R - 0.01), ``n_violating_segments``,
        ``first_violation_continuous`` and ``closest_approach`` (each ``{"timestep", "time", "vehicles", "distance"}`` or
        None).

        conflicts=True (with continuous=True) lists every between-sample conflict: ``conflicts``, one dictionary per pair and
        contiguous stretch of time below R - 0.01 (conflicts.conflict_windows: vehicles, t_start, t_end, duration,
        min_distance, t_min_distance, first_timestep, n_segments, pieces), sorted by start time, and ``n_conflicts``.

        clearance=True (with continuous=True) adds the clearance profiles (scp_clearance_profile): ``vehicle_clearance``, a
        dictionary of length-N arrays -- every vehicle's closest approach over the whole flight: ``min_distance``, ``time``
        (seconds from the start), ``timestep``, ``partner``, ``sample_min_distance`` (at the samples only) and
        ``n_violating_segments``; ``step_clearance``, a dictionary of length-K arrays -- the fleet's closest approach within
        every segment: ``min_distance``, ``time``, ``vehicles`` (K x 2), ``sample_min_distance``, ``n_violating_segments``; and
        ``most_exposed_vehicle``: ``{"vehicle", "partner", "time", "distance"}`` of the smallest vehicle clearance (None
        without a pair).  A vehicle or step without a pair has min_distance inf, time nan and partner / vehicles -1.

        delay=S (an int, 0 <= S <= K, with continuous=True) adds the delay margins (scp_delay_margins): how close every vehicle
        comes to anybody if it ALONE starts s = 0 .. S steps late (held at its start, everybody else on schedule and parked at
        the goal afterwards).  ``delay_margin``: a dictionary of N x (S + 1) arrays ``min_distance``, ``time`` (seconds from
        the start; nan without a pair), ``partner`` (-1 without a pair) and ``n_violating_segments``; ``delay_tolerance``: a
        dictionary of length-N arrays ``steps`` (the largest s <= S such that the lags 0 .. s are all free of violating
        segments; -1 if lag 0 already violates), ``seconds`` (steps * h) and ``limited_by`` (the partner at lag steps + 1, -1
        where steps = S); ``least_tolerant_vehicle``: ``{"vehicle", "steps", "seconds", "partner", "time", "distance"}`` of
        the smallest ``steps`` (ties: the lowest index; partner, time and distance are those of lag steps + 1, or of lag S
        where steps = S; None without a pair).

        After set_corridors the report also has ``corridor``, what validate_corridor() returns (tolerance 0)."""
        if conflicts and not continuous:
            raise ValueError("conflicts=True lists the conflicts of the continuous-time check: it needs continuous=True")
        if clearance and not continuous:
            raise ValueError("clearance=True profiles the continuous-time check: it needs continuous=True")
        if delay is not None:
            if not continuous:
                raise ValueError("delay=S delays the vehicles of the continuous-time check: it needs continuous=True")
            whole_number(delay, 0, self.K, f"delay={delay!r}: the largest delay is a whole number of steps in [0, K = {self.K}]")
        self._require("validate_solution", trajectories=True)
        N, K, D, h = self.N, self.K, self.D, self.h
        a, v, p = (self.trajectories[k] for k in ("accelerations", "velocities", "positions"))
        q0, q1 = self.shard.pair_range()
        c = self._ctx
        dev = self._device_trajectories() if continuous else (c.tensor(p),)  # one upload for every pass below
        min_dist, first, _, _ = c.check_avoidance(N, K, D, self.R, dev[0], q0, q1)
        min_dist = self.shard.all_min(min_dist)
        first = self.shard.all_min_int(first)
        pf = self.final_positions.reshape(N, D)
        vf = self.final_velocities.reshape(N, D)
        vK = v[:, K - 1] + h * a[:, K - 1]
        pK = p[:, K - 1] + h * v[:, K - 1] + 0.5 * h * h * a[:, K - 1]
        over = lambda x, lo, hi: float(max(0.0, (lo - x).max(), (x - hi).max()))  # noqa: E731
        report = {
            "min_pair_distance": min_dist,
            "collision_free": first >= (1 << 63) - 1,
            "first_violation": None,
            "acc_violation": over(a, self.acc_min, self.acc_max),
            "jerk_violation": over(np.diff(a, axis=1) / h, self.jerk_min, self.jerk_max),
            "vel_violation": max(over(v[:, 1:], self.vel_min, self.vel_max), over(vK, self.vel_min, self.vel_max)),
            "pos_violation": over(p[:, 1:], np.asarray(self.pos_min, float), np.asarray(self.pos_max, float)),
            "final_position_error": float(np.abs(pK - pf).max()),
            "final_velocity_error": float(np.abs(vK - vf).max()),
        }
        if not report["collision_free"]:
            k, q = divmod(first, self.shard.pairs)
            i, j = pair_from_index(q, N)
            report["first_violation"] = {"timestep": int(k), "vehicles": (i, j),
                                         "distance": float(np.linalg.norm(p[i, k] - p[j, k]))}
        if continuous:
            report.update(self._continuous_separation(p, v, a, dev, q0, q1))
        if conflicts:
            mine = c.list_conflicts(N, K, D, h, self.R, *dev, q0, q1)
            report["conflicts"] = conflict_windows(self.shard.allgather_records(mine), N, K, h)
            report["n_conflicts"] = len(report["conflicts"])
        if clearance:
            report.update(self._clearance_profiles(dev, q0, q1))
        if delay is not None:
            report.update(self._delay_margins(dev, int(delay)))
        if self._corridor is not None:
            report["corridor"] = self.validate_corridor(dev=dev if continuous else None)
        return report

    def _delay_margins(self, dev, S):
        """The delay part of validate_solution: one device pass (scp_delay_margins) over this rank's vehicles of the device
        tensors dev = (positions, velocities, accelerations); the ranks' blocks are concatenated, nothing is merged."""
        N, K, D, h = self.N, self.K, self.D, self.h
        a0, a1 = self.shard.agent_range()
        mine = self._ctx.delay_margins(N, K, D, h, self.R, *dev, S, a0, a1)
        e = gather_delay_blocks(self.shard, mine, a0).reshape(N, S + 1)
        some = e["partner"] != np.uint32(_hip.NO_INDEX)
        n_viol = e["n_violating"].astype(np.int64)
        partner = np.where(some, e["partner"].astype(np.int64), -1)
        margin = {"min_distance": e["min_dist"].copy(),
                  "time": np.where(some, np.where(some, e["segment"], 0).astype(np.float64) * h + e["t_min"], np.nan),
                  "partner": partner, "n_violating_segments": n_viol}
        bad = n_viol > 0
        steps = np.where(bad.any(axis=1), bad.argmax(axis=1), S + 1).astype(np.int64) - 1  # the first violating lag, less one
        at = np.minimum(steps + 1, S)  # the lag that limits the vehicle (lag S where nothing does)
        idx = np.arange(N)
        tolerance = {"steps": steps, "seconds": steps * h, "limited_by": np.where(steps < S, partner[idx, at], -1)}
        least = None
        if N > 1:
            v = int(np.argmin(steps))  # ties: the lowest index
            least = {"vehicle": v, "steps": int(steps[v]), "seconds": float(steps[v] * h), "partner": int(partner[v, at[v]]),
                     "time": float(margin["time"][v, at[v]]), "distance": float(margin["min_distance"][v, at[v]])}
        return {"delay_margin": margin, "delay_tolerance": tolerance, "least_tolerant_vehicle": least}

    def _clearance_profiles(self, dev, q0, q1):
        """The clearance part of validate_solution: one device pass (scp_clearance_profile) over this rank's pair range of the
        device tensors dev = (positions, velocities, accelerations), combined entry by entry over the ranks (lexicographic
        minimum of (distance, row), minimum, integer sum)."""
        N, K, D, h = self.N, self.K, self.D, self.h
        pairs = self.shard.pairs
        out = {}
        for name, e in zip(("vehicle_clearance", "step_clearance"),
                           self._ctx.clearance_profile(N, K, D, h, self.R, *dev, q0, q1)):
            dist, row, t = self.shard.all_argmin_arrays(e["min_dist"], e["row"], e["t_min"])
            some = row != np.uint64(_hip.NO_ROW)
            r = np.where(some, row, 0).astype(np.int64)
            k, q = np.divmod(r, max(pairs, 1))
            i, j = pairs_from_index(q, N) if pairs else (np.zeros_like(q), np.zeros_like(q))
            prof = {"min_distance": dist, "time": np.where(some, k * h + t, np.nan)}
            if name == "vehicle_clearance":
                prof["timestep"] = np.where(some, k, -1)
                prof["partner"] = np.where(some, np.where(i == np.arange(N), j, i), -1)
            else:
                prof["vehicles"] = np.where(some[:, None], np.stack([i, j], axis=1), -1)
            prof["sample_min_distance"] = self.shard.all_min(e["sample_min_dist"])
            prof["n_violating_segments"] = self.shard.all_sum_int(e["n_violating"].astype(np.int64))
            out[name] = prof
        vc = out["vehicle_clearance"]
        out["most_exposed_vehicle"] = None
        if pairs:
            best = int(np.argmin(vc["min_distance"]))  # the closest approach of the continuous-time check; of its two vehicles the first
            out["most_exposed_vehicle"] = {"vehicle": best, "partner": int(vc["partner"][best]), "time": float(vc["time"][best]),
                                           "distance": float(vc["min_distance"][best])}
        return out

    def _continuous_separation(self, p, v, a, dev, q0, q1):
        """The continuous-time part of validate_solution: between two samples a vehicle flies p + t v + t^2/2 a (the
        kinematics of the stored trajectories), so two vehicles can pass each other inside a segment while every sampled
        distance is fine.  One device pass (scp_check_separation) over this rank's pair range of the device tensors dev (the
        host arrays p, v, a uploaded), combined over the ranks."""
        N, K, D, h = self.N, self.K, self.D, self.h
        st = self._ctx.check_separation(N, K, D, h, self.R, *dev, q0, q1)
        min_dist, row, t = self.shard.all_argmin(st["min_dist"], st["argmin_row"], st["argmin_t"])
        first = self.shard.all_min_int(st["first_violation"])
        n_viol = self.shard.all_sum_int(st["n_violating"])

        def where(r):
            k, q = divmod(int(r), self.shard.pairs)
            return int(k), pair_from_index(q, N)

        out = {"min_pair_distance_continuous": min_dist, "collision_free_continuous": n_viol == 0,
               "n_violating_segments": n_viol, "first_violation_continuous": None, "closest_approach": None}
        if self.shard.pairs and row < (1 << 63) - 1:
            k, (i, j) = where(row)
            out["closest_approach"] = {"timestep": k, "time": k * h + t, "vehicles": (i, j), "distance": min_dist}
        if n_viol:
            k, (i, j) = where(first)
            m, t1 = segment_min_distance(p[i, k] - p[j, k], v[i, k] - v[j, k], a[i, k] - a[j, k], h)
            out["first_violation_continuous"] = {"timestep": k, "time": k * h + t1, "vehicles": (i, j), "distance": m}
        return out
