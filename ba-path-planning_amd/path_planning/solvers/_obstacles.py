"""Static obstacles (not in the reference): the map, safe flight corridors as per-state position boxes,
reference paths around the obstacles, the distance field and the clearance of a plan.  ObstacleMethods is a state-free base of
solvers.scp.SCP.  It reads ``N``, ``K``, ``D``, ``h``, ``R``, ``space_dims``, ``acc_min`` / ``acc_max``, ``pos_min`` / ``pos_max``,
``initial_positions`` / ``final_positions``, ``trajectories`` and ``_ctx`` and calls ``_require`` / ``_device_trajectories``; it writes
``_obstacles`` (None or an ObstacleMap), ``obstacle_info`` (None or what set_obstacle_shapes rasterised), ``_corridor`` (None or
{"cells"}: the boxes of the segments, on the map's grid), ``_boxes`` (None or (lo, hi) device tensors (N, K, D) by state),
``_metric`` ((metric, prefer, weight) of set_search_metric) and ``last_info["corridor"]`` / ``last_info["reference"]``."""
import numpy as np

from .. import _hip
from ..scenarios.obstacles import default_search_stride


def whole_number(value, lo, hi, message):
    """The planner's one argument check for a count: ``value`` is an int (no bool, no float) in [lo, hi] (hi None: no upper
    bound), or ValueError(message)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        raise ValueError(message)


def search_metric(metric, keep_clear, clear_weight):
    """The checks of find_reference's ``metric`` / ``keep_clear`` / ``clear_weight`` -> (prefer, weight) of
    scp_lattice_penalties: prefer = keep_clear cells, weight = round(70 clear_weight) (one missing cell of clearance costs
    clear_weight straight moves per node passed)."""
    if metric not in ("hops", "length"):
        raise ValueError(f"metric={metric!r}: \"hops\" (fewest lattice moves) or \"length\" (weighted moves and clearance)")
    whole_number(keep_clear, 0, None, f"keep_clear={keep_clear!r}: a whole number of cells >= 0")
    if isinstance(clear_weight, bool) or not isinstance(clear_weight, (int, float, np.integer, np.floating)) or \
            not (clear_weight >= 0 and np.isfinite(clear_weight)):
        raise ValueError(f"clear_weight={clear_weight!r}: a finite number >= 0")
    if keep_clear > 0 and metric == "hops":
        raise ValueError(f"keep_clear={keep_clear} needs metric=\"length\": the search by hops does not read the distance field")
    weight = int(round(_hip.MOVE_WEIGHTS[0] * float(clear_weight)))
    if weight * int(keep_clear) > _hip.PENALTY_MAX_PRODUCT:
        raise ValueError(f"keep_clear={keep_clear} with clear_weight={clear_weight}: round(70 clear_weight) keep_clear = "
                         f"{weight * int(keep_clear)} exceeds {_hip.PENALTY_MAX_PRODUCT} (costs are 32-bit)")
    return int(keep_clear), weight


def path_sharing(share, capacity, groups, rounds):
    """The checks of set_path_sharing -> None (share = 0: off) or (share_weight, capacity, groups, rounds) for
    scp_negotiate_paths: share_weight = round(70 share); rounds stays None until the search knows N (twice the groups it runs
    with, at most the supported 64)."""
    if isinstance(share, bool) or not isinstance(share, (int, float, np.integer, np.floating)) or \
            not (share >= 0 and np.isfinite(share)):
        raise ValueError(f"share={share!r}: a finite number >= 0")
    share_weight = int(round(_hip.MOVE_WEIGHTS[0] * float(share)))
    if share_weight > _hip.PENALTY_MAX_PRODUCT:
        raise ValueError(f"share={share!r}: round(70 share) = {share_weight} exceeds {_hip.PENALTY_MAX_PRODUCT} (costs are 32-bit)")
    whole_number(capacity, 1, None, f"capacity={capacity!r}: a whole number of vehicles per node >= 1")
    whole_number(groups, 1, None, f"groups={groups!r}: a whole number >= 1")
    if rounds is not None:
        whole_number(rounds, 0, _hip.NEGOTIATE_MAX_ROUNDS, f"rounds={rounds!r}: a whole number in [0, {_hip.NEGOTIATE_MAX_ROUNDS}]")
    return (share_weight, int(capacity), int(groups), rounds if rounds is None else int(rounds)) if share_weight > 0 else None


def straight_reference(p0, pf, K):
    """The default reference path of SCP.set_corridors: the straight line from start to goal, sampled uniformly at the states
    j = 0 .. K -- (N, K + 1, D) from p0, pf (N, D)."""
    p0, pf = np.asarray(p0, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    s = (np.arange(K + 1, dtype=np.float64) / float(K))[None, :, None]
    return p0[:, None, :] + s * (pf - p0)[:, None, :]


def check_position_boxes(N, K, D, pos_min, pos_max, lo, hi):
    """Host validation of per-(vehicle, state) position boxes: (N, K, D) float arrays without NaN whose intersection with the
    workspace box is not empty for any state j = 1 .. K-1 (state 0 is fixed to the start and never constrained).  Returns
    (lo, hi) as contiguous float64 arrays; raises ValueError naming the first offending state."""
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    if lo.shape != (N, K, D) or hi.shape != (N, K, D):
        raise ValueError(f"position boxes need shape (N, K, D) = ({N}, {K}, {D}), got {lo.shape} and {hi.shape}")
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("position boxes must not hold NaN (use -inf / +inf for an unconstrained entry)")
    l = np.maximum(np.asarray(pos_min, dtype=np.float64), lo[:, 1:])
    u = np.minimum(np.asarray(pos_max, dtype=np.float64), hi[:, 1:])
    bad = np.argwhere(l > u)
    if bad.size:
        i, j, d = (int(x) for x in bad[0])
        raise ValueError(f"position box of vehicle {i}, state {j + 1}, coordinate {d} is empty inside the workspace: "
                         f"[{l[i, j, d]}, {u[i, j, d]}]")
    return lo, hi


def corridor_shrink(acc_min, acc_max, h, pad):
    """shrink of SCP.set_corridors: a quadratic leaves the chord of its end values by at most |a| h^2 / 8; pad pays for the
    QP's constraint tolerance"""
    pad = float(pad)
    if not (pad >= 0.0 and np.isfinite(pad)):
        raise ValueError(f"pad={pad!r}: a finite number >= 0")
    return max(abs(float(acc_min)), abs(float(acc_max))) * float(h) * float(h) / 8.0 + pad


class ObstacleMap:
    """The map of one SCP.set_obstacles on the device: the geometry ``grid`` (scp_occupancy_grid), the occupancy ``occ``, its
    summed table ``sat`` and the device time ``prepare_ms`` of making it -- and what is derived from the map once and kept
    while it lives: ``edge_masks`` {(stride, clearance): the search lattice's edge masks}, ``fields`` {gap: (distance
    field, its device ms)} and ``node_penalties`` {(stride, prefer, weight): the weighted search's node penalties}.  A new map
    is a new object, so all three are dropped with the old one."""

    def __init__(self, ctx, D, grid, occ):
        self.ctx, self.D, self.grid = ctx, D, grid
        self.occ, self.sat = ctx.occupancy_prepare(D, grid, occ)
        self.prepare_ms = ctx.last_pair_ms()
        self.edge_masks, self.fields, self.node_penalties = {}, {}, {}

    def edges(self, stride, clearance):
        """(the edge masks of the lattice of `stride` / `clearance` (device tensor), their device ms: 0.0 when cached)"""
        ms = 0.0
        if (stride, clearance) not in self.edge_masks:
            self.edge_masks[stride, clearance] = self.ctx.lattice_edges(self.D, self.grid, self.sat, stride, clearance)
            ms = self.ctx.last_pair_ms()
        return self.edge_masks[stride, clearance], ms

    def penalties(self, stride, prefer, weight):
        """(the node penalties of the lattice of `stride` from the gap-1 field (device tensor), their device ms -- the field's
        included where this call made it --: 0.0 when cached)"""
        ms = 0.0
        if (stride, prefer, weight) not in self.node_penalties:
            made = 1 not in self.fields
            field, field_ms = self.field(1)
            self.node_penalties[stride, prefer, weight] = self.ctx.lattice_penalties(self.D, self.grid, field, stride, prefer, weight)
            ms = self.ctx.last_pair_ms() + (field_ms if made else 0.0)
        return self.node_penalties[stride, prefer, weight], ms

    def field(self, gap):
        """(the distance field at `gap` (device tensor), the device ms of the call that made it)"""
        if gap not in self.fields:
            field = self.ctx.obstacle_distance(self.D, self.grid, self.occ, int(gap))
            self.fields[gap] = (field, self.ctx.last_pair_ms())
        return self.fields[gap]


class ObstacleMethods:
    def set_obstacles(self, occ, origin, cell):
        """Static obstacles as an occupancy grid: ``occ`` [nz][ny][nx] ([ny][nx] in 2-D; nonzero = occupied), ``origin`` the
        lower corner of cell (0, 0, 0), ``cell`` the edge length -- what scenarios.obstacles.rasterize returns.  Uploads the
        grid and prepares its summed table (scp_occupancy_prepare); corridors and boxes set before are dropped."""
        self._require("set_obstacles", one_rank=True)
        occ = np.asarray(occ)
        if self.D == 2 and occ.ndim == 2:
            occ = occ[None]
        if occ.ndim != 3 or (self.D == 2 and occ.shape[0] != 1) or min(occ.shape) < 1:
            raise ValueError(f"occ has shape {occ.shape}: need [nz][ny][nx]" + (" with nz = 1 (or [ny][nx])" if self.D == 2 else ""))
        if occ.size > _hip.CORRIDOR_MAX_CELLS:
            raise ValueError(f"the grid has {occ.size} cells, more than the supported 2^24")
        origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        cell = float(cell)
        if origin.size != self.D or not np.isfinite(origin).all():
            raise ValueError(f"origin needs {self.D} finite entries")
        if not (cell > 0.0 and np.isfinite(cell)):
            raise ValueError(f"cell={cell!r}: a finite number > 0")
        self._obstacles = ObstacleMap(self._ctx, self.D, _hip.occupancy_grid(self.D, origin, cell, occ.shape[::-1]), occ)
        self._corridor = self._boxes = None
        self.obstacle_info = None

    def set_obstacle_shapes(self, cell, *, discs=(), boxes=(), capsules=(), polygons=(), margin=None):
        """Static obstacles as shapes, rasterised on the device (scp_rasterize_shapes): ``discs`` (x, y[, z], r) (spheres in
        3-D) and ``boxes`` (min..., max...) as scenarios.obstacles.rasterize takes them, ``capsules`` (a..., b..., r) -- a
        segment with a radius: an oblique wall, a beam, a pipe -- and ``polygons`` (vertices (n, 2),) in 2-D, (vertices, z0,
        z1) in 3-D (the prism over a height range; any winding direction, convex or not); scenarios.obstacles.pack_shapes
        checks them.  The grid is scenarios.obstacles.grid_shape(space_dims, cell); a cell is occupied if it comes closer than
        ``margin`` (None: min_distance / 2, the body radius) to a shape or touches it.  The grid never visits the host: the
        device tensor goes straight to scp_occupancy_prepare.  Corridors and boxes set before are dropped, as with
        set_obstacles.  Returns and stores as ``obstacle_info``: {"n_shapes", "counts" (per kind), "dims", "cell", "margin",
        "n_cells", "n_occupied", "rasterize_ms", "prepare_ms" (device milliseconds)}."""
        from ..scenarios.obstacles import grid_shape, pack_shapes

        self._require("set_obstacle_shapes", one_rank=True)
        packed = pack_shapes(self.D, discs=discs, boxes=boxes, capsules=capsules, polygons=polygons)
        origin, dims = grid_shape(self.space_dims, cell)
        margin = float(self.R) / 2.0 if margin is None else float(margin)
        if not (margin >= 0.0 and np.isfinite(margin)):
            raise ValueError(f"margin={margin!r}: a finite number >= 0")
        c = self._ctx
        grid = _hip.occupancy_grid(self.D, origin, float(cell), dims)
        occ = c.rasterize_shapes(self.D, grid, packed, margin)
        rasterize_ms = c.last_pair_ms()
        self._obstacles = ObstacleMap(c, self.D, grid, occ)
        self._corridor = self._boxes = None
        self.obstacle_info = {"n_shapes": int(packed["shapes"].size), "counts": dict(packed["counts"]), "dims": tuple(dims),
                              "cell": float(cell), "margin": margin, "n_cells": int(occ.numel()),
                              "n_occupied": int(self._obstacles.sat.reshape(-1)[-1].item()), "rasterize_ms": rasterize_ms,
                              "prepare_ms": self._obstacles.prepare_ms}
        return self.obstacle_info

    def set_corridors(self, reference=None, max_grow=8, pad=0.02, allow_open=False):
        """Safe flight corridors around a reference path: for every vehicle and segment an axis-aligned box of free cells
        (scp_corridor_boxes: the cells of the segment's two reference points, grown by at most ``max_grow`` cells per
        direction), and for every state the intersection of the boxes of the two segments it ends, shrunk by
        ``max(|acc_min|, |acc_max|) h^2 / 8 + pad`` (scp_corridor_state_boxes) -- with that the whole segment stays in its box,
        not only its end states.  The state boxes become the bounds of the position rows of every QP of
        generate_trajectories / scp_iteration / repair_conflicts; validate_solution(corridor=True) checks the result.

        ``reference``: (N, K + 1, D), the reference point of every state j = 0 .. K; None: the straight line from start to
        goal; "search": what find_reference() returns with its defaults (paths around the obstacles); "shortened": what
        shorten_reference() returns with its defaults (those paths cut down to the corners they need).  A segment whose reference points lie on occupied cells or outside the grid is blocked, a state whose
        intersection is empty is open (unconstrained): both raise ValueError naming the first one unless ``allow_open``.
        Returns {"n_blocked", "n_open", "shrink", "boxes_ms", "state_boxes_ms"} (device milliseconds of the two kernels)."""
        self._require("set_corridors", one_rank=True)
        if isinstance(reference, str):
            if reference not in ("search", "shortened"):
                raise ValueError(f"reference={reference!r}: an array (N, K + 1, D), None (straight lines), \"search\" or "
                                 "\"shortened\"")
            reference, _ = self.find_reference() if reference == "search" else self.shorten_reference()
        self._require("set_corridors", obstacles=True, states=True)
        whole_number(max_grow, 0, _hip.CORRIDOR_MAX_GROW,
                     f"max_grow={max_grow!r}: a whole number of cells in [0, {_hip.CORRIDOR_MAX_GROW}]")
        shrink = corridor_shrink(self.acc_min, self.acc_max, self.h, pad)
        N, K, D, c, ob = self.N, self.K, self.D, self._ctx, self._obstacles
        if reference is None:
            reference = straight_reference(self.initial_positions.reshape(N, D), self.final_positions.reshape(N, D), K)
        reference = np.ascontiguousarray(reference, dtype=np.float64)
        if reference.shape != (N, K + 1, D):
            raise ValueError(f"reference needs shape (N, K + 1, D) = ({N}, {K + 1}, {D}), got {reference.shape}")
        cells, n_blocked = c.corridor_boxes(N, K, D, ob.grid, ob.sat, c.tensor(reference), int(max_grow))
        boxes_ms = c.last_pair_ms()
        lo, hi, n_open = c.corridor_state_boxes(N, K, D, ob.grid, cells, shrink)
        state_ms = c.last_pair_ms()
        info = {"n_blocked": int(n_blocked.item()), "n_open": int(n_open.item()), "shrink": shrink, "boxes_ms": boxes_ms,
                "state_boxes_ms": state_ms}
        if (info["n_blocked"] or info["n_open"]) and not allow_open:
            hc = cells.cpu().numpy()
            blocked = np.argwhere(hc[..., 3] < hc[..., 0])
            if blocked.size:
                i, g = (int(x) for x in blocked[0])
                raise ValueError(f"corridor: segment {g} of vehicle {i} is blocked (its reference points "
                                 f"{reference[i, g].tolist()} -> {reference[i, g + 1].tolist()} lie on occupied cells or outside "
                                 f"the grid); {info['n_blocked']} blocked segments, {info['n_open']} open states in all")
            opened = np.argwhere(np.isinf(lo.cpu().numpy()[:, 1:, 0]))
            i, j = (int(x) for x in opened[0])
            raise ValueError(f"corridor: state {j + 1} of vehicle {i} is open (the boxes of segments {j} and {j + 1}, shrunk by "
                             f"{shrink:.4g}, do not meet); {info['n_open']} open states in all")
        check_position_boxes(N, K, D, self.pos_min, self.pos_max, lo.cpu().numpy(), hi.cpu().numpy())
        self._corridor = {"cells": cells}
        self._boxes = (lo, hi)
        self.last_info["corridor"] = info
        return info

    def set_search_metric(self, metric="hops", keep_clear=0, clear_weight=1.0):
        """What the lattice search of find_reference / shorten_reference / set_corridors(reference="search" / "shortened")
        minimises from now on (the planner's setting: it outlives set_obstacles, and set_space_dims, which begins the next
        scenario of a reused solver, returns it to the default).  ``metric``: "hops" counts lattice moves, a
        diagonal one like a straight one (the default, scp_reference_paths); "length" searches by weighted length -- a straight
        move 70, a diagonal one 99 or, in space, 121 (scp_reference_paths_weighted, run to its fixed point) -- and, with
        ``keep_clear`` > 0, by clearance: every node whose block comes nearer to an obstacle than ``keep_clear`` cells (by the
        gap-1 distance field, rounded down) pays ``clear_weight`` straight moves per missing cell on every edge that touches
        it (scp_lattice_penalties, made once per map, stride and setting), so a path keeps to open space where that costs
        less than the detour.  assign_goals(cost="length") weighs its paths with the same ``keep_clear`` / ``clear_weight``.
        ValueError: a metric other than the two, keep_clear > 0 with "hops", round(70 clear_weight) keep_clear > 32768."""
        self._require("set_search_metric", one_rank=True)
        self._metric = (metric,) + search_metric(metric, keep_clear, clear_weight)

    def set_path_sharing(self, share=0.0, capacity=1, groups=4, rounds=None):
        """Whether the reference paths of find_reference / shorten_reference / set_corridors(reference="search" /
        "shortened") avoid each other's routes from now on (a planner setting like set_search_metric's: set_space_dims returns
        it to off).  Alone, every vehicle takes the cheapest doorway; with ``share`` > 0 the search is negotiated
        (scp_negotiate_paths): a node that more than ``capacity`` vehicles' paths use costs every further vehicle ``share``
        straight moves per vehicle over capacity on each edge that touches it (share_weight = round(70 share)), the fleet
        re-routes in ``groups`` groups, one group per round, for ``rounds`` rounds (None: 2 groups), and the set of paths with
        the smallest overuse -- the sum over the nodes of the vehicles beyond capacity -- is kept.  ``groups`` larger than N is
        clipped to N.  ``share`` = 0 is off.  It needs set_search_metric("length"): the search by hops has no penalties (the
        searches raise ValueError otherwise).  ValueError: share negative, not finite or round(70 share) > 32768; capacity < 1;
        groups < 1; rounds outside 0 .. 64."""
        self._require("set_path_sharing", one_rank=True)
        self._sharing = path_sharing(share, capacity, groups, rounds)

    def find_reference(self, stride=None, clearance=0, max_path=None, allow_unreachable=False):
        """Reference paths around the obstacles, one per vehicle, for set_corridors(reference=...): a breadth-first search on
        a lattice of blocks of ``stride`` x ``stride`` (x ``stride``) cells whose edges exist only where both blocks -- for a
        diagonal move the whole 2 x 2 (2 x 2 x 2) group -- grown by ``clearance`` cells are free (scp_lattice_edges, once per
        (stride, clearance)), then per vehicle the path with the fewest lattice moves from its start to its goal, sampled at
        the states j = 0 .. K (scp_reference_paths: one workgroup per vehicle).  ``stride`` None:
        scenarios.obstacles.default_search_stride; ``max_path`` None: min(lattice nodes, 8 K) nodes.

        Returns (reference (N, K + 1, D) ndarray, info) and stores info as ``last_info["reference"]``: ``status`` (per vehicle:
        0 found, 1 / 2 start / goal off the lattice or on a block that is not free, 3 unreachable, 4 longer than max_path),
        ``n_nodes``, ``n_failed``, ``stride``, ``clearance``, ``lattice``, ``max_edges`` (the largest E = n_nodes + 1),
        ``guaranteed`` (every found path has E <= K or 2 clearance >= stride ceil(E / K): set_corridors then reports no blocked
        segment for those vehicles), ``edges_ms`` / ``search_ms`` (device milliseconds; edges_ms 0 when the masks were
        cached).  A vehicle without a path keeps the straight line; unless ``allow_unreachable`` that raises ValueError.

        After set_search_metric("length", ...) the path is the cheapest by weighted length and clearance instead.  info
        also holds ``metric``, ``keep_clear``, ``cost`` (int64 per vehicle: the path's weighted cost under the penalties the
        path was found with, with "hops" its number of moves; -1 without a path) and ``penalties_ms`` (0.0 when cached or not
        needed).

        After set_path_sharing(share > 0) the search is the negotiation of scp_negotiate_paths (``search_ms``: all its rounds)
        and info holds ``sharing``: ``share_weight``, ``capacity``, ``groups``, ``rounds`` as they ran, ``overuse`` (a list:
        after the plain search and after every round), ``best_round`` (the round whose paths are returned), ``n_kept``
        (re-routings that kept the old path because the new one was longer than max_path) and ``max_load`` (the most paths of
        the returned set through one node: one further call, scp_path_load on the returned paths, and one further host read
        of its maximum)."""
        if clearance is None:
            raise ValueError("clearance=None: a whole number of cells >= 0")
        found = self._search_reference("find_reference", stride, clearance, max_path, want_path=False)
        info = found["info"]
        self.last_info["reference"] = info
        self._require_paths(info, allow_unreachable)
        return found["ref"].cpu().numpy(), info

    def _search_reference(self, who, stride, clearance, max_path, want_path):
        """the checks and the calls of find_reference -> {"ref", "path", "rec" (device tensors), "p0", "pf", "max_path",
        "info": what find_reference reports}"""
        metric, prefer, weight = self._metric
        sharing = self._sharing
        if sharing is not None and metric != "length":
            raise ValueError(f"{who}: set_path_sharing needs set_search_metric(\"length\") (the search by hops has no penalties "
                             "for the other vehicles' paths to add to)")
        stride, clearance, lattice, edges, edges_ms = self._lattice_edges(who, stride, clearance)
        N, K, D, c = self.N, self.K, self.D, self._ctx
        nodes = lattice[0] * lattice[1] * lattice[2]
        if max_path is None:
            max_path = min(nodes, 8 * K)
        whole_number(max_path, 1, nodes, f"max_path={max_path!r}: a whole number of nodes in [1, {nodes}]")
        p0, pf = self.initial_positions.reshape(N, D), self.final_positions.reshape(N, D)
        ref = c.tensor(straight_reference(p0, pf, K))
        d_p0, d_pf = c.tensor(p0), c.tensor(pf)
        pen, penalties_ms, path_cost, shared = None, 0.0, None, None
        if metric == "length":
            if prefer > 0 and weight > 0:
                pen, penalties_ms = self._obstacles.penalties(stride, prefer, weight)
            if sharing is not None:
                share_weight, capacity, groups, rounds = sharing
                # (`want_path` is not passed on: the path table is always made, path_load below reads it for max_load)
                groups = min(groups, N)
                rounds = min(2 * groups, _hip.NEGOTIATE_MAX_ROUNDS) if rounds is None else rounds
                path, dev_rec, path_cost, n_failed, overuse, best_round, n_kept = c.negotiate_paths(
                    N, K, D, self._obstacles.grid, stride, edges, d_p0, d_pf, int(max_path), ref, share_weight, capacity, groups,
                    rounds, pen=pen)
                shared = {"share_weight": share_weight, "capacity": capacity, "groups": groups, "rounds": rounds}
            else:
                path, dev_rec, path_cost, _, n_failed = c.reference_paths_weighted(
                    N, K, D, self._obstacles.grid, stride, edges, d_p0, d_pf, int(max_path), ref, pen=pen, want_path=want_path)
        else:
            path, dev_rec, _, n_failed = c.reference_paths(N, K, D, self._obstacles.grid, stride, edges, d_p0, d_pf, int(max_path),
                                                           ref, want_path=want_path)
        search_ms = c.last_pair_ms()
        rec = dev_rec.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:N]
        found = rec["status"] == 0
        cost = rec["n_nodes"].astype(np.int64) - 1 if path_cost is None else path_cost.cpu().numpy().view(np.uint32)[:N].astype(np.int64)
        E = rec["n_nodes"].astype(np.int64) + 1
        info = {"status": rec["status"].copy(), "n_nodes": rec["n_nodes"].copy(), "n_failed": int(n_failed.item()),
                "stride": stride, "clearance": clearance, "lattice": lattice[:D],
                "max_edges": int(E[found].max()) if found.any() else 0,
                "guaranteed": bool(((E <= K) | (2 * clearance >= stride * -(-E // K)))[found].all()),
                "edges_ms": edges_ms, "search_ms": search_ms, "metric": metric, "keep_clear": prefer,
                "cost": np.where(found, cost, -1), "penalties_ms": penalties_ms}
        if shared is not None:
            load, _ = c.path_load(N, int(max_path), nodes, path, dev_rec, capacity)
            shared.update(overuse=[int(v) for v in overuse.cpu().numpy().view(np.uint64)], best_round=int(best_round.item()),
                          n_kept=int(n_kept.item()), max_load=int(load.max().item()))
            info["sharing"] = shared
        return {"ref": ref, "path": path, "rec": dev_rec, "p0": d_p0, "pf": d_pf, "max_path": int(max_path), "info": info}

    def _lattice_edges(self, who, stride, clearance):
        """the checks of a call on the search lattice and its edge masks, made once per (stride, clearance) and map ->
        (stride, clearance, lattice (L_x, L_y, L_z), edges (device tensor), edges_ms: 0 when the masks were cached)"""
        self._require(who, one_rank=True, obstacles=True, states=True)
        K, D, grid = self.K, self.D, self._obstacles.grid
        dims = [int(grid.dims[d]) for d in range(D)]
        if stride is None:
            stride = default_search_stride(dims, K, D)
        if clearance is None:  # (shorten_reference: the stride)
            clearance = stride
        for name, value, least in (("stride", stride, 1), ("clearance", clearance, 0)):
            whole_number(value, least, None, f"{name}={value!r}: a whole number of cells >= {least}")
        stride, clearance = int(stride), int(clearance)
        lattice = _hip.lattice_shape(D, grid, stride)
        nodes = lattice[0] * lattice[1] * lattice[2]
        if nodes < 1 or nodes > _hip.LATTICE_MAX_NODES:
            raise ValueError(f"stride={stride}: a lattice of {lattice} nodes on a grid of {tuple(dims)} cells; supported are 1 .. "
                             f"{_hip.LATTICE_MAX_NODES} nodes")
        edges, edges_ms = self._obstacles.edges(stride, clearance)
        return stride, clearance, lattice, edges, edges_ms

    @staticmethod
    def _require_paths(info, allow_unreachable):
        if info["n_failed"] and not allow_unreachable:
            i = int(np.nonzero(info["status"] != 0)[0][0])
            raise ValueError(f"reference path: vehicle {i} has none: {_hip.PATH_STATUS[int(info['status'][i])]} (status "
                             f"{int(info['status'][i])}; stride {info['stride']}, clearance {info['clearance']}, lattice "
                             f"{info['lattice']}); {info['n_failed']} vehicles without a path in all")

    def shorten_reference(self, stride=None, clearance=None, max_path=None, allow_unreachable=False):
        """find_reference's paths, shortened: of every lattice path only the nodes that cannot be skipped are kept -- a node
        sees another if every lattice step of the straight run between them, grown by ``clearance`` cells, is free -- and
        the states j = 0 .. K are placed evenly by chord length along start, kept block centres, goal (scp_shorten_paths: one
        wave per vehicle).  ``clearance`` None: ``stride``, with which every path shorter than K block edges is guaranteed;
        the other parameters are find_reference's (after set_search_metric("length", ...) the weighted path is what gets
        shortened).

        Returns (reference (N, K + 1, D) ndarray, info) and stores info as ``last_info["reference"]``: what find_reference
        reports (its ``guaranteed`` replaced), and per vehicle ``n_kept`` (0 without a path), ``length`` / ``length_before``
        (metres, after / before) and ``delta`` = floor(length / (K cell)) + 1, the most cells two consecutive reference points
        lie apart per coordinate; ``guaranteed``: every found vehicle has clearance >= delta (set_corridors then reports no
        blocked segment for those vehicles); ``shorten_ms`` (device milliseconds)."""
        found = self._search_reference("shorten_reference", stride, clearance, max_path, want_path=True)
        info = found["info"]
        N, K, D, c, ob = self.N, self.K, self.D, self._ctx, self._obstacles
        _, out = c.shorten_paths(N, K, D, ob.grid, ob.sat, info["stride"], info["clearance"], found["p0"],
                                 found["pf"], found["max_path"], found["path"], found["rec"], found["ref"], want_kept=False)
        info["shorten_ms"] = c.last_pair_ms()
        out = out.cpu().numpy().view(_hip.SHORTEN_INFO_DTYPE)[:N]
        ok = info["status"] == 0
        info["n_kept"], info["length"], info["length_before"] = out["n_kept"].copy(), out["length"].copy(), out["length_before"].copy()
        info["delta"] = np.floor(out["length"] / (float(K) * float(ob.grid.cell))).astype(np.int64) + 1
        info["guaranteed"] = bool((info["clearance"] >= info["delta"])[ok].all())
        self.last_info["reference"] = info
        self._require_paths(info, allow_unreachable)
        return found["ref"].cpu().numpy(), info

    def set_position_boxes(self, lo, hi):
        """Per-(vehicle, state) position boxes, the general form of set_corridors (waypoints, keep-in regions): ``lo`` / ``hi``
        (N, K, D), state j = 0 .. K-1 of vehicle i must lie in [lo[i, j], hi[i, j]] intersected with the workspace box;
        -inf / +inf leave an entry unconstrained, state 0 (the start) is never constrained.  Both None: no boxes.  Every QP
        with boxes runs the round-2 persistent kernel or the three-launch pipeline."""
        if lo is None and hi is None:
            self._boxes = None
            return
        if lo is None or hi is None:
            raise ValueError("set_position_boxes: lo and hi are both given or both None")
        self._require("set_position_boxes", one_rank=True)
        lo, hi = check_position_boxes(self.N, self.K, self.D, self.pos_min, self.pos_max, lo, hi)
        self._boxes = (self._ctx.tensor(lo), self._ctx.tensor(hi))

    def _apply_boxes(self, qp):
        """the boxes into a QP whose problem has just been set (the Python-driven loops)"""
        if self._boxes is not None:
            self._require("position boxes", one_rank=True)
            qp.set_position_boxes(*self._boxes)

    def _native_boxes(self, nat):
        """the boxes (or none: a pooled solver may remember a released object's) into the native solver, before solve / step"""
        if self._boxes is not None:
            self._require("position boxes", one_rank=True)
        nat.set_position_boxes(*(self._boxes or (None, None)))

    def validate_corridor(self, tol=0.0, dev=None):
        """Does every segment of every vehicle of the stored trajectories stay inside its un-shrunk corridor box (set_corridors)
        over its whole duration, not only at its samples?  Exact per segment and coordinate (scp_check_corridor).  Returns
        ``vehicles``: a dictionary of length-N arrays ``max_excess`` (the largest distance by which a segment leaves its box in
        any coordinate; <= 0: inside), ``segment`` (where; -1: none judged), ``n_blocked`` (blocked segments are not judged)
        and ``n_outside`` (segments with excess > tol); the totals ``n_outside``, ``n_blocked``, ``max_excess``,
        ``worst_vehicle``; ``inside`` = no segment outside and none blocked; ``check_ms`` (device time).  validate_solution
        includes it as ``report["corridor"]``.  The cells stay those of the latest set_corridors, also after
        set_position_boxes(None, None): a plan made without boxes can be judged against them."""
        if self._corridor is None:
            raise ValueError("validate_corridor checks the boxes of set_corridors: call it first")
        self._require("validate_corridor", trajectories=True)
        c = self._ctx
        if dev is None:
            dev = self._device_trajectories()
        st = c.check_corridor(self.N, self.K, self.D, self.h, self._obstacles.grid, self._corridor["cells"], *dev, tol=float(tol))
        seg = np.where(st["segment"] == np.uint32(_hip.NO_INDEX), -1, st["segment"].astype(np.int64))
        n_out, n_blk = int(st["n_outside"].sum()), int(st["n_blocked"].sum())
        return {"vehicles": {"max_excess": st["max_excess"].copy(), "segment": seg, "n_blocked": st["n_blocked"].astype(np.int64),
                             "n_outside": st["n_outside"].astype(np.int64)},
                "n_outside": n_out, "n_blocked": n_blk, "max_excess": float(st["max_excess"].max()),
                "worst_vehicle": int(np.argmax(st["max_excess"])), "inside": n_out == 0 and n_blk == 0,
                "check_ms": c.last_pair_ms()}

    def _obstacle_field(self, who, gap):
        """the device field of the current obstacles at `gap` (made once per set_obstacles), and the device time it took"""
        self._require(who, one_rank=True, obstacles=True)
        if isinstance(gap, bool) or gap not in (0, 1):
            raise ValueError(f"gap={gap!r}: 0 (between cells) or 1 (between the closed cubes of the cells)")
        return self._obstacles.field(gap)

    def obstacle_distance_field(self, gap=1):
        """The exact squared distance field of the obstacles (scp_obstacle_distance), in cells: a numpy uint32 array
        [nz][ny][nx]; entry c = min over the occupied cells o of sum_d max(|c_d - o_d| - gap, 0)^2, 2^32 - 1 everywhere on an
        empty map.  ``gap=0``: the squared Euclidean distance transform between cells.  ``gap=1``: the squared distance between
        the closed cubes of the cells, so every point of cell c keeps at least cell * sqrt(field[c]) from the occupied
        cells -- what obstacle_clearance reduces, and the input for choosing a corridor clearance or for plots.  The device
        field is computed once per set_obstacles and gap."""
        field, _ = self._obstacle_field("obstacle_distance_field", gap)
        return field.cpu().numpy().view(np.uint32)

    def obstacle_clearance(self, pieces=4, dev=None):
        """How close does every vehicle of the stored trajectories come to the obstacles, where and when?  Judges the plan
        against the map itself (scp_obstacle_clearance), whatever made the plan: it needs set_obstacles and trajectories, no
        corridors and no boxes.  Every segment is cut into ``pieces`` (1 .. 16) pieces; a piece's value is the minimum of the
        gap-1 distance field over the exact range of cells it passes through, so the piece keeps at least that distance.
        Returns ``vehicles``: a dictionary of length-N arrays ``clearance`` (metres, a guaranteed lower bound: cell *
        sqrt(min_sq); 0: may touch; inf: nothing judged or an empty map), ``min_sq`` (cells squared; -1 where clearance is
        inf), ``segment``, ``piece``, ``cell`` (the linear index (z ny + y) nx + x of the cell that attains it; -1: none),
        ``n_touch`` (pieces whose range holds an occupied cell), ``n_off`` (pieces off the map, not judged) and ``n_wide``
        (pieces whose range holds more than 4096 cells, not judged: use more pieces); ``steps``: length-K arrays
        ``clearance`` (the fleet's clearance within every time step) and ``vehicle`` (who attains it, the lowest index on
        ties; -1 where no piece of the step was judged); the totals ``clearance``, ``worst_vehicle``, ``n_touch``, ``n_off``,
        ``n_wide``; ``clear`` = no piece touches and none is wide; ``field_ms`` and ``check_ms`` (device time of the field,
        made once per set_obstacles, and of the pass)."""
        self._require("obstacle_clearance", one_rank=True, obstacles=True, trajectories=True)
        whole_number(pieces, 1, _hip.OBSTACLE_MAX_PIECES, f"pieces={pieces!r}: a whole number in [1, {_hip.OBSTACLE_MAX_PIECES}]")
        c, ob = self._ctx, self._obstacles
        field, field_ms = ob.field(1)
        if dev is None:
            dev = self._device_trajectories()
        st, step_min = c.obstacle_clearance(self.N, self.K, self.D, self.h, ob.grid, ob.sat, field, int(pieces), *dev)
        check_ms = c.last_pair_ms()
        cell = float(ob.grid.cell)

        def metres(sq):  # (sq as int64; DIST_NONE: inf)
            none = sq == _hip.DIST_NONE
            return np.where(none, np.inf, cell * np.sqrt(np.where(none, 0, sq).astype(np.float64)))

        sq = st["min_sq"].astype(np.int64)
        none = sq == _hip.DIST_NONE
        vehicles = {"clearance": metres(sq), "min_sq": np.where(none, -1, sq),
                    "segment": np.where(none, -1, st["segment"].astype(np.int64)),
                    "piece": np.where(none, -1, st["piece"].astype(np.int64)), "cell": st["cell"].astype(np.int64),
                    "n_touch": st["n_touch"].astype(np.int64), "n_off": st["n_off"].astype(np.int64),
                    "n_wide": st["n_wide"].astype(np.int64)}
        step_sq = (step_min >> np.uint64(32)).astype(np.int64)
        judged = step_min != np.uint64(2**64 - 1)
        steps = {"clearance": metres(step_sq),
                 "vehicle": np.where(judged, (step_min & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)}
        n_touch, n_off, n_wide = (int(vehicles[k].sum()) for k in ("n_touch", "n_off", "n_wide"))
        return {"vehicles": vehicles, "steps": steps, "clearance": float(vehicles["clearance"].min()),
                "worst_vehicle": int(np.argmin(vehicles["clearance"])), "n_touch": n_touch, "n_off": n_off, "n_wide": n_wide,
                "clear": n_touch == 0 and n_wide == 0, "field_ms": field_ms, "check_ms": check_ms}
