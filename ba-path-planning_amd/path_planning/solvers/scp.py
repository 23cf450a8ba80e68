"""SCP trajectory planner -- MI355X-native drop-in for the reference's ``path_planning.solvers.scp.SCP``.

Same constructor, attributes, methods, stdout lines and error behaviour as
/root/reference/src/path_planning/solvers/scp.py (class SCP, :31-616); every method below cites the lines it
replaces.  The numerical work runs in hand-written HIP kernels behind the C-ABI of include/scp_hip.h
(libscp_hip.so, bound with ctypes in path_planning/_hip.py); PyTorch-ROCm tensors are device buffers only.
There is no CPU fallback: constructing the solver without a GPU or without the built library raises.

Differences to the reference that a caller can observe (INTEGRATION.md has the full list):
  * the QP solver is this repo's ADMM (OSQP's algorithm, matrix-free) instead of the `osqp` package, so
    iterates agree with the reference only up to OSQP's own tolerance (eps_abs = eps_rel = 1e-3);
  * ``_add_collision_constraints`` returns the compact form (eta, l) of the constraint rows instead of a
    2.6e9-non-zero CSC matrix; ``C_jerk/C_acc/C_vel/C_pos`` are not materialised (they stay None);
  * new keyword-only arguments: ``dim`` (2 or 3), ``device``, ``qp_settings``, ``working_set_margin``,
    ``feasibility_tol``, ``max_rounds``, ``refresh_feasibility``, ``polish``/``polish_eps``, ``native``, ``row_free``, ``carry_rho``, ``kernel_timing``,
    ``qp_row_capacity``, ``reuse_native``, ``verbose``, ``rank``/``world_size``/``group`` (pair-range-sharded multi-GPU: the SCP iteration natively,
    split at its exchange points -- ``scp_iteration_sharded``).
"""
from __future__ import annotations

import atexit
import threading
import time

import numpy as np

from .. import _hip
from .._sharding import Shard
from ..scenarios.obstacles import default_search_stride
from .conflicts import conflict_windows, pairs_from_index
from .stagger import candidate_orders, refined_orders, schedule_key, staggered_fleet

# The reference's callers build a NEW solver object per scenario (compute_trajectories_batch.py:103-117).  Here an object owns a
# library context and a native solver (device workspace, pinned host words, the K x K blocks cached per rho): ~0.7 ms to
# create, against a 2.5 ms solve at 128 agents.  So the native halves of released SCP objects on the DEFAULT stream are kept,
# per (device, shape, settings), and the next object of the same shape adopts them -- same results bit for bit (a pooled solver is what
# compute-trajectories-batch has always reused per worker; tests/test_scp_gpu.py::test_released_solvers_are_reused).
_POOL = {}
_POOL_LOCK = threading.Lock()
_POOL_LIMIT = 4  # per key
_POOL_STATS = {"hits": 0, "misses": 0, "returned": 0}


def native_pool_stats():
    """{"hits", "misses", "returned", "held"}: how often a new SCP object adopted the native solver of a released one."""
    with _POOL_LOCK:
        return dict(_POOL_STATS, held=sum(len(v) for v in _POOL.values()))


def clear_native_pool():
    """Destroy every pooled native solver and context (also registered with atexit: before the HIP runtime goes away)."""
    with _POOL_LOCK:
        entries = [e for v in _POOL.values() for e in v]
        _POOL.clear()
    for ctx, nat in entries:
        try:
            nat.close()
            ctx.close()
        except Exception:
            pass


atexit.register(clear_native_pool)


def gather_delay_blocks(shard, mine, a0):
    """The ranks' blocks of delay margins (DELAY_DTYPE, (vehicles of the rank, S + 1), the rank's first vehicle a0) concatenated
    in vehicle order, flat: the records travel through Shard.allgather_records under the row id a (S + 1) + s, as their bytes."""
    lags = mine.shape[1]
    rec = np.empty(mine.size, dtype=[("row", np.uint64)] + _hip.DELAY_DTYPE.descr)
    rec["row"] = a0 * lags + np.arange(mine.size)
    for f in _hip.DELAY_DTYPE.names:
        rec[f] = mine.reshape(-1)[f]
    return shard.allgather_records(rec)[list(_hip.DELAY_DTYPE.names)]


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


class SCP:
    def __init__(
        self,
        n_vehicles=5,
        time_horizon=3.0,
        time_step=0.1,
        min_distance=0.1,
        space_dims=None,
        *,
        dim=2,
        device=None,
        qp_settings=None,
        working_set_margin=0.5,
        feasibility_tol=1e-6,
        max_rounds=20,
        refresh_feasibility=False,
        polish=False,
        polish_eps=1e-8,
        native=True,
        row_free=True,
        carry_rho=False,
        kernel_timing=True,
        qp_row_capacity=None,
        verbose=True,
        rank=0,
        world_size=1,
        group=None,
        reuse_native=True,
    ):
        # --- reference attributes (scp.py:40-91) ---
        self.N = n_vehicles
        self.T = time_horizon
        self.h = time_step
        self.K = int(self.T / self.h)  # scp.py:43
        self.R = min_distance
        self.D = int(dim)
        if self.D not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        if space_dims is None:
            space_dims = [0, 0, 20, 20] if self.D == 2 else [0, 0, 0, 20, 20, 20]
        self.space_dims = space_dims
        if len(space_dims) != 2 * self.D:
            raise ValueError(f"space_dims needs {2 * self.D} entries [min..., max...]")
        self.convergence_tolerance = 1.5e-2
        self.trajectories = None
        self.initial_positions = None
        self.initial_velocities = None
        self.final_positions = None
        self.final_velocities = None
        self._final_given = None  # final states in the order given to set_final_states, once assign_goals has permuted them
        self.goal_assignment = None
        self.assignment_info = None
        self.pos_min = np.array(space_dims[: self.D])
        self.pos_max = np.array(space_dims[self.D:])
        self.vel_min = -2
        self.vel_max = 2
        self.acc_min = -15.0
        self.acc_max = 15.0
        self.jerk_min = -20
        self.jerk_max = 20
        self.C_jerk = self.C_acc = self.C_vel = self.C_pos = None  # never materialised on this path
        self.l_jerk, self.u_jerk = [], []
        self.l_acc, self.u_acc = [], []
        self.l_vel, self.u_vel = [], []
        self.l_pos, self.u_pos = [], []

        # --- MI355X path ---
        self.verbose = verbose
        self.working_set_margin = float(working_set_margin)
        self.feasibility_tol = float(feasibility_tol)
        self.max_rounds = int(max_rounds)
        self.refresh_feasibility = bool(refresh_feasibility)
        self.polish = bool(polish)
        self.polish_eps = float(polish_eps)
        self.native = bool(native)  # drive the SCP loop from C++ (scp_solver_solve) instead of from Python: same calls, same bits
        # native loop: linearise WITHOUT writing the 24-byte rows of all N(N-1)/2 K pairs (scp_select_pairs) and recompute eta / l
        # for the selected rows only (scp_qp_add_rows_at); False: scp_linearize_pairs writes every row (what
        # _add_collision_constraints returns, and what the Python-driven loop does).  Same working rows, same bits.
        self.row_free = bool(row_free)
        # opt-in: the joint QP of SCP iteration n + 1 starts at the rho iteration n ended with instead of OSQP's 0.1 (the
        # reference builds a new osqp.OSQP() per iteration, scp.py:441): saves the adaptive-rho transient of every later QP
        self.carry_rho = bool(carry_rho)
        self._rho_start = 0.0
        self._native = None
        self._qp_row_capacity = qp_row_capacity  # initial working-set capacity (grows on demand)
        self._qp_overrides = dict(qp_settings or {})
        self.shard = Shard(self.N, rank, world_size, group)
        if device is None:
            import torch

            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        # the native half of a released object of the same shape on this stream, if there is one (module docstring of _POOL)
        self.reuse_native = bool(reuse_native)
        self._pool_key = None
        if self.reuse_native:
            import torch

            st = self._qp_settings()
            tdev = torch.device("cuda", int(device))
            on_default = torch.cuda.is_available() and (torch.cuda.current_stream(tdev).cuda_stream
                                                        == torch.cuda.default_stream(tdev).cuda_stream)
            if on_default:  # (a context is bound to its stream: only the default stream is sure to outlive the pool)
                self._pool_key = (int(device), int(self.N), int(self.K), self.D, float(self.h), float(self.R), bytes(st),
                                  self._qp_row_capacity)
                with _POOL_LOCK:
                    held = _POOL.get(self._pool_key)
                    entry = None
                    while held and entry is None:
                        entry = held.pop()
                        if not getattr(entry[0], "h", None):  # (collected in one cycle with its owner: the owner's finaliser
                            entry = None                      # pooled the context, the context's own then destroyed it)
                    _POOL_STATS["hits" if entry else "misses"] += 1
                if entry:
                    self._ctx, self._native = entry
        if self._native is None:
            self._ctx = _hip.Context(device)  # raises without a GPU / without libscp_hip.so
        # False: no HIP events around the kernels (linearize_ms / violations_ms read 0, solve_ms is host wall clock): fewer queue
        # packets per solve, for many concurrent solves on one GPU
        self.kernel_timing = bool(kernel_timing)
        self._ctx.set_timing(self.kernel_timing)
        self._qp = None
        self._pairs = None
        self._holds = None  # (device table, count) of repair_conflicts while one of its passes runs
        self.staggered = None  # the fleet of the latest stagger_starts (its trajectories stay as they are)
        self._obstacles = None  # set_obstacles: {"grid", "occ", "sat"} (device), the occupancy grid and its summed table;
                                # find_reference adds "edges": {(stride, clearance): the lattice's edge masks},
                                # obstacle_distance_field / obstacle_clearance "field": {gap: (device field, its ms)}
        self._corridor = None   # set_corridors: {"cells", "grid"}: the boxes of the segments, what validate_solution checks
        self._boxes = None      # (lo, hi) device tensors (N, K, D) by state: set_corridors / set_position_boxes
        self._dev = {}
        self.last_info = {}

        self._print("---=== SCP Problem initialized ===---")
        self._print(f"Number of timesteps: {self.K}")
        self._print(f"Timestep: {self.h}")
        self._print(f"Minimum distance between vehicles: {self.R}")
        self._print(f"Space dimensions: {self.space_dims}")

    def _print(self, *a):
        if self.verbose and self.shard.rank == 0:
            print(*a)

    def set_space_dims(self, space_dims):
        """Change the workspace box of an existing solver (same N, T, h, R, dim).  Together with set_initial_states /
        set_final_states this lets one solver object -- its context, streams, pinned buffers and the QP workspace, whose
        creation costs more than a 100-agent solve -- be reused for the next scenario (compute-trajectories-batch)."""
        if len(space_dims) != 2 * self.D:
            raise ValueError(f"space_dims needs {2 * self.D} entries [min..., max...]")
        self.space_dims = space_dims
        self.pos_min = np.array(space_dims[: self.D])
        self.pos_max = np.array(space_dims[self.D:])
        self.trajectories = None
        self._obstacles = self._corridor = self._boxes = None  # (they belong to the scenario that is being replaced)

    # ------------------------------------------------------------------------------------------------
    # static obstacles (not in the reference): safe flight corridors as per-state position boxes, DESIGN.md section 3.9
    # ------------------------------------------------------------------------------------------------
    def _one_rank(self, what):
        if self.shard.world != 1:
            raise ValueError(f"{what} supports one rank only (world_size == 1)")

    def set_obstacles(self, occ, origin, cell):
        """Static obstacles as an occupancy grid: ``occ`` [nz][ny][nx] ([ny][nx] in 2-D; nonzero = occupied), ``origin`` the
        lower corner of cell (0, 0, 0), ``cell`` the edge length -- what scenarios.obstacles.rasterize returns.  Uploads the
        grid and prepares its summed table (scp_occupancy_prepare); corridors and boxes set before are dropped."""
        self._one_rank("set_obstacles")
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
        grid = _hip.occupancy_grid(self.D, origin, cell, occ.shape[::-1])
        occ_dev, sat = self._ctx.occupancy_prepare(self.D, grid, occ)
        self._obstacles = {"grid": grid, "occ": occ_dev, "sat": sat, "prepare_ms": self._ctx.last_pair_ms()}
        self._corridor = self._boxes = None

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
        self._one_rank("set_corridors")
        if isinstance(reference, str):
            if reference not in ("search", "shortened"):
                raise ValueError(f"reference={reference!r}: an array (N, K + 1, D), None (straight lines), \"search\" or "
                                 "\"shortened\"")
            reference, _ = self.find_reference() if reference == "search" else self.shorten_reference()
        if self._obstacles is None:
            raise ValueError("set_corridors needs set_obstacles first")
        if self.initial_positions is None or self.final_positions is None:
            raise ValueError("set_corridors needs both set_initial_states and set_final_states first")
        if isinstance(max_grow, bool) or not isinstance(max_grow, (int, np.integer)) or not 0 <= max_grow <= _hip.CORRIDOR_MAX_GROW:
            raise ValueError(f"max_grow={max_grow!r}: a whole number of cells in [0, {_hip.CORRIDOR_MAX_GROW}]")
        shrink = corridor_shrink(self.acc_min, self.acc_max, self.h, pad)
        N, K, D, c = self.N, self.K, self.D, self._ctx
        if reference is None:
            reference = straight_reference(self.initial_positions.reshape(N, D), self.final_positions.reshape(N, D), K)
        reference = np.ascontiguousarray(reference, dtype=np.float64)
        if reference.shape != (N, K + 1, D):
            raise ValueError(f"reference needs shape (N, K + 1, D) = ({N}, {K + 1}, {D}), got {reference.shape}")
        grid = self._obstacles["grid"]
        cells, n_blocked = c.corridor_boxes(N, K, D, grid, self._obstacles["sat"], c.tensor(reference), int(max_grow))
        boxes_ms = c.last_pair_ms()
        lo, hi, n_open = c.corridor_state_boxes(N, K, D, grid, cells, shrink)
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
        self._corridor = {"cells": cells, "grid": grid}
        self._boxes = (lo, hi)
        self.last_info["corridor"] = info
        return info

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
        cached).  A vehicle without a path keeps the straight line; unless ``allow_unreachable`` that raises ValueError."""
        if clearance is None:
            raise ValueError("clearance=None: a whole number of cells >= 0")
        found = self._search_reference("find_reference", stride, clearance, max_path, want_path=False)
        info = found["info"]
        self.last_info["reference"] = info
        self._require_paths(info, allow_unreachable)
        return found["ref"].cpu().numpy(), info

    def _search_reference(self, who, stride, clearance, max_path, want_path):
        """the checks and the two calls of find_reference -> {"ref", "path", "rec" (device tensors), "p0", "pf", "max_path",
        "info": what find_reference reports}"""
        stride, clearance, lattice, edges, edges_ms = self._lattice_edges(who, stride, clearance)
        N, K, D, c = self.N, self.K, self.D, self._ctx
        grid = self._obstacles["grid"]
        nodes = lattice[0] * lattice[1] * lattice[2]
        if max_path is None:
            max_path = min(nodes, 8 * K)
        if isinstance(max_path, bool) or not isinstance(max_path, (int, np.integer)) or not 1 <= max_path <= nodes:
            raise ValueError(f"max_path={max_path!r}: a whole number of nodes in [1, {nodes}]")
        p0, pf = self.initial_positions.reshape(N, D), self.final_positions.reshape(N, D)
        ref = c.tensor(straight_reference(p0, pf, K))
        d_p0, d_pf = c.tensor(p0), c.tensor(pf)
        path, dev_rec, _, n_failed = c.reference_paths(N, K, D, grid, stride, edges, d_p0, d_pf, int(max_path), ref,
                                                       want_path=want_path)
        search_ms = c.last_pair_ms()
        rec = dev_rec.cpu().numpy().view(_hip.PATH_INFO_DTYPE)[:N]
        found = rec["status"] == 0
        E = rec["n_nodes"].astype(np.int64) + 1
        info = {"status": rec["status"].copy(), "n_nodes": rec["n_nodes"].copy(), "n_failed": int(n_failed.item()),
                "stride": stride, "clearance": clearance, "lattice": lattice[:D],
                "max_edges": int(E[found].max()) if found.any() else 0,
                "guaranteed": bool(((E <= K) | (2 * clearance >= stride * -(-E // K)))[found].all()),
                "edges_ms": edges_ms, "search_ms": search_ms}
        return {"ref": ref, "path": path, "rec": dev_rec, "p0": d_p0, "pf": d_pf, "max_path": int(max_path), "info": info}

    def _lattice_edges(self, who, stride, clearance):
        """the checks of a call on the search lattice and its edge masks, made once per (stride, clearance) and map ->
        (stride, clearance, lattice (L_x, L_y, L_z), edges (device tensor), edges_ms: 0 when the masks were cached)"""
        self._one_rank(who)
        if self._obstacles is None:
            raise ValueError(f"{who} needs set_obstacles first")
        if self.initial_positions is None or self.final_positions is None:
            raise ValueError(f"{who} needs both set_initial_states and set_final_states first")
        K, D, c = self.K, self.D, self._ctx
        grid = self._obstacles["grid"]
        dims = [int(grid.dims[d]) for d in range(D)]
        if stride is None:
            stride = default_search_stride(dims, K, D)
        if clearance is None:  # (shorten_reference: the stride)
            clearance = stride
        for name, value, least in (("stride", stride, 1), ("clearance", clearance, 0)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
                raise ValueError(f"{name}={value!r}: a whole number of cells >= {least}")
        stride, clearance = int(stride), int(clearance)
        lattice = _hip.lattice_shape(D, grid, stride)
        nodes = lattice[0] * lattice[1] * lattice[2]
        if nodes < 1 or nodes > _hip.LATTICE_MAX_NODES:
            raise ValueError(f"stride={stride}: a lattice of {lattice} nodes on a grid of {tuple(dims)} cells; supported are 1 .. "
                             f"{_hip.LATTICE_MAX_NODES} nodes")
        cache = self._obstacles.setdefault("edges", {})
        edges_ms = 0.0
        if (stride, clearance) not in cache:
            cache[stride, clearance] = c.lattice_edges(D, grid, self._obstacles["sat"], stride, clearance)
            edges_ms = c.last_pair_ms()
        return stride, clearance, lattice, cache[stride, clearance], edges_ms

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
        the other parameters are find_reference's.

        Returns (reference (N, K + 1, D) ndarray, info) and stores info as ``last_info["reference"]``: what find_reference
        reports (its ``guaranteed`` replaced), and per vehicle ``n_kept`` (0 without a path), ``length`` / ``length_before``
        (metres, after / before) and ``delta`` = floor(length / (K cell)) + 1, the most cells two consecutive reference points
        lie apart per coordinate; ``guaranteed``: every found vehicle has clearance >= delta (set_corridors then reports no
        blocked segment for those vehicles); ``shorten_ms`` (device milliseconds)."""
        found = self._search_reference("shorten_reference", stride, clearance, max_path, want_path=True)
        info = found["info"]
        N, K, D, c = self.N, self.K, self.D, self._ctx
        grid = self._obstacles["grid"]
        _, out = c.shorten_paths(N, K, D, grid, self._obstacles["sat"], info["stride"], info["clearance"], found["p0"],
                                 found["pf"], found["max_path"], found["path"], found["rec"], found["ref"], want_kept=False)
        info["shorten_ms"] = c.last_pair_ms()
        out = out.cpu().numpy().view(_hip.SHORTEN_INFO_DTYPE)[:N]
        ok = info["status"] == 0
        info["n_kept"], info["length"], info["length_before"] = out["n_kept"].copy(), out["length"].copy(), out["length_before"].copy()
        info["delta"] = np.floor(out["length"] / (float(K) * float(grid.cell))).astype(np.int64) + 1
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
        self._one_rank("set_position_boxes")
        lo, hi = check_position_boxes(self.N, self.K, self.D, self.pos_min, self.pos_max, lo, hi)
        self._boxes = (self._ctx.tensor(lo), self._ctx.tensor(hi))

    def _apply_boxes(self, qp):
        """the boxes into a QP whose problem has just been set (the Python-driven loops)"""
        if self._boxes is not None:
            self._one_rank("position boxes")
            qp.set_position_boxes(*self._boxes)

    def _native_boxes(self, nat):
        """the boxes (or none: a pooled solver may remember a released object's) into the native solver, before solve / step"""
        if self._boxes is not None:
            self._one_rank("position boxes")
        nat.set_position_boxes(*(self._boxes or (None, None)))

    # ------------------------------------------------------------------------------------------------
    # a0: states (scp.py:99-129)
    # ------------------------------------------------------------------------------------------------
    def set_initial_states(self, positions, velocities=None):
        """Set initial states for all vehicles in flat format (scp.py:99-113)."""
        if velocities is None:
            velocities = np.zeros((self.N, self.D))
        self.initial_positions = np.asarray(positions, dtype=float).flatten()
        self.initial_velocities = np.asarray(velocities, dtype=float).flatten()
        assert len(self.initial_positions) == len(self.initial_velocities) == self.D * self.N, (
            f"Initial states mismatch"
            f"positions={len(self.initial_positions)}, "
            f"velocities={len(self.initial_velocities)}, "
            f"expected={self.D * self.N}"
        )
        self._dev.pop("p0", None)

    def set_final_states(self, positions, velocities=None):
        """Set final states for all vehicles in flat format (scp.py:115-129)."""
        if velocities is None:
            velocities = np.zeros((self.N, self.D))
        self.final_positions = np.asarray(positions, dtype=float).flatten()
        self.final_velocities = np.asarray(velocities, dtype=float).flatten()
        assert len(self.final_positions) == len(self.final_velocities) == self.D * self.N, (
            f"Final states mismatch"
            f"positions={len(self.final_positions)}, "
            f"velocities={len(self.final_velocities)}, "
            f"expected={self.D * self.N}"
        )
        self._dev.pop("p0", None)
        self._final_given = None  # (assign_goals keeps the order given here)
        self.goal_assignment = None
        self.assignment_info = None

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

        Returns goal_assignment."""
        from ..scenarios.assignment import _ASSIGN_KEYS, _LINE_KEYS, assign_method, hop_totals, path_costs

        if cost not in ("line", "path"):
            raise ValueError(f"cost={cost!r}: \"line\" or \"path\"")
        if cost == "path":
            if self.N > _hip.ASSIGN_COSTS_MAX_N:
                raise ValueError(f"assign_goals(cost=\"path\") supports up to {_hip.ASSIGN_COSTS_MAX_N} vehicles (one N x N cost "
                                 f"matrix in one workgroup), not {self.N}; cost=\"line\" goes up to 65536")
            stride, clearance, lattice, edges, edges_ms = self._lattice_edges("assign_goals(cost=\"path\")", stride, clearance)
        else:
            assign = assign_method(self._ctx, method, self.N)
        if self.initial_positions is None or self.final_positions is None:
            raise ValueError("assign_goals needs both set_initial_states and set_final_states first")
        if self._final_given is None:
            self._final_given = (self.final_positions.copy(), self.final_velocities.copy())
        pf, vf = (a.reshape(self.N, self.D) for a in self._final_given)
        start = self.initial_positions.reshape(1, self.N, self.D)
        sep = float(self.R if min_sep is None else min_sep)
        if cost == "path":
            c, s0 = self._ctx, start[0]
            hops, _, _, _ = c.lattice_distances(self.D, self._obstacles["grid"], stride, edges, c.tensor(s0), c.tensor(pf))
            distances_ms = c.last_pair_ms()
            hops = hops.cpu().numpy().view(np.uint16)
            diff = s0[:, None, :] - pf[None, :, :]
            costs, how = path_costs(hops, (diff * diff).sum(-1), power)
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
        self.final_positions = pf[perm].flatten()
        self.final_velocities = vf[perm].flatten()
        self._dev.pop("p0", None)
        self.trajectories = None
        self.goal_assignment = perm
        self.assignment_info = info
        return perm

    # ------------------------------------------------------------------------------------------------
    # device-side setup
    # ------------------------------------------------------------------------------------------------
    def _limits(self):
        return [self.vel_min, self.vel_max, self.acc_min, self.acc_max, self.jerk_min, self.jerk_max]

    def _space(self):
        return np.concatenate([np.asarray(self.pos_min, float), np.asarray(self.pos_max, float)])

    def _states(self):
        if "p0" not in self._dev:
            # one upload for the four arrays (each is a contiguous (N, D) view of it)
            packed = self._ctx.tensor(np.stack([self.initial_positions, self.initial_velocities, self.final_positions,
                                                self.final_velocities]).reshape(4, self.N, self.D))
            self._dev["p0"], self._dev["v0"], self._dev["pf"], self._dev["vf"] = packed[0], packed[1], packed[2], packed[3]
        d = self._dev
        return d["p0"], d["v0"], d["pf"], d["vf"]

    def _qp_settings(self):
        """the library's default QP settings with the qp_settings overrides that are fields of scp_qp_settings (max_iter0 is not)"""
        known = {k for k, _ in _hip.QpSettings._fields_}
        return _hip.default_settings(**{k: v for k, v in self._qp_overrides.items() if k in known})

    def _warn_joint_qp(self, info):
        """the warning of scp.py:446-447, or ours when constraint generation stopped (max_rounds or the iteration budget) with
        violated rows outside the working set: x then solves the QP over the working set only, not the full one of scp.py:399-451"""
        if info["status_val"] not in (1, 2):
            self._print(f"Warning: OSQP status {info['status']}")
        elif info["unresolved_rows"]:
            self._print(f"Warning: OSQP status constraint generation stopped with {info['unresolved_rows']} violated collision "
                        f"rows outside the working set (max violation {info['max_violation']:.3e})")

    def _ensure_qp(self):
        if self._qp is None:
            self._qp = _hip.QP(self._ctx, self.N, self.K, self.D, self.h, self._qp_settings(),
                               row_capacity=self._qp_row_capacity)
        return self._qp

    def _ensure_pairs(self):
        if self._pairs is None:
            q0, q1 = self.shard.pair_range()
            self._pairs = _hip.PairPass(self._ctx, self.N, self.K, self.D, self.R, self.h, q0, q1)
        return self._pairs

    def _grow_qp(self, need, keep_state=False):
        """Working set outgrew the QP's row capacity: move the solver to a workspace with room for `need` rows
        (keep_state: iterate, duals, working set and rho travel along, so the solve continues unchanged)."""
        old = self._qp
        cap = int(min(self.K * self.shard.pairs, max(need, 2 * old.row_capacity)))
        new = _hip.QP(self._ctx, self.N, self.K, self.D, self.h, old.settings, row_capacity=cap)
        if keep_state:
            new.take_state_of(old)
        else:
            p0, v0, pf, vf = self._states()
            new.set_problem(self._limits(), self._space(), p0, v0, pf, vf)
            self._apply_boxes(new)
        old.close()
        self._qp = new
        return new

    # ------------------------------------------------------------------------------------------------
    # a1: SCP loop (scp.py:131-180)
    # ------------------------------------------------------------------------------------------------
    def generate_trajectories(self, max_iterations=15):
        """Main method to generate collision-free trajectories using SCP (scp.py:131-180)."""
        if self._boxes is not None:
            self._one_rank("generate_trajectories with position boxes")
        if self.native and self.shard.world == 1:
            return self._generate_trajectories_native(max_iterations)
        is_feasible = False
        start_time = time.time()

        self._precompute_constraint_matrices()
        acc = self._solve_initial_trajectory()
        init_guess_positions, _ = self._kinematics(acc, want_vel=False)
        is_feasible = self._fast_check_avoidance_constraints(init_guess_positions)

        iteration = 0
        converged = False
        self._rho_start = 0.0
        self.last_info = {"iterations": [], "qp0": dict(self._last_qp_info)}
        # `is_feasible` is evaluated once and never refreshed inside the loop (scp.py:144, :152)
        while iteration < max_iterations and not converged and not is_feasible:
            self._print(f"SCP Iteration {iteration+1}")
            t_it = time.perf_counter()
            if self.native and self.shard.world > 1 and self.row_free:
                # multi-rank: the iteration natively, split only at its exchange points (same bits as one rank)
                new_acc, it_info = self.scp_iteration_sharded(acc)
                rel_step_norm = it_info["rel_step"]
                self._warn_joint_qp(it_info)
            else:
                new_acc = self._solve_with_avoidance_constraints(acc)
                _, _, rel_step_norm = self._ctx.rel_step(new_acc, acc)  # scp.py:157-159 (no zero guard)
            self._print(rel_step_norm)
            self.last_info["iterations"].append(dict(self._last_qp_info, rel_step=rel_step_norm,
                                                     time_sec=time.perf_counter() - t_it))
            if self.carry_rho:
                self._rho_start = float(self._last_qp_info["rho"])
            if rel_step_norm <= self.convergence_tolerance:
                converged = True
                self._print(f"Converged after {iteration+1} iterations.")
            acc = new_acc
            iteration += 1
            if self.refresh_feasibility and not converged:
                # opt-in (the reference leaves this as a TODO, scp.py:150): stop as soon as the new trajectories are
                # collision free instead of waiting for the relative-step test
                pos_now, _ = self._kinematics(acc, want_vel=False)
                verbose, self.verbose = self.verbose, False
                is_feasible = self._fast_check_avoidance_constraints(pos_now)
                self.verbose = verbose

        self._rho_start = 0.0
        if self.polish:
            # opt-in (not in the reference): one more joint QP, linearised at the final trajectories and solved to
            # polish_eps instead of OSQP's 1e-3.  Every linearised row then holds to ~polish_eps, and a satisfied row
            # eta.(p_i - p_j) >= R implies ||p_i - p_j|| >= R, so the result passes the reference's own R - 0.01 check
            # (scp.py:610) and meets the fixed rows to the same accuracy; the reference's loop stops at OSQP's tolerance,
            # which leaves millimetres of violation in a converged result.
            t_p = time.perf_counter()
            acc = self._solve_with_avoidance_constraints(acc, eps=self.polish_eps)
            self.last_info["polish"] = dict(self._last_qp_info, time_sec=time.perf_counter() - t_p)

        positions, velocities = self._kinematics(acc)
        self.trajectories = {
            "positions": positions.cpu().numpy(),  # Shape (N, K, D)
            "velocities": velocities.cpu().numpy(),
            "accelerations": acc.cpu().numpy(),
        }
        self.last_info.update(converged=converged, initially_feasible=bool(is_feasible), n_iterations=iteration)
        end_time = time.time()
        self._print(f"Trajectory generation completed in {end_time - start_time:.3f} seconds")
        return self.trajectories

    def close(self):
        """Release the device objects.  The native solver and its context go to the process-wide pool (reuse_native) for the
        next SCP object of the same shape; everything else is destroyed.  Called by __del__; the object is unusable after."""
        ctx, nat = getattr(self, "_ctx", None), getattr(self, "_native", None)
        self._native = None
        for name in ("_qp", "_pairs"):
            obj = getattr(self, name, None)
            if obj is not None and hasattr(obj, "close"):
                try:
                    obj.close()
                except Exception:
                    pass
            setattr(self, name, None)
        self._dev = {}
        self._ctx = None
        if ctx is None:
            return
        keep = (nat is not None and self._pool_key is not None and getattr(ctx, "h", None)
                and not getattr(ctx, "options_changed", False))
        if keep:
            with _POOL_LOCK:
                held = _POOL.setdefault(self._pool_key, [])
                if len(held) < _POOL_LIMIT:
                    held.append((ctx, nat))
                    _POOL_STATS["returned"] += 1
                    return
        if nat is not None:
            nat.close()
        ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ensure_native(self):
        if self._native is None:
            self._native = _hip.NativeSolver(self._ctx, self.N, self.K, self.D, self.h, self.R, self._qp_settings(),
                                             row_capacity=self._qp_row_capacity)
        return self._native

    def _native_options(self, max_iterations=15):
        return self._ensure_native().default_options(
            max_iterations=int(max_iterations), max_rounds=self.max_rounds,
            max_iter0=int(self._qp_overrides.get("max_iter0", self._qp_overrides.get("max_iter", 4000))),
            max_iter=int(self._qp_overrides.get("max_iter", 10000)), refresh_feasibility=int(self.refresh_feasibility),
            polish=int(self.polish), working_set_margin=self.working_set_margin, feasibility_tol=self.feasibility_tol,
            polish_eps=self.polish_eps, convergence_tolerance=self.convergence_tolerance, row_free=int(self.row_free),
            carry_rho=int(self.carry_rho))

    def scp_iteration(self, accelerations):
        """ONE pass of the SCP loop body (scp.py:152-166) in one library call (scp_solver_step): linearise around
        `accelerations` (device (N, K, D)), joint QP, relative step.  Returns (new accelerations, info dict).  This is what
        bench.py times; generate_trajectories runs the same code in its native loop."""
        if self.shard.world != 1:
            return self.scp_iteration_sharded(accelerations)
        nat = self._ensure_native()
        self._native_boxes(nat)
        p0, v0, pf, vf = self._states()
        new, rec = nat.step(self._limits(), self._space(), p0, v0, pf, vf, self._native_options(),
                            self._to_device_acc(accelerations))
        info = rec.iteration_dict()
        self._last_qp_info = info
        return new, info

    def scp_iteration_sharded(self, accelerations, exchange_positions=True):
        """The same iteration with the O(N^2 K) passes sharded over the ranks (scp_solver_shard_*): every rank selects /
        checks the pairs of ITS range, the row ids are allgathered (sorted: the single-rank order), the joint QP is
        replicated -- deterministic, so every rank holds the same bits and nothing is broadcast.  With one rank this is
        scp_solver_step phase by phase (same result, bit for bit); the exchanges are the only difference otherwise.

        exchange_positions: the per-shard trajectories of the linearisation point are computed by the rank that owns the
        agents and allgathered (one collective per SCP iteration, the north-star layout); False: every rank integrates
        all agents itself (N K^2 flops, cheaper than the collective below ~10^4 agents)."""
        nat = self._ensure_native()
        self._native_boxes(nat)
        p0, v0, pf, vf = self._states()
        acc = self._to_device_acc(accelerations)
        opts = self._native_options()
        if not opts.row_free:
            raise ValueError("the sharded step is row-free: a rank does not hold the rows of another rank's pairs")
        pos_in = None
        if exchange_positions and not self.shard.alone:
            pos_in, _ = self._kinematics(acc, want_vel=False)  # agent-sharded kinematics + allgather of the trajectories
        q0, q1 = self.shard.pair_range()
        rec, rows = nat.shard_begin(self._limits(), self._space(), p0, v0, pf, vf, opts, acc, pos_in, q0, q1)
        rows, _ = self.shard.allgather_ids(rows)
        more = opts.max_rounds >= 1
        if not more:
            raise ValueError("the sharded step needs max_rounds >= 1")
        while more:
            nat.shard_qp(rows, rec)
            rows, max_v = nat.shard_violations()
            rows, max_v = self.shard.allgather_ids(rows, extra=max_v)
            more = nat.shard_round_done(int(rows.numel()), max_v, rec)
        new = nat.shard_end(rec)
        info = rec.iteration_dict()
        self._last_qp_info = info
        return new, info

    def _generate_trajectories_native(self, max_iterations):
        """generate_trajectories with the loop driven by scp_solver_solve (one C call; the Python-driven loop above makes
        the same library calls in the same order and gives bit-identical results).  The reference's stdout lines are
        printed from the returned records, in the reference's order."""
        start_time = time.time()
        self._drop_bound_attributes()  # l_* / u_* are recomputed when somebody reads them (see __getattr__)
        nat = self._ensure_native()
        self._native_boxes(nat)
        p0, v0, pf, vf = self._states()
        opts = self._native_options(max_iterations)
        acc, pos, vel, res, recs = nat.solve(self._limits(), self._space(), p0, v0, pf, vf, opts)
        qp0 = dict(recs[0].as_dict(), rounds=1, added=[])
        self._last_qp_info = qp0
        if res.qp0_status not in (1, 2):  # Solved / Solved Inaccurate (scp.py:363-365)
            self._print("not feasible")
            raise RuntimeError(f"OSQP failed: {qp0['status']}")
        if not res.initially_feasible:
            self._print(f"Avoidance constraint violation at timestep {res.first_violation_k} between vehicles "
                        f"{res.first_violation_i} and {res.first_violation_j}: distance = {res.first_violation_distance:.3f}")
        its = []
        for n, r in enumerate(recs[1:1 + res.n_iterations]):
            d = r.iteration_dict()
            self._print(f"SCP Iteration {n+1}")
            self._warn_joint_qp(d)
            self._print(d["rel_step"])
            if d["rel_step"] <= self.convergence_tolerance:
                self._print(f"Converged after {n+1} iterations.")
            its.append(d)
        self.last_info = {"iterations": its, "qp0": qp0, "converged": bool(res.converged),
                          "initially_feasible": bool(res.feasible_at_exit), "n_iterations": int(res.n_iterations)}
        if res.polished:
            r = recs[res.n_records - 1]
            self.last_info["polish"] = dict(r.as_dict(), time_sec=float(r.time_sec))
        if its:
            self._last_qp_info = its[-1]
        # acc, pos, vel are the three slices of one device buffer: one device-to-host copy for all of them
        host = acc._base.cpu().numpy() if acc._base is not None else None
        self.trajectories = {
            "positions": host[1] if host is not None else pos.cpu().numpy(),  # Shape (N, K, D)
            "velocities": host[2] if host is not None else vel.cpu().numpy(),
            "accelerations": host[0] if host is not None else acc.cpu().numpy(),
        }
        self._print(f"Trajectory generation completed in {time.time() - start_time:.3f} seconds")
        return self.trajectories

    # ------------------------------------------------------------------------------------------------
    # a2: fixed rows (scp.py:182-321) -- bounds only; the matrices are the shared K-column blocks
    # ------------------------------------------------------------------------------------------------
    def _precompute_constraint_matrices(self):
        p0, v0, pf, vf = self._fill_bound_attributes()
        self._ensure_qp().set_problem(self._limits(), self._space(), p0, v0, pf, vf)
        self._apply_boxes(self._qp)

    _BOUND_ATTRS = ("l_jerk", "u_jerk", "l_acc", "u_acc", "l_vel", "u_vel", "l_pos", "u_pos")

    def _drop_bound_attributes(self):
        for name in self._BOUND_ATTRS:
            self.__dict__.pop(name, None)

    def __getattr__(self, name):
        # The native loop does not need the reference's l_* / u_* arrays (scp.py:189-257) on the host; they are built on
        # first access (one small kernel + a device-to-host copy) instead of once per solve.
        if (name in SCP._BOUND_ATTRS and self.__dict__.get("initial_positions") is not None
                and self.__dict__.get("final_positions") is not None):
            self._fill_bound_attributes()
            return self.__dict__[name]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _fill_bound_attributes(self):
        """l_* / u_* attributes of the reference (scp.py:189-257), bitwise equal; returns the device states."""
        N, K, D = self.N, self.K, self.D
        p0, v0, pf, vf = self._states()
        lo, hi = self._ctx.fixed_bounds(N, K, D, self.h, self._limits(), self._space(), p0, v0, pf, vf)
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
        nj, na = N * (K - 1) * D, N * K * D
        self.l_jerk, self.u_jerk = lo[:nj], hi[:nj]
        self.l_acc, self.u_acc = lo[nj:nj + na], hi[nj:nj + na]
        self.l_vel, self.u_vel = lo[nj + na:nj + 2 * na], hi[nj + na:nj + 2 * na]
        self.l_pos, self.u_pos = lo[nj + 2 * na:], hi[nj + 2 * na:]
        # size checks of the reference (scp.py:265-299)
        assert self.l_acc.shape == self.u_acc.shape == (D * N * K,)
        assert self.l_jerk.shape == self.u_jerk.shape == (D * N * (K - 1),)
        assert self.l_vel.shape == self.u_vel.shape == (D * N * K,)
        assert self.l_pos.shape == self.u_pos.shape == (D * N * K,)
        return p0, v0, pf, vf

    # ------------------------------------------------------------------------------------------------
    # a3: QP#0 (scp.py:323-369)
    # ------------------------------------------------------------------------------------------------
    def _solve_initial_trajectory(self):
        """Solve initial trajectory without avoidance constraints.  Returns a device tensor (N, K, D)."""
        qp = self._ensure_qp()
        qp.update_settings(max_iter=int(self._qp_overrides.get("max_iter0", self._qp_overrides.get("max_iter", 4000))))
        qp.reset(None)
        info = qp.solve()
        info["status_val"], info["iter"] = self.shard.broadcast_ints([info["status_val"], info["iter"]])
        info["status"] = _hip.STATUS_TEXT.get(info["status_val"], str(info["status_val"]))
        self._last_qp_info = dict(info, rounds=1, added=[])
        if info["status_val"] not in (1, 2):  # Solved / Solved Inaccurate (scp.py:363-365)
            self._print("not feasible")
            raise RuntimeError(f"OSQP failed: {info['status']}")
        x = qp.solution()
        self.shard.broadcast(x)
        return x

    # ------------------------------------------------------------------------------------------------
    # a4 / a7: kinematics (scp.py:371-397, :559-595)
    # ------------------------------------------------------------------------------------------------
    def _kinematics(self, acc, want_vel=True):
        """Agent-sharded kinematics + allgather of the per-shard trajectories (device tensors)."""
        p0, v0, _, _ = self._states()
        i0, i1 = self.shard.agent_range()
        n = i1 - i0
        if self.shard.world == 1:
            return self._ctx.kinematics(self.N, self.K, self.D, self.h, acc, p0, v0, want_vel)
        pos, vel = self._ctx.kinematics(n, self.K, self.D, self.h, acc[i0:i1].contiguous(), p0[i0:i1].contiguous(),
                                        v0[i0:i1].contiguous(), want_vel)
        pos = self.shard.allgather_positions(pos)
        vel = self.shard.allgather_positions(vel) if want_vel else None
        return pos, vel

    def _to_device_acc(self, accelerations):
        import torch

        if isinstance(accelerations, torch.Tensor):
            return accelerations.reshape(self.N, self.K, self.D).to(self._ctx.tdev, torch.float64).contiguous()
        return self._ctx.tensor(np.asarray(accelerations, dtype=float).reshape(self.N, self.K, self.D))

    def _compute_positions_velocities(self, accelerations):
        """positions, velocities (N, K, D) numpy arrays from accelerations (scp.py:371-397)."""
        pos, vel = self._kinematics(self._to_device_acc(accelerations))
        return pos.cpu().numpy(), vel.cpu().numpy()

    def _accelerations_to_positions_velocities(self, accelerations_flat):
        """Same recurrences on the flat vector (scp.py:559-595); bitwise equal to the method above."""
        return self._compute_positions_velocities(accelerations_flat)

    # ------------------------------------------------------------------------------------------------
    # a5: pairwise linearisation (scp.py:453-557)
    # ------------------------------------------------------------------------------------------------
    def _add_collision_constraints(self, previous_solution):
        """Compact form of A_collision: returns (eta (rows, D), l_collision (rows,), u_collision (rows,)) as numpy
        arrays for THIS rank's pair range, rows in the reference's k-major / i / j>i order.  Row r of the
        reference's matrix is eta_r[d] h^2 (k-m-.5) on a_i[m] and the negative on a_j[m], m < k."""
        acc = self._to_device_acc(previous_solution)
        pos, _ = self._kinematics(acc, want_vel=False)
        p0, v0, _, _ = self._states()
        pp = self._ensure_pairs()
        pp.linearize(pos, p0, v0, self.working_set_margin)
        l = pp.l_rows().cpu().numpy()
        return pp.eta_rows().cpu().numpy(), l, np.full(l.shape, np.inf)

    # ------------------------------------------------------------------------------------------------
    # a6: joint QP with collision rows (scp.py:399-451)
    # ------------------------------------------------------------------------------------------------
    def _solve_with_avoidance_constraints(self, accelerations_flat, eps=None):
        """Solve with collision avoidance constraints.  Takes / returns a device tensor (N, K, D).
        eps: termination tolerances of this one QP (the polish step), None = the solver's settings.

        The joint QP over ALL collision rows is solved by exact constraint generation: ADMM runs on the fixed rows
        and a working set (rows with dist - R < working_set_margin at the linearisation point); a full pairwise
        pass then checks every row at the solution and violated rows join the working set until none is left."""
        acc = self._to_device_acc(accelerations_flat)
        p0, v0, _, _ = self._states()
        pp = self._ensure_pairs()
        qp = self._ensure_qp()
        max_iter = int(self._qp_overrides.get("max_iter", 10000))  # scp.py:442
        saved = (qp.settings.eps_abs, qp.settings.eps_rel, qp.settings.max_iter)
        try:
            x, info, total, added, max_v = self._joint_qp_rounds(acc, p0, v0, pp, qp, max_iter, eps)
        finally:
            # the per-QP tolerances (polish) and the per-round iteration budget must not outlive this call, whatever
            # happens inside it (self._qp: the solver may have moved to a larger workspace meanwhile)
            self._qp.update_settings(eps_abs=saved[0], eps_rel=saved[1], max_iter=saved[2])
        self._last_qp_info = dict(info, **total, rounds=len(added), added=added, unresolved_rows=added[-1],
                                  max_violation=max_v)
        self._warn_joint_qp(self._last_qp_info)
        return x

    def _joint_qp_rounds(self, acc, p0, v0, pp, qp, max_iter, eps):
        """The rounds of _solve_with_avoidance_constraints: linearise, working set, ADMM, violations pass, repeat."""
        if eps is not None:
            qp.update_settings(eps_abs=float(eps), eps_rel=float(eps))
            max_iter = max(max_iter, 40000)  # three more digits take a few times OSQP's budget

        prev_pos, _ = self._kinematics(acc, want_vel=False)
        rows, _, _ = pp.linearize(prev_pos, p0, v0, self.working_set_margin)
        if self._holds is not None:
            # repair_conflicts: the held rows of the planes become their fixed half-planes and all of them join the working set
            # (marked in the bitmap, so no violations pass adds their own-direction form again)
            import torch

            held = pp.apply_holds(*self._holds, p0, v0)
            if held.numel():
                rows = torch.cat([rows, held]).sort().values
        w_eta, w_l = pp.gather(rows)
        rows, w_eta, w_l = self.shard.allgather_rows(rows, w_eta, w_l)

        qp.reset(acc)
        if self._rho_start > 0.0:
            qp.set_rho(self._rho_start)
        try:
            qp.add_rows(rows, w_eta, w_l)
        except _hip.HipError as e:
            if e.code != _hip.SCP_ERR_CAPACITY:
                raise
            qp = self._grow_qp(int(rows.numel()))
            qp.reset(acc)
            if self._rho_start > 0.0:
                qp.set_rho(self._rho_start)
            qp.add_rows(rows, w_eta, w_l)

        used = 0
        added = []
        info = None
        x = acc
        max_v = 0.0
        total = {"iter": 0, "cg_iters_total": 0, "rho_updates": 0, "solve_ms": 0.0, "persist_launches": 0,
                 "persist_gave_up": 0, "rho_switches_in_kernel": 0}
        pipes = set()
        for rnd in range(self.max_rounds):
            qp.update_settings(max_iter=max(max_iter - used, 1))
            info = qp.solve()
            # rank 0's counters drive the loop on every rank (see Shard.broadcast_ints)
            info["status_val"], info["iter"] = self.shard.broadcast_ints([info["status_val"], info["iter"]])
            info["status"] = _hip.STATUS_TEXT.get(info["status_val"], str(info["status_val"]))
            used += info["iter"]
            for k in total:
                total[k] += info[k]
            pipes.update(info["pipeline"].split("+"))
            x = qp.solution()
            self.shard.broadcast(x)
            pos_new, _ = self._kinematics(x, want_vel=False)
            new_rows, max_v = pp.violations(pos_new, p0, v0, self.feasibility_tol)
            n_eta, n_l = pp.gather(new_rows)
            new_rows, n_eta, n_l = self.shard.allgather_rows(new_rows, n_eta, n_l)
            added.append(int(new_rows.numel()))
            if new_rows.numel() == 0 or used >= max_iter:
                break
            try:
                qp.add_rows(new_rows, n_eta, n_l)
            except _hip.HipError as e:
                if e.code != _hip.SCP_ERR_CAPACITY:
                    raise
                # continue in a larger workspace: the state of the solve travels along
                qp = self._grow_qp(qp.n_rows + int(new_rows.numel()), keep_state=True)
                qp.add_rows(new_rows, n_eta, n_l)
        total["pipeline"] = "+".join(n for n in _hip.PIPELINES if n in pipes) or "none"
        return x, info, total, added, max_v

    # ------------------------------------------------------------------------------------------------
    # a8: avoidance check (scp.py:597-615)
    # ------------------------------------------------------------------------------------------------
    def _fast_check_avoidance_constraints(self, positions):
        """True when every pair keeps ||p_i - p_j|| >= R - 0.01 at every stored sample; otherwise prints the first
        violation in k -> i -> j order exactly like the reference (scp.py:602-615)."""
        import torch

        pos = positions if isinstance(positions, torch.Tensor) else self._ctx.tensor(np.asarray(positions, dtype=float))
        pos = pos.reshape(self.N, self.K, self.D).contiguous()
        q0, q1 = self.shard.pair_range()
        _, first, _, _ = self._ctx.check_avoidance(self.N, self.K, self.D, self.R, pos, q0, q1)
        first = self.shard.all_min_int(first)
        if first >= (1 << 63) - 1:
            return True
        pairs = self.shard.pairs
        k, q = divmod(first, pairs)
        i, j = pair_from_index(q, self.N)
        d = float(torch.linalg.vector_norm(pos[i, k] - pos[j, k]).item())
        self._print(
            f"Avoidance constraint violation at timestep {k} between vehicles {i} and {j}: distance = {d:.3f}"
        )
        return False

    # ------------------------------------------------------------------------------------------------
    # post-solve validation: one device pass over all pairs + the fixed rows on the host copy
    # ------------------------------------------------------------------------------------------------
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
            if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or not 0 <= delay <= self.K:
                raise ValueError(f"delay={delay!r}: the largest delay is a whole number of steps in [0, K = {self.K}]")
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")
        N, K, D, h = self.N, self.K, self.D, self.h
        a, v, p = (self.trajectories[k] for k in ("accelerations", "velocities", "positions"))
        q0, q1 = self.shard.pair_range()
        c = self._ctx
        dev = (c.tensor(p), c.tensor(v), c.tensor(a)) if continuous else (c.tensor(p),)  # one upload for every pass below
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
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")
        c = self._ctx
        if dev is None:
            dev = tuple(c.tensor(self.trajectories[k]) for k in ("positions", "velocities", "accelerations"))
        st = c.check_corridor(self.N, self.K, self.D, self.h, self._corridor["grid"], self._corridor["cells"], *dev, tol=float(tol))
        seg = np.where(st["segment"] == np.uint32(_hip.NO_INDEX), -1, st["segment"].astype(np.int64))
        n_out, n_blk = int(st["n_outside"].sum()), int(st["n_blocked"].sum())
        return {"vehicles": {"max_excess": st["max_excess"].copy(), "segment": seg, "n_blocked": st["n_blocked"].astype(np.int64),
                             "n_outside": st["n_outside"].astype(np.int64)},
                "n_outside": n_out, "n_blocked": n_blk, "max_excess": float(st["max_excess"].max()),
                "worst_vehicle": int(np.argmax(st["max_excess"])), "inside": n_out == 0 and n_blk == 0,
                "check_ms": c.last_pair_ms()}

    def _obstacle_field(self, who, gap):
        """the device field of the current obstacles at `gap` (made once per set_obstacles), and the device time it took"""
        self._one_rank(who)
        if self._obstacles is None:
            raise ValueError(f"{who} needs set_obstacles first")
        if isinstance(gap, bool) or gap not in (0, 1):
            raise ValueError(f"gap={gap!r}: 0 (between cells) or 1 (between the closed cubes of the cells)")
        cache = self._obstacles.setdefault("field", {})
        if gap not in cache:
            field = self._ctx.obstacle_distance(self.D, self._obstacles["grid"], self._obstacles["occ"], int(gap))
            cache[gap] = (field, self._ctx.last_pair_ms())
        return cache[gap]

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
        self._one_rank("obstacle_clearance")
        if self._obstacles is None:
            raise ValueError("obstacle_clearance needs set_obstacles first")
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")
        if isinstance(pieces, bool) or not isinstance(pieces, (int, np.integer)) or not 1 <= pieces <= _hip.OBSTACLE_MAX_PIECES:
            raise ValueError(f"pieces={pieces!r}: a whole number in [1, {_hip.OBSTACLE_MAX_PIECES}]")
        c, ob = self._ctx, self._obstacles
        field, field_ms = self._obstacle_field("obstacle_clearance", 1)
        if dev is None:
            dev = tuple(c.tensor(self.trajectories[k]) for k in ("positions", "velocities", "accelerations"))
        st, step_min = c.obstacle_clearance(self.N, self.K, self.D, self.h, ob["grid"], ob["sat"], field, int(pieces), *dev)
        check_ms = c.last_pair_ms()
        cell = float(ob["grid"].cell)

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

    # ------------------------------------------------------------------------------------------------
    # repair of between-sample conflicts (not in the reference): holds, DESIGN.md section 3.7
    # ------------------------------------------------------------------------------------------------
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
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")
        if self.shard.world != 1:
            raise ValueError("repair_conflicts supports one rank only (world_size == 1)")
        t_start = time.perf_counter()
        N, K, D, h, c = self.N, self.K, self.D, self.h, self._ctx
        p0, v0, pf, vf = self._states()
        traj = self.trajectories
        acc = c.tensor(traj["accelerations"])
        dev = (c.tensor(traj["positions"]), c.tensor(traj["velocities"]), acc)
        cost_before = float(np.sum(traj["accelerations"] ** 2))
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

    # ------------------------------------------------------------------------------------------------
    # staggered starts (not in the reference): pair-lag masks and a greedy launch schedule, DESIGN.md section 3.7
    # ------------------------------------------------------------------------------------------------
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
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")
        if self.shard.world != 1:
            raise ValueError("stagger_starts supports one rank only (world_size == 1)")
        top = min(self.K, _hip.MAX_LAG)
        if isinstance(max_delay, bool) or not isinstance(max_delay, (int, np.integer)) or not 0 <= max_delay <= top:
            raise ValueError(f"max_delay={max_delay!r}: the largest delay is a whole number of steps in [0, min(K, 63) = {top}]")
        if self.N > _hip.SCHEDULE_MAX_N:
            raise ValueError(f"stagger_starts schedules at most {_hip.SCHEDULE_MAX_N} vehicles")
        if order is not None:
            order = np.asarray(order, dtype=np.int64).reshape(-1)
            if order.size != self.N or not np.array_equal(np.sort(order), np.arange(self.N)):
                raise ValueError("order must be a permutation of 0 .. N-1")
        if isinstance(search, bool) or not isinstance(search, (int, np.integer)) or not 0 <= search <= _hip.SCHEDULE_MAX_BATCH:
            raise ValueError(f"search={search!r}: the candidate orders per round are an int in [0, {_hip.SCHEDULE_MAX_BATCH}]")
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or rounds < 1:
            raise ValueError(f"rounds={rounds!r}: an int >= 1")
        if objective not in _hip.SCHEDULE_OBJECTIVES:
            raise ValueError(f"objective={objective!r}: one of {sorted(_hip.SCHEDULE_OBJECTIVES)}")
        t_start = time.perf_counter()
        N, K, D, h, c = self.N, self.K, self.D, self.h, self._ctx
        S = int(max_delay)
        host = tuple(self.trajectories[k] for k in ("positions", "velocities", "accelerations"))
        dev = tuple(c.tensor(x) for x in host)
        before = c.check_separation(N, K, D, h, self.R, *dev)
        mask = c.lag_conflicts(N, K, D, h, self.R, *dev, S, device=True)
        lag_ms = c.last_pair_ms()
        if search:
            delays, st, schedule_ms, found = self._search_start_orders(mask, S, order, int(search), int(rounds), seed, objective)
        else:
            delays, st = c.schedule_starts(mask, S, order)
            schedule_ms = c.last_pair_ms()
        pos, vel, acc = staggered_fleet(*host, h, delays)
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

    # ------------------------------------------------------------------------------------------------
    # visualisation passthroughs (scp.py:644-840): host-side matplotlib over the stored numpy trajectories
    # ------------------------------------------------------------------------------------------------
    def visualize_trajectories(self, show_animation=False, save_path="trajectories.pdf"):
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")  # scp.py:646-647
        from ..viz.plot_trajectories import plot_trajectories

        return plot_trajectories(self, show=show_animation, save_path=save_path)

    def visualize_time_snapshots(self, num_snapshots=5, save_path=None):
        if self.trajectories is None:
            raise ValueError("Trajectories not generated yet")  # scp.py:782-783
        from ..viz.plot_trajectories import plot_time_snapshots

        return plot_time_snapshots(self, num_snapshots=num_snapshots, save_path=save_path)


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


def pair_from_index(q, N):
    """Lexicographic pair index -> (i, j), i < j (host helper, exact integer arithmetic)."""
    i = int(((2 * N - 1) - np.sqrt(float((2 * N - 1) ** 2 - 8 * q))) // 2)
    i = max(0, min(i, N - 2))
    off = lambda a: a * (2 * N - a - 1) // 2
    while off(i) > q:
        i -= 1
    while i < N - 2 and off(i + 1) <= q:
        i += 1
    return i, int(q - off(i) + i + 1)
