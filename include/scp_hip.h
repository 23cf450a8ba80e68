/*
 * scp_hip.h -- C-ABI of the MI355X (gfx950) SCP hot path: libscp_hip.so
 *
 * Drop-in boundary for /root/reference/src/path_planning/solvers/scp.py (class SCP).  The reference is
 * pure Python with no FFI of its own; each entry point below replaces the body of
 * one reference method and is what a ctypes binding inside that method would call (INTEGRATION.md shows the
 * stub).  All `double*` / `int64_t*` arguments are DEVICE pointers unless marked [host]; the caller owns
 * them (torch-ROCm tensors in our host code).  No torch types cross this boundary.
 *
 * Conventions
 *   - boundary arrays use the reference layout: accelerations/positions/velocities are [N][K][D]
 *     (flat index (i*K + k)*D + d, scp.py:15-26, :168, :581-582); states are [N][D].
 *   - D is 2 (the reference) or 3 (extension).
 *   - collision rows are numbered as the reference orders them: r = k*pairs + q, q = lexicographic index of
 *     (i, j), i < j  (scp.py:487-496); pairs = N(N-1)/2.
 *   - every function returns 0 on success or a negative scp_status; scp_last_error(ctx) gives the text.
 *   - all work is enqueued on the ctx's HIP stream; functions that return host values synchronise it.
 *   - a ctx and the objects created from it must be used from one thread at a time (one ctx per rank).
 */
#ifndef SCP_HIP_H
#define SCP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCP_ABI_VERSION 7

typedef enum scp_status {
  SCP_OK = 0,
  SCP_ERR_INVALID = -1,   /* bad argument (shape, NULL pointer, D not in {2,3}) */
  SCP_ERR_HIP = -2,       /* a HIP runtime call failed */
  SCP_ERR_CAPACITY = -3,  /* a caller-provided buffer is too small (row capacity, workspace) */
  SCP_ERR_STATE = -4      /* call order violated (e.g. solve before set_problem) */
} scp_status;

typedef struct scp_ctx scp_ctx;
typedef struct scp_qp scp_qp;

/* Result of a pairwise pass; lives in DEVICE memory (32 bytes), written by scp_linearize_pairs,
 * scp_check_avoidance and scp_collision_violations. */
typedef struct scp_pair_stats {
  double min_dist;            /* min over processed rows of ||p_i[k] - p_j[k]|| (before the dist:=1 rule) */
  uint64_t first_violation;   /* smallest row id with dist < R - 0.01 (scp.py:610), UINT64_MAX if none */
  uint64_t n_selected;        /* rows selected (may exceed the capacity of the output list: then only the first
                                 `capacity` ids were stored, the call still returns SCP_OK and the caller repeats it
                                 with a larger list) */
  double max_violation;       /* scp_collision_violations: max over rows of l_r - (A x)_r */
} scp_pair_stats;

/* Settings of the QP solver.  Defaults (scp_qp_default_settings) are OSQP's, because the reference calls
 * osqp with its defaults (scp.py:360) resp. max_iter=10000 (scp.py:442). */
typedef struct scp_qp_settings {
  double rho;                    /* 0.1 */
  double sigma;                  /* 1e-6 */
  double alpha;                  /* 1.6 */
  double rho_eq_scale;           /* 1e3: rho multiplier on equality rows */
  double eps_abs;                /* 1e-3 */
  double eps_rel;                /* 1e-3 */
  int32_t max_iter;              /* 4000 (QP#0, scp.py:360) / 10000 (scp.py:442) */
  int32_t check_termination;     /* 25 */
  int32_t adaptive_rho;          /* 1 */
  int32_t adaptive_rho_interval; /* 50 (iterations; a multiple of check_termination.  OSQP's default is a wall-clock rule;
                                    50 is the measured choice of profiles/r03_rho_interval_sweep.txt) */
  double adaptive_rho_tolerance; /* 5 */
  int32_t cg_iters;              /* 1: PCG steps per ADMM step (fixed count >= 1, warm started at x) */
  int32_t use_mfma;              /* 1: column kernels, H_f^{-1} on v_mfma_f64_16x16x4_f64: the single-step pipeline
                                    (cg_iters == 1, K <= 1024) and QP#0's column-local kernel (K <= 120, any cg_iters);
                                    everything else, cg_iters > 1 with collision rows among it, runs as with 2;
                                    2: one MFMA product per launch (generic path); 0: VALU products */
  double rho_col_scale;          /* 10: rho of the collision rows = rho * rho_col_scale (like OSQP's per-row rho,
                                    which the reference gets x 1e3 on equality rows only).  Measured at 1024 x 50:
                                    the same SCP iterates with 3.5 x fewer ADMM iterations than scale 1 */
  double eps_prim_inf;           /* 1e-4: OSQP's primal infeasibility tolerance; the certificate (delta-y test) is
                                    evaluated at every termination check; <= 0 disables it */
  int32_t persistent;            /* 1: with cg_iters == 1, K <= 64 and at most one block of agents per compute unit, all ADMM
                                    steps between two termination checks run in ONE persistent launch (solver state on chip,
                                    two grid-wide exchanges per step).  Which kernel: 2-D up to 2048 agents the lean kernel
                                    with 8 agents per workgroup, up to 4096 with 16; 3-D up to 1024 agents the 4-agent kernel
                                    of round 2, up to 2048 the lean one with 8.  2 / 3 / 4: force the lean 16-agent / lean
                                    8-agent / round-2 kernel where it fits (tests, measurements); 0: three launches per step.
                                    Same arithmetic up to the association of sums */
  int32_t check_fine;            /* 5: adaptive check cadence.  After a termination check that finds both residuals within
                                    check_fine_ratio x their tolerances, or that changes rho, the next check comes after
                                    check_fine steps (a divisor of check_termination) instead of check_termination: a QP
                                    no longer pays up to 24 surplus steps for every check interval it does not need, and
                                    pays the fine checks (about one step each inside the persistent kernels) only near the
                                    end (profiles/r03_check_cadence.txt).  Applies to QPs with collision rows (QP#0 keeps
                                    the fixed cadence: a better converged start saves the first joint QP more) of up to
                                    4096 columns (beyond, it measured slower: profiles/r03_check_cadence.txt).  0, or a value that does not
                                    divide check_termination: fixed cadence */
  double check_fine_ratio;       /* 2 */
} scp_qp_settings;

/* [host] result of scp_qp_solve */
typedef struct scp_qp_info {
  int32_t status_val;   /* OSQP codes: 1 solved, 2 solved inaccurate (max_iter reached, 10 x eps met),
                           -2 maximum iterations reached, -3 primal infeasible */
  int32_t iter;         /* ADMM iterations of this call */
  int32_t rho_updates;
  int32_t cg_iters_total;
  int64_t working_rows;
  double r_prim, r_dual;
  double rho;
  double solve_ms;      /* device time of this call (HIP events on the ctx stream) */
  int32_t pipeline;     /* which pipelines ran the ADMM iterations of this call: OR of (1 << scp_qp_pipeline) */
  int32_t persist_launches;       /* persistent launches of this call that ran (their steps are in `iter`) */
  int32_t persist_gave_up;        /* persistent launches that timed out on a workgroup and left without writing state
                                     back; the iterations were repeated on the three-launch pipeline */
  int32_t rho_switches_in_kernel; /* adaptive-rho updates made inside a persistent launch (included in rho_updates) */
} scp_qp_info;

/* the pipelines of scp_qp_solve (bit numbers of scp_qp_info.pipeline / scp_qp_record.pipeline) */
typedef enum scp_qp_pipeline {
  SCP_PIPE_QP0 = 0,        /* fixed rows only: all steps up to a check in one column-local launch */
  SCP_PIPE_PERSIST = 1,    /* persistent single-step kernel, one wave per agent, 16/D agents per workgroup */
  SCP_PIPE_PERSIST16 = 2,  /* its lean form: 16 agents per workgroup (2-D, 2048 < N <= 4096) */
  SCP_PIPE_CG1 = 3,        /* single-step pipeline, three launches per ADMM step */
  SCP_PIPE_CG1_BIGK = 4,   /* the same with one workgroup per column (K > 120) */
  SCP_PIPE_FUSED = 5,      /* retired, never set (cg_iters > 1 runs SCP_PIPE_GENERIC); kept so that no other bit moves */
  SCP_PIPE_GENERIC = 6,    /* one product per launch */
  SCP_PIPE_PERSIST8L = 7   /* the lean kernel's state diet with 8 agents per workgroup (3-D, 1024 < N <= 2048) */
} scp_qp_pipeline;

int scp_abi_version(void);
/* How host threads wait for a kernel's completion word (process-wide): 0 = spin (default: lowest latency, one core per
 * waiting thread), 1 = spin ~20 us, then poll from 20 us sleeps (many solver threads on few cores), 2 = sleep between polls
 * from the first miss (more solver threads than cores). */
void scp_set_host_wait(int mode);

/* Plane stride (in doubles) of the SoA eta array of scp_linearize_pairs: K*nq rounded up to an even count so
 * that every plane starts 16-byte aligned. */
static inline int64_t scp_eta_stride(int64_t K, int64_t nq) { return (K * nq + 1) & ~(int64_t)1; }

/* ---- context -------------------------------------------------------------------------------------- */
int scp_ctx_create(int device, void* hip_stream /* hipStream_t or NULL for the default stream */, scp_ctx** out);
void scp_ctx_destroy(scp_ctx* ctx);
const char* scp_last_error(const scp_ctx* ctx);
int scp_ctx_synchronize(scp_ctx* ctx);
/* device time (ms) of the most recent pairwise kernel launch alone (scp_linearize_pairs, scp_check_avoidance,
 * scp_collision_violations), from HIP events recorded on the ctx stream around that launch; synchronises. */
int scp_ctx_last_pair_ms(scp_ctx* ctx, float* ms);
/* Per-context switches; results never depend on them.
 *   "kernel_timing" (default 1): HIP events around the pairwise kernels and the QP solves -- two queue packets each, ~25 per
 *     complete solve.  0: none are recorded; scp_ctx_last_pair_ms and the records' linearize_ms / violations_ms then read 0
 *     and solve_ms is the host's wall clock around the solve.  For many concurrent solver streams on one GPU
 *     (compute-trajectories-batch), where every packet of a stream costs dispatch latency.
 *   "single_launch_passes" (default 1): pairwise passes of small problems (<= 2 M collision rows) run as ONE launch -- staging
 *     from the [N][K][D] arrays, reduction, sorted row list and host-visible stats in the pass kernel's last workgroup.
 *     0: prep kernel + pass + compaction launches as for large problems.
 *   "fused_step_prep" (default 1): where a pass runs as several launches, its prep launch derives the positions it stages --
 *     from acc_in at the start of scp_solver_step, from the QP's time-major solution in every round -- instead of following
 *     a layout change and a kinematics launch.  0: those launches run separately.
 *   "delay_lag_chunk", "delay_time_chunk" (default 0: chosen by the call): the lags / the global segments one workgroup of
 *     scp_delay_margins covers; developer switches for tests and measurements.
 *   "lagc_lag_chunk", "lagc_time_chunk" (default 0: chosen by the call): the same two of scp_lag_conflicts.
 *   "stg_batch_threads" (default 0: chosen by the call from N; or 256 or 1024): threads per workgroup of
 *     scp_schedule_starts_batch; a developer switch.
 *   "stg_batch_transposed" (default -1: chosen by the call, from 16 candidates on; 0 never; 1 always): scp_schedule_starts_batch
 *     first writes a transposed copy of the masks (N^2 words in the context's workspace) and reads the masks' columns from
 *     its rows; a developer switch.
 *   "ref_path_threads" (default 0: chosen by the call; or 64, 256, 512 or 1024): threads per workgroup of scp_reference_paths,
 *     scp_reference_paths_weighted, scp_reference_paths_shared, scp_lattice_distances and scp_lattice_costs; a developer
 *     switch.
 *   "shorten_threads" (default 0: chosen by the call; or 64, 128 or 256): threads per workgroup of scp_shorten_paths (one
 *     wave per vehicle, so 1, 2 or 4 vehicles per workgroup); a developer switch.
 *   "raster_item_cells" (default 0: 1024; or 64 .. 2^24): the most cells of one work item (one workgroup) of
 *     scp_rasterize_shapes; a developer switch. */
int scp_ctx_set_option(scp_ctx* ctx, const char* key, int value);
/* The near form of scp_collision_violations_at: only the pairs close enough to be violated are evaluated (a uniform grid
 * per time step), with the exhaustive pass as the fallback when no examined row is close to active or an input is not
 * finite -- the results are the exhaustive pass's, bit for bit.  mode 0: never; 1 (default): for problems too large for
 * the one-launch passes, when feas_tol >= 0 and a time step's tables fit the LDS; 2: wherever it can run, small problems
 * included (tests, A/B runs). */
int scp_ctx_set_near_pass(scp_ctx* ctx, int mode);
/* Near passes this ctx has run, and how many of them were followed by the exhaustive pass. */
int scp_ctx_near_pass_counts(scp_ctx* ctx, uint64_t* n_near /* [host] */, uint64_t* n_fell_back /* [host] */);
/* Test hook: the first `words` words of the scratch bitmap of the violations passes (all zero between calls).  Synchronises. */
int scp_ctx_peek_scratch_map(scp_ctx* ctx, uint32_t* out /* [host] */, int64_t words);
/* Test hook: fills every device workspace the ctx owns at this moment, to its current size, with `word` -- the time-major
 * copy, the compaction totals, the per-workgroup partials and row sub-lists of the one-launch passes, the workspaces of the
 * scenario generator, of the continuous-time / hold / reference-path / distance-field calls, of the line check, of the wide
 * auction and of the rasteriser, and the 64 partial sums of scp_rel_step on the device and in pinned host memory.  Every
 * call writes each of these words before it reads it, so no result may change.  NOT touched: the scratch bitmap of the
 * violations passes, the ticket / counter block, scp_rel_step's ticket and completion word and the stats mirror -- what
 * they hold between calls is relied upon.  Enqueued on the ctx's stream; allocates nothing. */
int scp_ctx_debug_fill(scp_ctx* ctx, uint32_t word);
/* [host] what scp_ctx_debug_state reports */
typedef struct scp_ctx_state {
  uint32_t ticket[16];       /* the block of device words that lives as long as the ctx: [0] last-workgroup ticket of the
                                one-launch pairwise passes, [1] and [2] those of the QP's checks and row build (all three zero
                                between calls), [3] number of the latest recomputing violations pass that staged a value that
                                was not finite, [4, 8) the two result words of scp_schedule_starts_batch, [8, 10) / [10, 12) /
                                [12, 14) / [14, 16) the 64-bit counters behind scp_ctx_last_lag_solved / _delay_solved /
                                _separation_solved / _clearance_solved */
  uint32_t rel_ticket;       /* last-workgroup ticket of scp_rel_step (zero between calls) */
  uint32_t reserved;
  uint64_t cmp_map_nonzero;  /* words of the violations passes' scratch bitmap that are not zero (none between calls) */
  uint64_t tm_bytes, cmp_map_bytes, cmp_tot_bytes, wg_rows_bytes, gen_ws_bytes, sep_ws_bytes, asg_ws_bytes, asgw_ws_bytes,
      rast_ws_bytes, rast_host_bytes; /* current size of each grown-on-demand buffer of the ctx (0: never allocated) */
} scp_ctx_state;
/* Test hook: the words above, after the ctx's stream has drained. */
int scp_ctx_debug_state(scp_ctx* ctx, scp_ctx_state* out /* [host] */);

/* ---- a4 / a7: SCP._compute_positions_velocities (scp.py:371-397),
 *               SCP._accelerations_to_positions_velocities (scp.py:559-595) ---------------------------
 * pos[i][k] = p0_i + (h*k) v0_i + sum_{j<k} (h*h*(k-j-0.5)) a_i[j],  vel[i][k] = v0_i + sum_{j<k} h a_i[j],
 * summed in the reference's order without FMA contraction (bitwise equal to the reference). */
int scp_kinematics(scp_ctx* ctx, int N, int K, int D, double h, const double* acc, const double* p0,
                   const double* v0, double* pos_out, double* vel_out);

/* ---- a2: bounds of SCP._precompute_constraint_matrices (scp.py:182-257) -------------------------------
 * l_out/u_out have N*D*(4K-1) entries in the reference's stacking order jerk, acc, vel, pos (scp.py:342-358).
 * limits = {vel_min, vel_max, acc_min, acc_max, jerk_min, jerk_max} [host]; space = {min_0..min_{D-1},
 * max_0..max_{D-1}} [host]. */
int scp_fixed_bounds(scp_ctx* ctx, int N, int K, int D, double h, const double* limits, const double* space,
                     const double* p0, const double* v0, const double* pf, const double* vf, double* l_out,
                     double* u_out);

/* ---- a5 (+a8 fused): SCP._add_collision_constraints (scp.py:453-557) ---------------------------------
 * Linearises the pairs q in [q_begin, q_end) at every k around pos_prev and writes the COMPACT form of
 * A_collision / l_collision: eta_out[d*scp_eta_stride(K,nq) + k*nq + (q-q_begin)] (SoA planes, nq = q_end-q_begin,
 * D*scp_eta_stride doubles, 16-byte aligned) and l_out[k*nq + (q-q_begin)].
 * Row r of the reference's matrix is  +eta_r[d] h^2 (k-m-.5) on a_i[m], -(same) on a_j[m], m < k; u = +inf.
 * Degenerate pairs (dist < 1e-6): eta = e_0, dist := 1 (the reference draws a random direction, scp.py:505).
 * Fused reductions: stats->min_dist, stats->first_violation (dist < R-0.01), and the rows with
 * dist - R < margin are appended (global row ids r = k*pairs + q) to sel_rows (capacity sel_cap) and marked
 * in sel_bitmap (one bit per LOCAL row k*nq + (q-q_begin), ceil(K*nq/32) uint32 words, zeroed by this call). */
int scp_linearize_pairs(scp_ctx* ctx, int N, int K, int D, double R, double h, int64_t q_begin, int64_t q_end,
                        const double* pos_prev, const double* p0, const double* v0, double* eta_out,
                        double* l_out, double margin, int64_t* sel_rows, int64_t sel_cap, uint32_t* sel_bitmap,
                        scp_pair_stats* stats);

/* The same pass WITHOUT the row stream ("row-free" linearisation): identical distances, selection test (dist - R < margin),
 * sel_rows / sel_bitmap / stats as scp_linearize_pairs, but eta / l are not written (24 B per row: 630 MB at 1024 x 50,
 * 10 GB at 4096 x 50, of which the loop consumes the ~0.05 % selected rows).  The consumer recomputes the selected rows
 * with scp_qp_add_rows_at; scp_collision_violations_at never needed the stored rows. */
int scp_select_pairs(scp_ctx* ctx, int N, int K, int D, double R, int64_t q_begin, int64_t q_end, const double* pos_prev,
                     double margin, int64_t* sel_rows, int64_t sel_cap, uint32_t* sel_bitmap, scp_pair_stats* stats);

/* ---- a8: SCP._fast_check_avoidance_constraints (scp.py:597-615) --------------------------------------
 * stats->first_violation = first row (k -> i -> j order) with ||p_i - p_j|| < R - 0.01, stats->min_dist. */
int scp_check_avoidance(scp_ctx* ctx, int N, int K, int D, double R, int64_t q_begin, int64_t q_end,
                        const double* pos, scp_pair_stats* stats);

/* ---- continuous-time separation: what a8 cannot see between two samples -------------------------------
 * Over segment k (k = 0..K-1; the last one ends in the final state) vehicle i flies p_i[k] + t v_i[k] + t^2/2 a_i[k],
 * t in [0, h] (the kinematics of scp_kinematics), so the squared distance of a pair is a quartic in t.  One pass over the
 * K * (q_end - q_begin) segments; pos, vel, acc are [N][K][D] as scp_kinematics leaves them.  A segment's distance is
 * sqrt(max(min over [0, h] of the quartic, 0)).  Rows are numbered as everywhere: k*pairs + q.  The result is deterministic and
 * does not depend on how a pair range is cut: over shards, the smallest (min_dist, argmin_row), the smallest
 * first_violation and the sum of n_violating are bit for bit those of the full range.  `stats` is DEVICE memory (48 bytes);
 * an empty pair range leaves min_dist = sample_min_dist = +inf and no violation.  Argument checks, error codes and stream
 * behaviour as scp_check_avoidance; scp_ctx_last_pair_ms then reports this call's kernels (staging, pass, final reduction). */
typedef struct scp_separation_stats {
  double min_dist;           /* smallest segment distance */
  double sample_min_dist;    /* smallest distance at the samples (t = 0) of the same rows: scp_check_avoidance's min_dist, bitwise */
  double argmin_t;           /* min_dist is attained argmin_t seconds into the segment ... */
  uint64_t argmin_row;       /* ... of this row; bitwise equal minima: the smallest row id.  UINT64_MAX: empty pair range */
  uint64_t first_violation;  /* smallest row id whose segment distance is < R - 0.01 (the a8 threshold), UINT64_MAX if none */
  uint64_t n_violating;      /* number of such segments */
} scp_separation_stats;
int scp_check_separation(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                         const double* pos, const double* vel, const double* acc, scp_separation_stats* stats);
/* Segments of the latest scp_check_separation of this ctx whose quartic was minimised (the others were excluded by one
 * comparison: too far apart to be a violation or the minimum); a cost figure, results never depend on it.  Synchronises. */
int scp_ctx_last_separation_solved(scp_ctx* ctx, uint64_t* n_solved /* [host] */);

/* ---- the conflict list: WHICH segments scp_check_separation counts in n_violating, when, and how close -----------------
 * A purely additive part of ABI version 7: one struct and one function, nothing else changes.
 * One record per violating segment of the pair range -- a segment whose distance sqrt(max(min f, 0)) is < R - 0.01, the test
 * of n_violating on the same bits (f: the quartic above; the arithmetic per segment is scp_check_separation's, so min_dist and
 * t_min are bit for bit what that call reports for the row).  out[0 .. *n_found) is in ascending row order; the result is
 * deterministic and does not depend on how a pair range is cut: the lists of disjoint shards, merged by row, are bit for
 * bit the list of the full range.  `out` (capacity records) and `n_found` are DEVICE memory.  If *n_found > capacity
 * NOTHING in `out` is defined and the call still returns SCP_OK: repeat it with a longer list (the protocol of
 * scp_collision_violations).  An empty pair range gives *n_found = 0.  Argument checks, error codes, stream and timing
 * behaviour as scp_check_separation (scp_ctx_last_pair_ms: staging, pass, sort); capacity in [0, 2^30]. */
typedef struct scp_conflict {
  uint64_t row;       /* k*pairs + q, as everywhere */
  double min_dist;    /* the segment's distance: sqrt(max(min f, 0)) */
  double t_min;       /* where in [0, h] it is attained */
  double t_enter;     /* smallest t in [0, h] with f(t) < (R - 0.01)^2 (to the 2^-48 h of a bisection); exactly 0 if the
                         segment starts inside */
  double t_exit;      /* largest such t; exactly h if it ends inside */
  uint32_t pieces;    /* 1 or 2: maximal sub-intervals of [t_enter, t_exit] below the threshold (2: the vehicles come within
                         the threshold, part, and come within it again inside one segment; [t_enter, t_exit] is the hull) */
  uint32_t reserved;  /* 0 */
} scp_conflict;
int scp_list_conflicts(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                       const double* pos, const double* vel, const double* acc, scp_conflict* out, int64_t capacity,
                       uint64_t* n_found);

/* ---- clearance profiles: the closest approach of every vehicle and of every time step -------------------------------------
 * A purely additive part of ABI version 7: one struct and two functions, nothing else changes.
 * The K * (q_end - q_begin) segment minima of scp_check_separation, reduced along the other two axes:
 *   per_vehicle[i] covers every row (k, q) of the pair range whose pair contains vehicle i (its margin, against whom, when);
 *   per_step[k]    covers the rows k*pairs + q, q in [q_begin, q_end) (the fleet's minimum distance over the horizon).
 * The arithmetic per segment is scp_check_separation's on the same bits: the lexicographic minimum of (min_dist, row) over the
 * vehicles, and over the steps, is that call's (min_dist, argmin_row) with its argmin_t; the n_violating of the steps sum to
 * its n_violating, those of the vehicles to twice that; the smallest sample_min_dist is its sample_min_dist; an entry with
 * n_violating > 0 carries the (min_dist, row, t_min) of the smallest scp_list_conflicts record that involves it.
 * An entry that covers no row (an empty range, N = 1, a vehicle without a pair in the shard) is
 * {+inf, 0, UINT64_MAX, +inf, 0, 0}.  Both arrays are DEVICE memory; one of them may be NULL (that profile is not written),
 * both NULL is SCP_ERR_INVALID.  The result is deterministic and does not depend on how a pair range is cut: over disjoint
 * shards the entry-wise lexicographic minimum of (min_dist, row) with that shard's t_min, the entry-wise minimum of
 * sample_min_dist and the entry-wise sum of n_violating are bit for bit those of the full range.  Unlike the check, a segment
 * is excluded without minimising its quartic only if its distance provably exceeds max(R - 0.01, the smallest sampled
 * distance of vehicle i, of vehicle j, of step k): more segments reach the quartic (scp_ctx_last_clearance_solved).
 * Argument checks, error codes, stream and timing behaviour as scp_check_separation (scp_ctx_last_pair_ms: all kernels of
 * the call). */
typedef struct scp_clearance {
  double min_dist;          /* smallest segment distance sqrt(max(min f, 0)) over the rows this entry covers; +inf: none */
  double t_min;             /* where in [0, h] of that row's segment it is attained */
  uint64_t row;             /* k*pairs + q of that segment; bitwise equal minima: the smallest row; UINT64_MAX: none */
  double sample_min_dist;   /* smallest distance at the samples (t = 0) of the same rows, as scp_check_avoidance computes it */
  uint64_t n_violating;     /* segments among them whose distance is < R - 0.01 (the test of scp_check_separation) */
  uint64_t reserved;        /* 0 */
} scp_clearance;
int scp_clearance_profile(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                          const double* pos, const double* vel, const double* acc,
                          scp_clearance* per_vehicle /* [N] or NULL */, scp_clearance* per_step /* [K] or NULL */);
/* Segments of the latest scp_clearance_profile of this ctx whose quartic was minimised; a cost figure.  Synchronises. */
int scp_ctx_last_clearance_solved(scp_ctx* ctx, uint64_t* n_solved /* [host] */);

/* ---- delay margins: the clearance of every vehicle against a late start ------------------------------------------------------
 * A purely additive part of ABI version 7: one struct and two functions, nothing else changes.
 * pos, vel, acc are [N][K][D] as scp_check_separation takes them.  Every vehicle i has K + 2 RECORDS (position, velocity,
 * acceleration), r = -1 .. K:
 *   r = -1        held at the start:    (p_i[0], 0, 0);
 *   r = 0 .. K-1  the stored segment:   (p_i[r], v_i[r], a_i[r]);
 *   r = K         parked at the goal:   (pK_i, 0, 0),  pK = p[K-1] + (h*v[K-1] + (0.5*h*h)*a[K-1]), every product and every sum
 *                 rounded on its own (no contraction), so that numpy reproduces the bits of pK.
 * DELAY s of vehicle a, s = 0 .. max_lag: a alone starts s steps late -- it is held at its start for s steps, then flies its
 * stored plan; everybody else flies on schedule and parks at the goal afterwards.  The comparison covers the global segments
 * g = 0 .. K+s-1; in segment g vehicle a uses record g - s (-1 while g < s) and a vehicle b != a record min(g, K).  The segment
 * distance is that of the other continuous-time passes, sqrt(max(min_{t in [0, h]} f(t), 0)), f the quartic of the two records'
 * differences (the arithmetic per segment is scp_check_separation's).
 * ENTRY (a, s), out[(a - a_begin) * (max_lag + 1) + s], reduces over all b != a and all g: min_dist, t_min, segment (the
 * global g) and partner (b) are those of the lexicographic minimum of (min f, g, b) -- bitwise equal minima go to the
 * smallest (g, b) --; n_violating counts the (b, g) whose segment distance is < R - 0.01 (the test of scp_check_separation).
 * An entry without a pair (N = 1) is {+inf, 0, UINT32_MAX, UINT32_MAX, 0}.  Two consequences:
 *   lag 0 is the clearance profile: entry (a, 0) has the min_dist, t_min and n_violating of scp_clearance_profile's
 *     per_vehicle[a] over the full pair range, bit for bit, and (segment, partner) is that entry's row decoded (the order
 *     (g, b) is the row order k*pairs + q restricted to vehicle a; the quartic's coefficients are products of two
 *     differences, so they carry the same bits whichever vehicle is subtracted from which);
 *   a delay is a shifted fleet: on arrays of horizon K + s in which vehicle a has s held records followed by its plan and
 *     everybody else the plan followed by s parked records, scp_clearance_profile's per_vehicle[a] is entry (a, s) bit for bit.
 * Ranges: 0 <= a_begin <= a_end <= N (an empty range writes nothing and returns SCP_OK), 0 <= max_lag <= K.  The result is
 * deterministic (no floating-point atomics) and does not depend on how the vehicle range is cut: the entries of disjoint
 * ranges, concatenated, are the bytes of the full call -- the vehicle range is the multi-rank cut, nothing has to be merged.
 * A segment is excluded without minimising its quartic only if its distance provably exceeds max(R - 0.01, the smallest
 * distance entry (a, s) has so far); results never depend on what was excluded (scp_ctx_last_delay_solved).  `out` is DEVICE
 * memory.  Argument checks, error codes, stream and timing behaviour as scp_clearance_profile (scp_ctx_last_pair_ms: all
 * kernels of the call).  scp_ctx_set_option "delay_lag_chunk" / "delay_time_chunk" (default 0: chosen by the call) fix the
 * lags / global segments a workgroup covers; developer switches, results never depend on them. */
typedef struct scp_delay_margin {   /* 32 bytes */
  double   min_dist;    /* smallest segment distance of vehicle a, started s steps late, to anybody; +inf: no pair */
  double   t_min;       /* where in [0, h] of that segment */
  uint32_t partner;     /* against whom; UINT32_MAX: none */
  uint32_t segment;     /* global segment g in [0, K + s); UINT32_MAX: none */
  uint64_t n_violating; /* (partner, segment) combinations below R - 0.01 */
} scp_delay_margin;
int scp_delay_margins(scp_ctx* ctx, int N, int K, int D, double h, double R, int a_begin, int a_end, int max_lag,
                      const double* pos, const double* vel, const double* acc,
                      scp_delay_margin* out /* DEVICE, [a_end - a_begin][max_lag + 1] */);
/* Segments of the latest scp_delay_margins of this ctx whose quartic was minimised; a cost figure.  Synchronises. */
int scp_ctx_last_delay_solved(scp_ctx* ctx, uint64_t* n_solved /* [host] */);

/* ---- staggered starts: pair-lag conflict masks and a greedy launch schedule ------------------------------------------------
 * A purely additive part of ABI version 7: one struct and four functions, nothing else changes.
 * The cheapest remedy for between-sample conflicts: every plan stays as it is and some vehicles start a few steps later.
 * Records, lags, global segments, the segment distance sqrt(max(min f, 0)) and the threshold R - 0.01 are those of
 * scp_delay_margins above; that call reduces over b, so it covers one late vehicle among punctual ones.  Here the same segment
 * test is kept per ORDERED pair and per lag:
 *   MASKS.  For a != b and s = 0 .. max_lag, bit s of mask[a][b] is set iff at least one global segment g in [0, K + s)
 *     violates the threshold, the segment comparing record max(g - s, -1) of a with record min(g, K) of b -- exactly the (b, g)
 *     entry (a, s) of scp_delay_margins counts in n_violating, decided on the same bits.  mask[a][a] = 0, bits above max_lag are
 *     0, and bit 0 is symmetric (the quartic's coefficients carry the same bits whichever vehicle is subtracted from which).
 *   ONLY THE RELATIVE LAG MATTERS.  If a starts d_a steps late and b d_b, d_a >= d_b, the segments before d_b compare two held
 *     records (a constant: f(0) of the first segment that lag d_a - d_b examines), those after K + d_a two parked records (the
 *     goal distance: the END of the last segment that lag examines, equal to it up to rounding), and in between lies the
 *     situation of lag d_a - d_b of (a, b).  So the pair conflicts iff bit d_a - d_b of mask[a][b] is set (d_a < d_b: bit
 *     d_b - d_a of mask[b][a]) -- unless a start or goal distance lies within rounding of the threshold.
 *   SCHEDULE.  Vehicles are taken in the order order[0], order[1], ... (a permutation of 0 .. N-1; NULL: the identity).
 *     Vehicle v gets the smallest d in [0, max_lag] that conflicts with no vehicle u PLACED before it: for d >= d_u bit d - d_u
 *     of mask[v][u] must be clear, for d < d_u bit d_u - d of mask[u][v].  Without such a d, delay[v] = -1: v is unplaced and
 *     takes no part in the later comparisons.  Integers only, deterministic; a fleet without lag-0 conflicts gets all zeros.
 *   THE STAGGERED FLEET has the horizon K + Dmax, Dmax the largest delay; vehicle v uses record clamp(g - d_v, -1, K) in
 *     segment g (unplaced vehicles: d = 0).  It is an ordinary input of scp_check_separation and scp_list_conflicts, which
 *     judge the result.
 * scp_lag_conflicts: arguments, argument checks, error codes, stream and timing behaviour as scp_delay_margins, plus
 * max_lag <= 63 (so 0 <= max_lag <= min(K, 63)).  `mask` is DEVICE memory, row a - a_begin of N words per vehicle of the range;
 * an empty range writes nothing; the rows of disjoint ranges, concatenated, are the bytes of the full call (the vehicle range
 * is the multi-rank cut).  A segment is excluded without minimising its quartic only if its distance provably exceeds
 * R - 0.01, and an (a, b, s) whose bit is set may skip its remaining segments; the mask never depends on either
 * (scp_ctx_last_lag_solved).  Results are combined by integer ORs only and do not depend on how lags and segments are cut over
 * workgroups: scp_ctx_set_option "lagc_lag_chunk" / "lagc_time_chunk" (default 0: chosen by the call) are developer switches.
 * scp_schedule_starts: all pointers DEVICE; supported 1 <= N <= 16384, 0 <= max_lag <= 63; only bits 0 .. max_lag of a word
 * are looked at.  One workgroup; the call synchronises (scp_ctx_last_pair_ms then reports its kernel).  An `order` that is no
 * permutation returns SCP_ERR_INVALID after the launch; delay and stats are then undefined. */
typedef struct scp_start_schedule_stats {   /* DEVICE, 48 bytes */
  int32_t n_delayed;       /* vehicles with delay > 0 */
  int32_t n_unplaced;      /* vehicles with delay = -1 */
  int32_t max_delay;       /* the largest delay (0 if nobody is placed) */
  int32_t first_unplaced;  /* the first vehicle, in schedule order, that found no delay; -1: none */
  int64_t total_delay;     /* sum of the delays of the placed vehicles */
  int64_t reserved[3];     /* 0 */
} scp_start_schedule_stats;
int scp_lag_conflicts(scp_ctx* ctx, int N, int K, int D, double h, double R, int a_begin, int a_end, int max_lag,
                      const double* pos, const double* vel, const double* acc,
                      uint64_t* mask /* DEVICE, [a_end - a_begin][N] */);
/* Segments of the latest scp_lag_conflicts of this ctx whose quartic was minimised; a cost figure.  Synchronises. */
int scp_ctx_last_lag_solved(scp_ctx* ctx, uint64_t* n_solved /* [host] */);
int scp_schedule_starts(scp_ctx* ctx, int N, int max_lag, const uint64_t* mask /* [N][N] */,
                        const int32_t* order /* [N] or NULL */, int32_t* delay /* [N] */, scp_start_schedule_stats* stats);
/* scp_schedule_starts_batch (one more function of ABI version 7, nothing else changes): the order is the only free parameter
 * of the SCHEDULE rule, so B candidate orders are scheduled on the same masks in ONE launch and the best is named.
 *   RULE.  For every candidate b = 0 .. B-1, delay[b][.] and stats[b] are the bytes scp_schedule_starts(ctx, N, max_lag, mask,
 *     orders + b N, ...) writes: every field, first_unplaced and the zeroed `reserved` included.  Integers only.
 *   OBJECTIVE.  *best is the candidate with the smallest key, compared lexicographically:
 *     objective 0 ("makespan"): (n_unplaced, max_delay, total_delay, b);   objective 1 ("total"): (n_unplaced, total_delay,
 *     max_delay, b).  The trailing b sends ties to the lowest index.  (n_unplaced <= 2^14, max_delay <= 63,
 *     total_delay < 2^20 and b < 2^16 pack into one 64-bit word whose integer minimum is the lexicographic one.)
 * mask, orders, delay and stats are DEVICE memory, `best` is host memory; `orders` must not be NULL.  Supported: 1 <= N <= 16384,
 * 0 <= max_lag <= 63, 1 <= B <= 65535, objective 0 or 1, non-null pointers; anything else returns SCP_ERR_INVALID with a
 * message.  One workgroup per candidate, no workgroup waits for another, the masks are only read (from 16 candidates on the
 * call first writes their transpose into N^2 words of the context's workspace, so that both reads of a step are rows).  Enqueued on the ctx
 * stream; the call synchronises, and scp_ctx_last_pair_ms then reports its device time.  If a candidate is no permutation the
 * call returns SCP_ERR_INVALID after the launch, the message names the lowest such candidate, delay / stats / *best are
 * undefined and the context stays usable.  Results do not depend on the threads a workgroup runs with
 * (scp_ctx_set_option "stg_batch_threads"). */
int scp_schedule_starts_batch(scp_ctx* ctx, int N, int max_lag, const uint64_t* mask /* [N][N] DEVICE */,
                              int B, const int32_t* orders /* [B][N] DEVICE, not NULL */, int objective,
                              int32_t* delay /* [B][N] DEVICE */, scp_start_schedule_stats* stats /* [B] DEVICE */,
                              int32_t* best /* [host] */);

/* ---- holds: repair between-sample conflicts with a separating half-plane per segment ------------------------------------------
 * A purely additive part of ABI version 7: one struct and two functions, nothing else changes.
 * A HOLD (row r = (k', q), unit vector e, margin c >= 0) replaces collision row r of the linearisation by the FIXED half-plane
 *   e . (p_i[k'] - p_j[k']) >= R + c,   in the row form of scp_linearize_pairs:  eta_r = e,
 *   l_r = (R + c) - e . ((p0_i - p0_j) + (k' h)(v0_i - v0_j)),
 * which does not depend on the linearisation point.  If the rows k and k + 1 of a pair carry the same e with margin c,
 * e . d(t) (d: the relative motion in segment k, a quadratic in t) is >= R + c at both ends of the segment, hence
 * >= R + c - |e . (a_i - a_j)[k]| h^2 / 8 inside it, and |d(t)| >= e . d(t).
 *
 * scp_update_holds: one repair pass's table update.  Every record of scp_list_conflicts (row (k, q), min_dist, t_min) whose pair
 * lies in [q_begin, q_end) yields, with the differences of pos / vel / acc[.][k] taken i minus j, every product and every sum
 * rounded on its own (no contraction) and coordinates in ascending order:
 *   t = t_min;  dm = dp + (t dv + ((0.5 t) t) da);  n = sqrt(sum_d dm_d^2);
 *   n >= 1e-6: e = dm / n;  otherwise w = dv + t da and  2-D: e = (-w_1, w_0) / |w|;  3-D: e = (w x e_m) / |w x e_m| with m the
 *   coordinate of the smallest |w_m| (the lowest on ties);  |w| < 1e-12: e = e_0;
 *   the shortfall s = (R - min_dist) + pad.
 * The record proposes (e, s) for row (k, q) and, if k + 1 < K, for row (k + 1, q).  Several proposals for one row: the largest
 * s wins, ties go to the proposal of the smaller conflict row.  Then the merge into the table (sorted by row, unique rows): a
 * row already held takes the new e and its margin becomes old + s; a new row enters with margin s.
 * `conflicts` is a list as scp_list_conflicts leaves it (ascending rows), `table` has room for `capacity` records, *n_holds
 * (in / out) of them are in use; all are DEVICE memory.  Capacity as scp_list_conflicts: if the result needs more than
 * `capacity` records the table is left as it was, *n_holds receives the size needed and the call returns SCP_OK.
 * Deterministic, no floating-point atomics.  The largest table (and the longest conflict list) is SCP_HOLD_MAX_TABLE records;
 * beyond it the call returns SCP_ERR_CAPACITY.  Argument checks, stream and timing as scp_list_conflicts; the host reads the two
 * counts first (drains the stream).
 *
 * scp_apply_holds: for every hold whose pair lies in [q_begin, q_end), e goes to the SoA planes `eta` and l_r (the formula
 * above, no contraction) to `l` at the local row, as scp_linearize_pairs lays them out, and the row's bit is set in
 * sel_bitmap; new_rows receives, in ascending order, the global ids of the holds whose bit was clear, *n_new (DEVICE) their
 * number.  If *n_new > new_cap NOTHING is written at all (planes, bitmap, list): repeat the call with a longer list.  Every
 * other entry of the planes and of the bitmap keeps its bits. */
#define SCP_HOLD_MAX_TABLE (1 << 20)
typedef struct scp_hold {   /* 48 bytes */
  uint64_t row;       /* k' * pairs + q */
  double eta[3];      /* the unit vector e; eta[2] = 0 in 2-D */
  double margin;      /* c >= 0 */
  uint64_t reserved;  /* 0 */
} scp_hold;
int scp_update_holds(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                     const double* pos, const double* vel, const double* acc, const scp_conflict* conflicts,
                     const uint64_t* n_conflicts /* DEVICE */, double pad, scp_hold* table, int64_t capacity,
                     uint64_t* n_holds /* DEVICE, in / out */);
int scp_apply_holds(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                    const scp_hold* table, const uint64_t* n_holds /* DEVICE */, const double* p0, const double* v0,
                    double* eta, double* l, uint32_t* sel_bitmap, int64_t* new_rows, int64_t new_cap,
                    uint64_t* n_new /* DEVICE */);

/* ---- constraint generation for the joint QP (a6): full pass over the linearised rows ------------------
 * For every local row not yet marked in sel_bitmap: if (A_col x)_r < l_r - feas_tol, mark it and append its
 * global id to new_rows.  (A_col x)_r = eta_r . ((pos_i - c_i) - (pos_j - c_j))[k], c = p0 + k h v0,
 * pos = kinematics(x).  stats->n_selected = rows found, stats->max_violation.  If n_selected exceeds new_cap NOTHING is
 * merged into sel_bitmap and new_rows is left untouched: repeat the call with a longer list. */
int scp_collision_violations(scp_ctx* ctx, int N, int K, int D, double h, int64_t q_begin, int64_t q_end,
                             const double* eta, const double* l_col, const double* pos, const double* p0,
                             const double* v0, double feas_tol, int64_t* new_rows, int64_t new_cap,
                             uint32_t* sel_bitmap, scp_pair_stats* stats);

/* The same pass without reading the stored rows back: eta_r and R - dist_r are recomputed from the linearisation
 * point pos_prev (the arithmetic of scp_linearize_pairs) and
 *   l_r - (A_col x)_r = (R - dist_r) - eta_r . ((pos_new - pos_prev)_i - (pos_new - pos_prev)_j)[k]
 * (the free motion c cancels), so the pass streams nothing from HBM (the stored rows cost 8 (D + 1) bytes per row to
 * read: 630 MB at 1024 x 50).  Differs from scp_collision_violations by rounding only (one fused sum instead of two). */
int scp_collision_violations_at(scp_ctx* ctx, int N, int K, int D, double R, int64_t q_begin, int64_t q_end,
                                const double* pos_prev, const double* pos_new, double feas_tol, int64_t* new_rows,
                                int64_t new_cap, uint32_t* sel_bitmap, scp_pair_stats* stats);

/* Gather the compact rows `rows` (global ids, all inside [q_begin,q_end) x K) out of (eta, l_col):
 * w_eta[n][D] (AoS) and w_l[n]. */
int scp_gather_rows(scp_ctx* ctx, int N, int K, int D, int64_t q_begin, int64_t q_end, const double* eta,
                    const double* l_col, const int64_t* rows, int64_t n, double* w_eta, double* w_l);

/* ---- a1: relative step of the SCP loop (scp.py:157-159) ----------------------------------------------
 * out[0] = ||a_new - a_prev||_2, out[1] = ||a_prev||_2, out[2] = out[0]/out[1] (no zero guard, as the
 * reference).  out is [host]. */
int scp_rel_step(scp_ctx* ctx, int64_t n, const double* a_new, const double* a_prev, double* out);

/* ---- a3 / a6 / a9: the joint QP  min ||x||^2  s.t. fixed rows, collision rows -------------------------
 * Replaces osqp.OSQP().setup/warm_start/solve at scp.py:326-367 and :441-449.  ADMM in OSQP's form with a
 * matrix-free x-update (PCG preconditioned by the exact inverse of the block-diagonal fixed part), on the
 * fixed rows plus a working set of collision rows supplied by the caller (exact constraint generation is
 * driven through scp_collision_violations). */
void scp_qp_default_settings(scp_qp_settings* s);
size_t scp_qp_workspace_bytes(int N, int K, int D, int64_t row_capacity);
int scp_qp_create(scp_ctx* ctx, int N, int K, int D, double h, const scp_qp_settings* s, void* workspace,
                  size_t workspace_bytes, int64_t row_capacity, scp_qp** out);
void scp_qp_destroy(scp_qp* qp);
int scp_qp_update_settings(scp_qp* qp, const scp_qp_settings* s);
/* bounds of the fixed rows from the problem data (same arithmetic as scp_fixed_bounds) */
int scp_qp_set_problem(scp_qp* qp, const double* limits /*[host]*/, const double* space /*[host]*/,
                       const double* p0, const double* v0, const double* pf, const double* vf);
/* start a new QP: x = x0 ([N][K][D], NULL -> 0), z = A x, y = 0 (primal warm start only, scp.py:443),
 * empty working set, rho = settings.rho */
int scp_qp_reset(scp_qp* qp, const double* x0);
/* Start (or continue) from another step size than settings.rho -- e.g. the value the previous SCP iteration's QP ended with
 * (scp_solve_options.carry_rho): the rho-dependent blocks are taken from the cache or rebuilt.  After scp_qp_reset. */
int scp_qp_set_rho(scp_qp* qp, double rho);
/* append working rows (global ids; eta AoS [n][D]; lower bounds); z = max(A x, l), y = 0 */
int scp_qp_add_rows(scp_qp* qp, int64_t n, const int64_t* rows, const double* w_eta, const double* w_l);
/* append working rows with eta / l recomputed from the linearisation point pos_prev ([N][K][D]) by the arithmetic of
 * scp_linearize_pairs (bit-identical to gathering its stored rows); p0, v0 [N][D]; R = min_distance */
int scp_qp_add_rows_at(scp_qp* qp, int64_t n, const int64_t* rows, const double* pos_prev, const double* p0,
                       const double* v0, double R);
int scp_qp_solve(scp_qp* qp, scp_qp_info* info /*[host]*/);
/* Move a QP to a larger workspace: dst (same N, K, D, h; row_capacity >= src's working rows) takes over the
 * problem bounds, iterate, duals, working set and rho of src, so a solve can continue after its working set outgrew
 * the capacity it was created with.  Where src's last check left S0 x and F x exact they travel too: the solve in dst
 * continues with the bits it would have had in src. */
int scp_qp_clone_state(scp_qp* dst, const scp_qp* src);
int scp_qp_get_solution(scp_qp* qp, double* x_out /*[N][K][D]*/);
/* duals: y_fixed in the reference stacking order (N*D*(4K-1)), y_col per working row (may be NULL) */
int scp_qp_get_duals(scp_qp* qp, double* y_fixed, double* y_col);

/* ---- a1 as ONE call: SCP.generate_trajectories (scp.py:131-180) driven natively ------------------------------
 * The SCP loop is control flow around the entry points above; path_planning/solvers/scp.py drives them from Python
 * (about a hundred calls and half a dozen blocking reads per SCP iteration).  scp_solver_solve makes the SAME calls in
 * the SAME order from C++: QP#0, the avoidance check evaluated once (scp.py:144), then per iteration kinematics,
 * scp_linearize_pairs, the joint QP with exact constraint generation (scp_qp_* + scp_collision_violations_at) and the
 * relative-step test, optionally the polish QP, and the final kinematics.  Bit-identical to the Python-driven loop.
 * The solver object owns its device memory (hipMalloc: compact rows, bitmap, row lists, QP workspace, trajectories). */
typedef struct scp_solver scp_solver;

typedef struct scp_solve_options {
  int32_t max_iterations;       /* 15: SCP iterations (compute_trajectories.py:75) */
  int32_t max_rounds;           /* 20: constraint-generation rounds per joint QP */
  int32_t max_iter0;            /* 4000: ADMM iterations of QP#0 (OSQP default, scp.py:360) */
  int32_t max_iter;             /* 10000: ADMM iterations per joint QP (scp.py:442) */
  int32_t refresh_feasibility;  /* 0: re-evaluate is_feasible inside the loop (the reference's TODO, scp.py:150) */
  int32_t polish;               /* 0: one more joint QP at polish_eps after the loop */
  double working_set_margin;    /* 0.5 m */
  double feasibility_tol;       /* 1e-6 */
  double polish_eps;            /* 1e-8 */
  double convergence_tolerance; /* 1.5e-2 (scp.py:52) */
  int32_t row_free;             /* 1: linearise with scp_select_pairs + scp_qp_add_rows_at (no eta / l planes are written
                                   or allocated); 0: scp_linearize_pairs writes all rows and the working rows are gathered
                                   from them.  Same working rows, same bits either way */
  int32_t carry_rho;            /* 0 (OSQP: every new solver object starts at settings.rho, scp.py:441); 1: the joint QP of SCP
                                   iteration n + 1 starts at the rho iteration n ended with (its blocks are cached), which saves
                                   the adaptive-rho transient: fewer ADMM steps, the same minimiser within eps */
} scp_solve_options;

#define SCP_MAX_ROUNDS_RECORDED 24
/* [host] one per QP of a solve: records[0] = QP#0, then one per SCP iteration, then the polish QP if requested */
typedef struct scp_qp_record {
  int32_t status_val;       /* of the last constraint-generation round */
  int32_t iter;             /* ADMM iterations, all rounds */
  int32_t rho_updates, cg_iters_total, rounds;
  int32_t pipeline;         /* OR over the rounds of scp_qp_info.pipeline */
  int64_t working_rows, unresolved_rows;
  int64_t added[SCP_MAX_ROUNDS_RECORDED]; /* rows found by the violations pass after each round */
  double r_prim, r_dual, rho, solve_ms, max_violation;
  double rel_step;          /* ||a_new - a_prev|| / ||a_prev|| (scp.py:157-159); -1 for QP#0 / polish */
  double time_sec;          /* wall time of the SCP iteration */
  double linearize_ms;      /* device time of the linearisation kernel alone (HIP events around that launch) */
  double violations_ms;     /* device time of the last violations kernel */
  int32_t persist_launches, persist_gave_up, rho_switches_in_kernel, reserved;  /* sums over the rounds (scp_qp_info) */
} scp_qp_record;

typedef struct scp_solve_result {
  int32_t n_iterations, converged, initially_feasible, feasible_at_exit, polished;
  int32_t qp0_status;       /* not in {1, 2}: the caller raises RuntimeError("OSQP failed: ...") like scp.py:363-365 */
  int32_t n_records;
  int32_t first_violation_k, first_violation_i, first_violation_j;  /* of the initial check (scp.py:611-613) */
  uint64_t first_violation; /* row id, UINT64_MAX if none */
  double first_violation_distance;
  double time_sec;
} scp_solve_result;

void scp_solve_default_options(scp_solve_options* o);
/* qp_row_capacity <= 0: the default min(K pairs, max(8192, 32 N K)) (grows on demand) */
int scp_solver_create(scp_ctx* ctx, int N, int K, int D, double h, double R, const scp_qp_settings* st,
                      int64_t qp_row_capacity, scp_solver** out);
void scp_solver_destroy(scp_solver* s);
int scp_solver_update_settings(scp_solver* s, const scp_qp_settings* st);
/* limits / space [host] as in scp_fixed_bounds; p0, v0, pf, vf [N][D] device; acc_out, pos_out, vel_out [N][K][D] device;
 * res, records [host], record_capacity >= max_iterations + 2.  Synchronises the stream before returning. */
int scp_solver_solve(scp_solver* s, const double* limits, const double* space, const double* p0, const double* v0,
                     const double* pf, const double* vf, const scp_solve_options* o, double* acc_out, double* pos_out,
                     double* vel_out, scp_solve_result* res, scp_qp_record* records, int record_capacity);

/* ONE SCP iteration (the loop body scp.py:152-166 without the convergence decision): linearise around acc_in, joint QP with
 * exact constraint generation, relative step -> *rec [host] (rel_step, time_sec, linearize_ms ... filled), acc_out = the new
 * accelerations ([N][K][D] device, may alias nothing).  Same calls in the same order as one pass of scp_solver_solve's loop;
 * bench.py times this call.  The host waits for the relative step; acc_out is written by that kernel and is ordered on the
 * ctx stream like any kernel's output (small problems, whose last pass computes the relative step, copy and drain). */
int scp_solver_step(scp_solver* s, const double* limits, const double* space, const double* p0, const double* v0,
                    const double* pf, const double* vf, const scp_solve_options* o, const double* acc_in, double* acc_out,
                    scp_qp_record* rec);

/* ---- the same iteration split at its exchange points: agents / pairs sharded over the GPUs of a node, one process per GPU ---
 * Every rank holds the whole (N, K, D) problem and calls, per SCP iteration,
 *   scp_solver_shard_begin       bounds, positions of the linearisation point (pos_in = the allgathered per-shard trajectories,
 *                                or NULL: computed from acc_in), row-free selection over ITS pair range -> its row ids
 *   [exchange: allgather of the ids, sorted ascending -- the only data that crosses ranks]
 *   scp_solver_shard_qp          the gathered rows join the REPLICATED working set (eta / l recomputed locally: every rank
 *                                has the linearisation point), ADMM on the joint QP: deterministic, the same bits on every rank
 *   scp_solver_shard_violations  every row of its pair range checked at the solution -> its new row ids, max violation
 *   [exchange: allgather of the ids, max of the violations]
 *   scp_solver_shard_round_done  *more = another round (-> shard_qp with the new rows) or not
 *   scp_solver_shard_end         relative step, acc_out, the record
 * which are the phases scp_solver_step runs back to back over the full pair range: a world of one rank that skips the
 * exchanges reproduces scp_solver_step bit for bit, and so does any world size (sorted ids = the single-rank row order).
 * rows_out (device, capacity rows_cap) receives this rank's ids, *n_local [host] their number; if n_local > rows_cap only the
 * first rows_cap were copied: fetch them again with scp_solver_shard_rows into a longer list.  rec [host] accumulates. */
int scp_solver_shard_begin(scp_solver* s, const double* limits, const double* space, const double* p0, const double* v0,
                           const double* pf, const double* vf, const scp_solve_options* o, const double* acc_in,
                           const double* pos_in, int64_t q_begin, int64_t q_end, scp_qp_record* rec,
                           int64_t* rows_out, int64_t rows_cap, int64_t* n_local);
int scp_solver_shard_rows(scp_solver* s, int64_t* rows_out, int64_t rows_cap);
int scp_solver_shard_qp(scp_solver* s, const int64_t* rows, int64_t n, scp_qp_record* rec);
int scp_solver_shard_violations(scp_solver* s, int64_t* rows_out, int64_t rows_cap, int64_t* n_local,
                                double* max_violation);
int scp_solver_shard_round_done(scp_solver* s, int64_t n_all, double max_violation_all, scp_qp_record* rec, int* more);
int scp_solver_shard_end(scp_solver* s, double* acc_out, scp_qp_record* rec);

/* ---- scenario family "grid-swap-device": B grid-swap scenarios per call ------------------------------------------------
 * Same geometry and acceptance rules as the host generator generate_grid_swap (path_planning/scenarios/
 * position_generator.py); the random draws come from a counter-based hash, so this is a family of its own (not the host's
 * numpy stream).  Scenario b depends on seeds[b] and the parameters only, never on B or on b.
 *
 * Layout.  layers = 1 (2-D) or the smallest L with L^3 >= N (3-D); per = ceil(N / layers); side = the smallest s with
 * s^2 >= per.  Agent k lies in layer L = k / per at in-layer index c = k - L per, cell (cx, cy) = (c / side, c % side); a
 * layer holds min(per, remaining) agents.  Block key = (cx / block) (side / block + 1) + cy / block; a block's local id
 * ("owner") is the rank of its key among the distinct keys of its layer, its members are its agents in ascending order
 * (m <= block^2 of them).  In 3-D every agent's z (start and goal) is L * layer_gap.
 *
 * Random numbers.  mix(z) = SplitMix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31 (uint64 arithmetic).  The number of a key (tag, layer, block, sweep,
 * round, cand, lane) is h = mix(mix(mix(mix(mix(mix(mix(mix(seed) ^ tag) ^ layer) ^ block) ^ sweep) ^ round) ^ cand) ^ lane).
 * u = (h >> 11) * 2^-53; a jitter is (2u - 1) * jitter; a coordinate is (double)cell * pitch + jitter, each product rounded.
 *   start of agent c of layer L, coordinate d (0 = x, 1 = y):  tag 1, (L, 0, 0, 0, 0, 2c + d)
 *   Fisher-Yates of candidate t in round r of block o at sweep s: tag 2, (L, o, s, r, t, i) for i = m-1 .. 1:
 *     j = ((h >> 32) (i + 1)) >> 32, swap(perm[i], perm[j]), perm starting as the identity
 *   goal jitter of that candidate's slot i, coordinate d: tag 3, (L, o, s, r, t, 2i + d)
 * Candidate t's goal of member i is cell(member perm[i]) * pitch + its jitter.
 *
 * Block draw (sweep s).  Rounds r = 0 .. max(1, max_tries / 256) - 1 of T = 256 candidates.  A candidate's score is the
 * smallest d^2 over the pairs i < j of the block (+inf for m = 1), d^2 the squared closest approach of
 * straight_line_min_distance without the sqrt: r0 = a_i - a_j, dr = (g_i - g_j) - r0, den = dr.dr,
 * s = clip(-(r0.dr) / (den > 0 ? den : 1), 0, 1), c = r0 + s dr, d^2 = c.c -- x terms before y terms, every product
 * rounded (no contraction).  A round picks its lowest-index candidate with d^2 >= min_sep^2, else the largest d^2 (lowest
 * index on ties); the block keeps the best pick over its rounds (a later round replaces it only with a strictly larger
 * d^2) and stops after the first round that has an acceptable candidate.
 *
 * Sweeps.  Sweep 0 draws every block.  Sweep s = 1 .. sweeps: every pair of a layer whose agents lie in different blocks
 * and have d^2 < min_sep^2 flags the block with the larger owner id; no flag ends the scenario's sweeps, otherwise the
 * flagged blocks are redrawn with sweep index s (a draw reads its own block's agents only, so redrawing them together is
 * the host's sequential redraw).
 *
 * Statistics per scenario (scp_gen_stats, DEVICE array of B): sweeps = redraw sweeps done; unmet_blocks = blocks whose
 * draw has no acceptable candidate; conflicts = cross-block pairs of a layer left with d^2 < min_sep^2; min_approach =
 * sqrt(min d^2 over all pairs of the scenario, z included; +inf for N = 1); ok = min_approach >= min_sep.
 * space[b] = [lo_0 .. lo_{D-1}, hi_0 .. hi_{D-1}], lo = min(init, goal) - 2, hi = max(init, goal) + 2 per coordinate.
 *
 * Supported: 1 <= N <= 65536, B >= 1, D in {2, 3}, 2 <= block <= 8 (m <= 64), finite pitch / layer_gap / min_sep >= 0,
 * jitter >= 0, 0 <= sweeps <= 1000; anything else returns SCP_ERR_INVALID.  init / goal [B][N][D], space [B][2D] and stats
 * are DEVICE pointers, seeds [host].  Enqueued on the ctx's stream; one 4-byte host read per sweep; synchronises. */
typedef struct scp_gen_params {
  double pitch;      /* 2.0: grid pitch (m) */
  double jitter;     /* 0.2: start / goal jitter, uniform in [-jitter, jitter) per coordinate */
  double layer_gap;  /* 2.0: z distance of the layers (3-D) */
  double min_sep;    /* 0.3: closest straight-line approach a draw aims at */
  int32_t block;     /* 4: goals are permuted inside block x block cells */
  int32_t max_tries; /* 8192: candidates per block draw (256 per round) */
  int32_t sweeps;    /* 20: cross-block sweeps at most */
  int32_t reserved;  /* 0 */
} scp_gen_params;

typedef struct scp_gen_stats {
  int32_t sweeps;        /* redraw sweeps this scenario needed */
  int32_t unmet_blocks;  /* blocks without an acceptable candidate */
  int64_t conflicts;     /* cross-block pairs left closer than min_sep */
  double min_approach;   /* closest straight-line approach over all pairs */
  int32_t ok;            /* min_approach >= min_sep */
  int32_t reserved;
} scp_gen_stats;

void scp_gen_default_params(scp_gen_params* p);
int scp_generate_grid_swap(scp_ctx* ctx, int B, int N, int D, const uint64_t* seeds /* [host] B */, const scp_gen_params* p,
                           double* init /* [B][N][D] */, double* goal /* [B][N][D] */, double* space /* [B][2D] */,
                           scp_gen_stats* stats /* [B] */);

/* ---- goal assignment for interchangeable vehicles: batched exact auction ------------------------------------------------
 * A purely additive part of ABI version 7: two structs and two functions, nothing else changes.
 * For each of B scenarios: the bijection goal_of (vehicle i flies to goal[goal_of[i]]) that minimises the sum of the squared
 * start-goal distances, exactly on costs quantised per scenario.  Integer arithmetic after the quantisation, so a CPU
 * restatement (tests/assignment_ref.py) agrees bit for bit.  Such an assignment has (s_i - s_j).(g_i - g_j) >= 0 for every pair
 * (exchange argument), so no two equal-time straight-line motions are opposed: head-on swaps cannot occur.
 *
 * Quantisation (per scenario; every product rounded, no contraction; coordinates d ascending).
 *   span_d = max - min over all 2N points;  Bd = sum_d span_d * span_d;  Bd = m 2^e with m in [0.5, 1) (frexp), s = 31 - e
 *   (s = 0 if Bd == 0);  d2_ij = sum_d (start_i[d] - goal_j[d])^2;  c_ij = (int64) floor(ldexp(d2_ij, s)), which is below 2^31
 *   because d2 <= Bd by the monotonicity of rounding;  a_ij = -(N + 1) c_ij;  quantum = ldexp(1, -s)  (m^2 per unit of c).
 *
 * Auction (Jacobi forward auction with epsilon scaling; prices p_j int64, starting at 0).
 *   eps_0 = max(1, ((N + 1) floor(ldexp(Bd, s))) / 2); the next eps is max(1, eps / 4) (integer division); the phase with
 *   eps = 1 is the last.  A phase starts with every person unassigned and keeps the prices of the previous phase.  In a round
 *   EVERY unassigned person i computes v_ij = a_ij - p_j over all j, j1 = argmax (lowest j on ties), w1 = v_ij1, w2 = the
 *   maximum over j != j1, and bids p_j1 + (w1 - w2) + eps for goal j1.  Every goal that received bids takes the highest
 *   (lowest i on ties): its price becomes that bid, its previous owner becomes unassigned.  The phase ends when nobody is
 *   unassigned.  N = 1: the identity, 0 phases.
 * Consequences: the costs are integers scaled by N + 1 and the last eps is 1, so goal_of is EXACTLY optimal for c (in m^2:
 * sum d2 within N quantum of the true optimum); a_{i,goal_of[i]} - p_{goal_of[i]} >= max_j (a_ij - p_j) - 1 with the returned
 * prices; hence c_{i,gi} + c_{j,gj} <= c_{i,gj} + c_{j,gi} for all pairs; prices stay below 2^55.
 *
 * Guard.  max_rounds_per_phase <= 0 means 256 N + 4096 (about 50 x the longest phase observed, ~5 N).  A scenario whose phase
 * is not finished after that many rounds gets status = 1, goal_of = the identity and cost_q = cost_q_identity (phases, rounds,
 * bids and prices as they stood when it stopped); the call still returns SCP_OK.
 *
 * One workgroup per scenario in one launch: prices, owners and the bid table in LDS, one wave per bidding person; no
 * workgroup waits for another.  Supported: B >= 1, 1 <= N <= 4096, D in {2, 3}, finite coordinates whose range does not
 * overflow; anything else returns SCP_ERR_INVALID (for the coordinates: after the launch, outputs then undefined).
 * start / goal [B][N][D], goal_of [B][N], prices [B][N] (or NULL) and stats [B] are DEVICE pointers.  Enqueued on the ctx's
 * stream; synchronises. */
typedef struct scp_assign_stats {  /* DEVICE, one per scenario, 48 bytes */
  int64_t cost_q;           /* sum_i c[i][goal_of[i]] */
  int64_t cost_q_identity;  /* sum_i c[i][i] */
  double quantum;           /* 2^-s, m^2 */
  int64_t rounds, bids;     /* over all phases; bids = persons that bid, summed over the rounds */
  int32_t phases, status;   /* 0 ok, 1 round limit */
} scp_assign_stats;
int scp_assign_goals(scp_ctx* ctx, int B, int N, int D, const double* start /* [B][N][D] */, const double* goal /* [B][N][D] */,
                     int32_t* goal_of /* [B][N] */, int64_t* prices /* [B][N] or NULL */, int64_t max_rounds_per_phase,
                     scp_assign_stats* stats /* [B] */);

/* The same rule with the state in global memory and, for the rounds in which many persons bid, the whole GPU behind one
 * scenario (a further additive part of ABI version 7: this one function).  Arguments, outputs, the rule (quantisation,
 * auction, guard, status 0 / 1, the behaviour on unusable coordinates), stream and synchronisation are scp_assign_goals's;
 * supported: B >= 1, 1 <= N <= 65536, D in {2, 3}.  For every input both functions accept, goal_of, prices and every field of
 * stats (rounds, bids and phases included) are the same bytes; for every N they are those of tests/assignment_ref.py.
 *
 * Price bound for this range.  Let C = (N + 1) 2^31 (so |a_ij| < C).  A goal that received a bid in a phase stays owned until
 * the phase ends, and the phase ends once every goal is owned.  So in every round but a phase's last, each bidder i with
 * target j1 finds a goal j0 != j1 that has received no bid in this phase (if only one such goal is left and somebody bids
 * for it, the round is the last).  j0 is still at its price p0_j0 of the phase's start, and w2 >= a_ij0 - p0_j0 gives
 * bid = a_ij1 - w2 + eps <= (a_ij1 - a_ij0) + p0_j0 + eps < C + P0 + eps (P0: the highest price at the phase's start).  In
 * the last round w2 >= a_ij - p_j for any j != j1 at its current price, so a bid stays below C + eps + the highest current
 * price.  So a phase raises the highest price by less than 2 (C + eps).  eps_0 <= C / 2 < 2^47 reaches 1 after at
 * most 24 divisions by 4, so there are at most 25 phases, and the sum of their eps is at most (4/3) eps_0 + 25.  Hence
 *   prices <= 50 C + (4/3) C + 50 < 52 (N + 1) 2^31, which is below 2^53 at N = 65536 (and below 2^49 at N = 4096);
 * v_ij = a_ij - p_j and every bid then stay within +-2^54: every intermediate fits int64 with nine bits to spare.
 * (tests/test_assignment_wide_cpu.py checks the bound on the reference's prices.)
 *
 * Rounds with few bidders run in one workgroup per scenario, round after round in one launch; rounds with many run as three
 * launches whose grids cover (scenario, bidder); DESIGN.md section 3.8 has the launch sequence.  No workgroup waits for
 * another.  Developer switches (scp_ctx_set_option; results never depend on them): "assign_wide_min_bidders" (0: chosen by the
 * call; otherwise rounds with at least that many bidders take the three launches: 1 = every round, a value >= N = none),
 * "assign_wide_prices_in_lds" (-1 auto, 0: the one-workgroup rounds read the prices from global memory, 1: from LDS where
 * 8 N bytes fit, N <= 16384), "assign_wide_control_threads" (0: 256 threads in the one workgroup up to N = 512 and 1024
 * beyond; 256 or 1024: that many). */
int scp_assign_goals_wide(scp_ctx* ctx, int B, int N, int D, const double* start /* [B][N][D] */,
                          const double* goal /* [B][N][D] */, int32_t* goal_of /* [B][N] */, int64_t* prices /* [B][N] or NULL */,
                          int64_t max_rounds_per_phase, scp_assign_stats* stats /* [B] */);

/* The same auction on costs the caller states (a further additive part of ABI version 7: this one function and one
 * constant).  The rule of scp_assign_goals word for word -- phases, eps scaling, bids, tie rules, the guard and its identity
 * fallback with status 1, N = 1 -- with
 *   c_ij = cost[b][i][j]  (person i, goal j; 0 <= c_ij <= SCP_ASSIGN_MAX_COST),   top = max_ij c_ij of the scenario,
 *   eps_0 = max(1, ((N + 1) top) / 2),   stats.quantum = 1.0,   cost_q / cost_q_identity = the sums of the entries.
 * goal_of is EXACTLY optimal for the matrix (sum_i cost[i][goal_of[i]] is minimal); tests/assign_paths_ref.py restates the
 * rule, and on the matrix c and the top of scp_assign_goals's quantisation it gives that call's bytes.  The price bound above
 * (C = (N + 1) 2^31) holds as written.  A negative entry raises the mapped host word like unusable coordinates: the call
 * returns SCP_ERR_INVALID after the launch, outputs then undefined.  One workgroup per scenario -- the kernel of
 * scp_assign_goals with its costs loaded from row i of the matrix (a bidding wave reads consecutive words) instead of
 * recomputed from coordinates; the matrix is read once more at the start for top.  Supported: B >= 1, 1 <= N <= 4096 (there is
 * no wide form: an N x N matrix for 65536 vehicles is out of scope).  cost [B][N][N], goal_of [B][N], prices [B][N] (or NULL)
 * and stats [B] are DEVICE pointers.  Enqueued on the ctx's stream; synchronises; timing through scp_ctx_last_pair_ms. */
#define SCP_ASSIGN_MAX_COST 2147483647
int scp_assign_costs(scp_ctx* ctx, int B, int N, const int32_t* cost /* DEVICE [B][N][N], cost[b][i][j] */,
                     int32_t* goal_of /* [B][N] */, int64_t* prices /* [B][N] or NULL */, int64_t max_rounds_per_phase,
                     scp_assign_stats* stats /* [B] */);

/* Straight-line check: one pass per scenario over the pairs i < j of the motions start_i -> goal[goal_of[i]] (goal_of NULL:
 * the identity).  d^2 is the squared closest approach of the "Block draw" rule above (the generator's device function, so a
 * grid-swap-device scenario's min_approach is scp_gen_stats.min_approach bit for bit), with r0 = s_i - s_j and
 * g = g_i - g_j; in 3-D the z terms come last.  A pair is opposed if sum_d r0[d] * g[d] < 0 (d ascending, no contraction),
 * close if d^2 < min_sep * min_sep.  Deterministic.  Supported: B >= 1, 1 <= N <= 65536, D in {2, 3}, finite min_sep >= 0,
 * goal_of entries in [0, N); anything else returns SCP_ERR_INVALID (for the entries: after the launch).  All pointers DEVICE;
 * stream and synchronisation as scp_assign_goals. */
typedef struct scp_line_stats {  /* DEVICE, one per scenario, 32 bytes */
  double min_approach;  /* sqrt(min d^2); +inf for N = 1 */
  int32_t arg_i, arg_j; /* the pair that attains it, the lowest (i, j) on ties; -1, -1 for N = 1 */
  int64_t n_close;      /* pairs with d^2 < min_sep^2 */
  int64_t n_opposed;    /* pairs with (s_i - s_j).(g_i - g_j) < 0 */
} scp_line_stats;
int scp_straight_line_check(scp_ctx* ctx, int B, int N, int D, const double* start, const double* goal,
                            const int32_t* goal_of /* [B][N] or NULL */, double min_sep, scp_line_stats* stats /* [B] */);

/* ---- static obstacles: safe flight corridors as per-step position boxes ---------------------------------------------------
 * A purely additive part of ABI version 7: three structs and seven functions; no other entry point changes its behaviour or
 * its bits while no boxes are set.  The obstacles are an occupancy grid; for every vehicle and every segment a box of free
 * cells is grown around a reference path; state j must lie in the intersection of the boxes of the two segments it ends,
 * which in the joint QP is a change of the bounds of position rows that exist already.  tests/corridor_ref.py restates every
 * rule below in numpy, integers exactly and doubles bit for bit.
 *
 * Conventions.  STATE j = 0 .. K is the position at time j h: states 0 .. K-1 are the stored pos[.][j], state 0 is fixed to p0
 * and state K to pf.  SEGMENT g = 0 .. K-1 runs from state g to state g + 1 with the kinematics of scp_check_separation:
 * inside it a coordinate is p + t v + t^2/2 a, (p, v, a) = (pos, vel, acc)[i][g][d], t in [0, h].  Every floating-point
 * formula below is evaluated with each product, quotient, sum and difference rounded on its own (no contraction).  max / min
 * of two doubles take the first operand unless the second is strictly greater / smaller; NaN inputs are not supported except
 * where a rule names them.
 *
 * Grid.  Cell (x, y, z) is the closed cube [origin_d + cell c_d, origin_d + cell (c_d + 1)] per coordinate; occ[(z ny + y) nx + x]
 * != 0 means occupied.  In 2-D nz = 1 and origin[2] is ignored.  Supported: D in {2, 3}, every dim >= 1, nx ny nz <= 2^24,
 * D = 2 => nz = 1, cell > 0 and finite, finite origin; anything else returns SCP_ERR_INVALID with a message.
 *
 * scp_occupancy_prepare: sat[(z ny + y) nx + x] = the number of occupied cells (x', y', z') with x' <= x, y' <= y, z' <= z
 * (the inclusive prefix count; integers only).  Separate from the corridor call so that re-planning with new reference
 * paths reuses it.  One launch per dimension (a wave scans a row along x, a thread walks a column along y / z); enqueued on
 * the ctx's stream, no host read.  The number of occupied cells in the cell range [a, b] (inclusive per coordinate) is the
 * inclusion-exclusion sum of sat over the 4 (8) corners (b or a - 1 per coordinate, a term with an index -1 is 0). */
typedef struct scp_occupancy_grid { /* [host] */
  double origin[3]; /* lower corner of cell (0,0,0); origin[2] ignored in 2-D */
  double cell;      /* edge length, > 0, finite */
  int32_t dims[3];  /* nx, ny, nz; nz = 1 in 2-D */
  int32_t reserved;
} scp_occupancy_grid;
int scp_occupancy_prepare(scp_ctx* ctx, int D, const scp_occupancy_grid* grid,
                          const uint8_t* occ /* DEVICE [nz][ny][nx], x fastest, nonzero = occupied */,
                          int32_t* sat /* DEVICE, nx*ny*nz words */);

/* scp_corridor_boxes: the box of segment g of vehicle i, in cells, from the reference points ref[i][g] and ref[i][g + 1].
 *   Cell lookup.  f_d(x) = floor((x - origin_d) / cell): one subtraction, one division.  The coordinate is INSIDE if it is
 *     finite and 0 <= f_d(x) < dims_d (compared as doubles); then c_d(x) = (int) f_d(x).
 *   Seed.  lo_d = min(c_d(ref[g]), c_d(ref[g+1])), hi_d = the max, d < D; in 2-D lo_z = hi_z = 0.
 *   Blocked.  If a coordinate (d < D) of either point is not inside, or the seed range [lo, hi] holds an occupied cell, the
 *     segment is BLOCKED: its record is (0, 0, 0, -1, -1, -1) and it counts in *n_blocked.
 *   Sweeps.  Otherwise sweeps repeat until a sweep extends nothing.  A sweep takes the directions in the order -x, +x, -y, +y
 *     (3-D: then -z, +z).  Direction -d extends the box by one cell (lo_d -= 1) if (a) seed_lo_d - lo_d < max_grow, (b)
 *     lo_d - 1 >= 0 and (c) the slab {c_d = lo_d - 1} x the box's CURRENT range in the other coordinates holds no occupied
 *     cell; direction +d likewise with hi_d - seed_hi_d < max_grow, hi_d + 1 < dims_d and the slab {c_d = hi_d + 1}.
 *     Extensions made earlier in the same sweep count.  (A direction that fails once fails ever after, so there are at most
 *     2 D max_grow + 1 sweeps.)
 * The record is cells[(i K + g) 6 ..] = lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, inclusive.  A box never holds an occupied cell
 * nor a cell outside the grid, contains both seed cells and is locally maximal.  Integers after the cell lookup; the result
 * does not depend on the launch geometry.  One THREAD per (vehicle, segment): the work of a segment is a short serial chain
 * of dependent table reads (4 per slab in 2-D, 8 in 3-D), which more lanes cannot shorten.
 * Supported: N, K >= 1, 0 <= max_grow <= 1024.  *n_blocked is written (not accumulated).  No host read. */
int scp_corridor_boxes(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* sat,
                       const double* ref /* DEVICE [N][K+1][D]: reference point of every state */,
                       int max_grow /* 0 .. 1024 cells */,
                       int32_t* cells /* DEVICE [N][K][6] */, uint64_t* n_blocked /* DEVICE */);

/* scp_corridor_state_boxes: the boxes of the states in metres.
 *   Segment box.  L_d = origin_d + cell * (double)lo_d,  H_d = origin_d + cell * (double)(hi_d + 1).
 *   State j = 1 .. K-1.  lo_d = max(L_d(seg j-1), L_d(seg j)) + shrink,  hi_d = min(H_d(seg j-1), H_d(seg j)) - shrink.
 *   Open.  If either segment is blocked, or lo_d > hi_d for some d, the WHOLE state gets (-inf, +inf) in every coordinate
 *     and counts in *n_open (written, not accumulated).  State 0 is always (-inf, +inf) and does not count.
 * Why the shrink: inside a segment a coordinate is a quadratic in t, which leaves the chord of its end values by at most
 * |a_d| h^2 / 8 (the maximum of t (h - t) / 2 |a_d|).  With shrink >= acc_max_abs h^2 / 8 + pad the end states lie in the
 * shrunk intersections, both of which lie inside box g shrunk by `shrink`, so the whole segment lies inside box g -- up to
 * the QP's constraint tolerance, which `pad` pays for.  Supported: finite shrink >= 0.  lo / hi are [N][K][D], indexed by
 * state j = 0 .. K-1.  One thread per (vehicle, state).  No host read. */
int scp_corridor_state_boxes(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* cells,
                             double shrink /* >= 0 */, double* lo, double* hi /* DEVICE [N][K][D] */,
                             uint64_t* n_open /* DEVICE */);

/* scp_qp_set_position_boxes: per-(vehicle, state) position boxes into the bounds of the QP.  Call it after
 * scp_qp_set_problem.  For state j = 1 .. K-1 and column c = (i, d) it rewrites row k = j - 1 of the position block of the
 * fixed bounds (row 3K - 1 + k of "lf" / "uf"):
 *   l = max(space_min_d, lo[i][j][d]) - off,   u = min(space_max_d, hi[i][j][d]) - off,
 *   off = p0 + hk * v0 with hk = h * (double)(k + 1)   (the offset of scp_fixed_bounds),
 * space, p0, v0 those of the latest scp_qp_set_problem.  Entry j = 0, the final row k = K - 1 and every other block keep
 * their bits; entries (-inf, +inf) reproduce the bits of scp_qp_set_problem.  l > u is the caller's error (the QP is then
 * infeasible; path_planning checks it on the host).  Enqueues one launch, no host read.  While boxes are set the QP's
 * persistent path runs the round-2 kernel (SCP_PIPE_PERSIST) where it fits and the three-launch pipeline otherwise, never
 * a lean kernel (SCP_PIPE_PERSIST16 / SCP_PIPE_PERSIST8L re-derive the bounds from space and the states), whatever
 * settings.persistent says.  scp_qp_set_problem rewrites the bounds and so clears the boxes; scp_qp_clone_state copies
 * them.  lo = hi = NULL is a no-op; exactly one NULL returns SCP_ERR_INVALID. */
int scp_qp_set_position_boxes(scp_qp* qp, const double* lo, const double* hi /* DEVICE [N][K][D] by state, or both NULL */);
/* The solver keeps the two pointers (the arrays must outlive its calls) and applies them right after every
 * scp_qp_set_problem it makes -- QP#0, every step, a QP that moves to a larger workspace.  Both NULL: none (the default). */
int scp_solver_set_position_boxes(scp_solver* s, const double* lo, const double* hi);

/* scp_check_corridor: does every segment stay inside its (un-shrunk) box?  Exact per segment and coordinate: the candidates
 * are t = 0, t = h and t* = -v / a if a != 0 and 0 < t* < h; the value at t is p + (t * v + ((0.5 * t) * t) * a) (the formula
 * of scp_update_holds); lo_v / hi_v = the min / max over the candidates;
 *   excess(segment) = max over d of max(L_d - lo_v, hi_v - H_d)      (<= 0: inside)
 * with L, H of scp_corridor_state_boxes.  Blocked segments are counted, not judged.  Per vehicle: max_excess over its judged
 * segments and the lowest g that attains it, n_blocked, n_outside = judged segments with excess > tol.  One wave per
 * vehicle; deterministic.  Supported: finite h > 0, finite trajectories.  No host read. */
typedef struct scp_corridor_stats { /* DEVICE, one per vehicle, 32 bytes */
  double max_excess;  /* <= 0: inside; -inf: no segment judged */
  uint32_t segment;   /* where (lowest g on ties); UINT32_MAX: none */
  uint32_t n_blocked; /* its blocked segments (not judged) */
  uint64_t n_outside; /* judged segments with excess > tol */
  uint64_t reserved;
} scp_corridor_stats;
int scp_check_corridor(scp_ctx* ctx, int N, int K, int D, double h, const scp_occupancy_grid* grid, const int32_t* cells,
                       const double* pos, const double* vel, const double* acc /* DEVICE [N][K][D] */, double tol,
                       scp_corridor_stats* out /* DEVICE [N] */);

/* ---- static obstacles: reference paths by a lattice search ------------------------------------------------------------------
 * A further additive part of ABI version 7: one struct and two functions; nothing above changes.  They find, for every
 * vehicle, a path of free lattice nodes from its start to its goal and sample it at the states j = 0 .. K: the `ref` of
 * scp_corridor_boxes for maps where the straight line is blocked.  Grid, cell lookup f_d, "inside" and the summed-table range
 * count are those of scp_occupancy_prepare / scp_corridor_boxes.  Integers everywhere except the two formulas of "reference
 * points", which are evaluated without contraction.  tests/reference_path_ref.py restates every rule in numpy / plain Python.
 *
 * Lattice.  Parameters: stride s >= 1 and clearance c >= 0, both in cells.  L_d = dims_d div s for d < D, L_z = 1 in 2-D.
 *   Supported: every L_d >= 1 and nodes = L_x L_y L_z <= SCP_LATTICE_MAX_NODES; anything else returns SCP_ERR_INVALID with a
 *   message.  Node (X, Y, Z) has the id (Z L_y + Y) L_x + X; its BLOCK is the cell range [X_d s, X_d s + s - 1] per
 *   coordinate d < D (z: [0, 0] in 2-D).  Cells beyond L_d s belong to no node.
 * Directions.  A code n = 0 .. 26 means dx = n mod 3 - 1, dy = (n div 3) mod 3 - 1, dz = n div 9 - 1; 2-D uses the codes with
 *   dz = 0; code 13 is the node itself.  DIRECTION ORDER: the codes other than 13 sorted by |dx| + |dy| + |dz|, then by code
 *   (straight moves before diagonal ones).
 *
 * scp_lattice_edges (once per map, stride and clearance; independent of the vehicles).  Bit n of edges[node] is set iff the
 *   neighbour in direction n lies in the lattice AND the cell range spanned by the two blocks (min of the lows, max of the
 *   highs), grown by c cells per coordinate d < D on both sides and then clipped to the grid, holds no occupied cell: one
 *   summed-table query (4 reads in 2-D, 8 in 3-D).  Bit 13 is therefore "the node's grown block is free" (the node is
 *   PASSABLE) and is implied by every other set bit; bits 27 .. 31 are 0; edges are symmetric; a diagonal edge exists only
 *   if the whole 2 x 2 (2 x 2 x 2) group of blocks is free, so a path never cuts a corner.  One thread per node.
 *
 * scp_reference_paths, per vehicle i from p0[i], pf[i]:
 *   Start node: the cell of p0 by the cell lookup, X_d = c_d div s.  STATUS 1 if a coordinate (d < D) is not inside, or some
 *     X_d >= L_d, or the node is not passable.  STATUS 2: the same for the goal, tested only if the start passed.
 *   dist: the breadth-first distance from the GOAL node over the edges at unit cost, uint16, 0xFFFF = unreached (a reached
 *     distance is at most 32767).  STATUS 3 if the start is unreached.  m = dist[start] + 1 is the number of nodes of the
 *     path; STATUS 4 if m > max_path.
 *   Path: node_0 = start; node_{t+1} = the first neighbour of node_t, in direction order, whose edge bit is set and whose
 *     dist equals dist(node_t) - 1.  dist is unique, so nothing depends on how the search is scheduled.
 *   Reference points: V_0 = p0; for t = 1 .. m, V_t = the centre of node_{t-1}: origin_d + cell * ((double)(X_d s) + 0.5 *
 *     (double)s); V_{m+1} = pf; E = m + 1.  For state j = 0 .. K, with q = (j E) div K and r = (j E) mod K in 64-bit integers:
 *     the point is V_E if q == E (only j = K), otherwise V_q + ((double)r / (double)K) * (V_{q+1} - V_q), every operation
 *     rounded on its own, also for r = 0.  Only coordinates d < D are written.
 *   A vehicle with status != 0: its rows of `ref` are NOT written (ref is in/out: the caller's pre-filled points stay), its
 *     path row is all -1 and its n_nodes 0.  info[i].start_node / goal_node is the node's id wherever the point lies on the
 *     lattice and was tested, else -1 (the goal is not tested with status 1).  *n_failed is written, not accumulated.
 *   dist_out (for tests): the vehicle's dist as the search leaves it.  The search stops after the level that reaches the
 *     start, so nodes farther from the goal than the start read 0xFFFF like the unreachable ones; with status 1 or 2 every
 *     entry reads 0xFFFF, with start node = goal node every entry but the goal's.
 * Why such a path serves as a corridor reference: if E <= K, two consecutive reference points lie on one edge or on two
 * adjacent ones, so their seed range lies inside cell ranges the edge rule has found free: scp_corridor_boxes reports no
 * blocked segment for that vehicle at any clearance >= 0.  Beyond that, with f = ceil(E / K), 2 c >= s f is sufficient.
 *
 * ONE workgroup per vehicle and no workgroup waits for another; dist lives in the workgroup's LDS (64 KiB plus a few
 * control words, static, two workgroups per CU); the search runs level by level with one barrier per level, at most `nodes`
 * levels, and stops as soon as the start is reached or a level changes nothing; one thread then walks the path and the
 * threads write the K + 1 points side by side.  The edge masks are read from global memory.  Supported: N, K >= 1, 1 <=
 * max_path <= nodes, the same stride as the edges were made with.  Both calls: argument checks, enqueue on the ctx's stream,
 * no host read, timing through scp_ctx_last_pair_ms. */
#define SCP_LATTICE_MAX_NODES 32768
int scp_lattice_edges(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const int32_t* sat, int stride, int clearance,
                      uint32_t* edges /* DEVICE [nodes] */);
typedef struct scp_path_info { /* DEVICE, one per vehicle, 16 bytes */
  int32_t status;     /* 0 found; 1 start, 2 goal off the lattice or not passable; 3 unreachable; 4 longer than max_path */
  int32_t n_nodes;    /* m; 0 unless status == 0 */
  int32_t start_node; /* -1 where it could not be determined */
  int32_t goal_node;
} scp_path_info;
int scp_reference_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                        const double* p0, const double* pf /* DEVICE [N][D] */, int max_path,
                        double* ref /* DEVICE [N][K+1][D], in/out */,
                        int32_t* path /* DEVICE [N][max_path] or NULL; entries beyond n_nodes are -1 */,
                        scp_path_info* info /* DEVICE [N] */, uint16_t* dist_out /* DEVICE [N][nodes] or NULL */,
                        uint64_t* n_failed /* DEVICE */);

/* Lattice distances (a further additive part of ABI version 7: this one function): the hop counts of the search between
 * EVERY source and EVERY destination, for costs that see the obstacles (scp_assign_costs).  The lattice, the node of a point
 * and "passable" are those of scp_lattice_edges / scp_reference_paths; edges are the masks scp_lattice_edges made with the
 * same stride.  Integers only; tests/assign_paths_ref.py restates the rule.
 *   Node of a point: its node id, or -1 where scp_reference_paths would give status 1 or 2: a coordinate (d < D) is not
 *     inside the grid, some X_d >= L_d, or the node is not passable.  src_node[a] / dst_node[b] report it.
 *   dist of source a: the breadth-first distance from src_node[a] over the set edge bits at unit cost (a diagonal move counts
 *     1), uint16, 0xFFFF = unreached.  The field is COMPLETE: the search ends when a level changes nothing.  With
 *     src_node[a] = -1 every entry reads 0xFFFF.
 *   hops[a][b] = dist[dst_node[b]]; 0xFFFF if either node is -1 or the destination is unreached; 0 on the same node.  Edge
 *     masks are symmetric, so the search from the start gives the distances of a search from the goal.
 *   dist_out (for tests): the complete field of every source.
 * ONE workgroup per source and no workgroup waits for another; dist lives in the workgroup's LDS (the layout of
 * scp_reference_paths: 64 KiB plus a few control words, static, two workgroups per CU); the level sweep is that call's, one
 * barrier per level, at most `nodes` levels; every workgroup looks the destinations' nodes up for itself.  The workgroup
 * width follows "ref_path_threads".  Supported: n_src, n_dst >= 1, nodes <= SCP_LATTICE_MAX_NODES.  Argument checks, enqueue
 * on the ctx's stream, no host read, timing through scp_ctx_last_pair_ms as scp_reference_paths. */
int scp_lattice_distances(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                          int n_src, const double* src /* DEVICE [n_src][D] */, int n_dst,
                          const double* dst /* DEVICE [n_dst][D] */, uint16_t* hops /* DEVICE [n_src][n_dst] */,
                          int32_t* src_node /* DEVICE [n_src] */, int32_t* dst_node /* DEVICE [n_dst] */,
                          uint16_t* dist_out /* DEVICE [n_src][nodes] or NULL */);

/* ---- static obstacles: shortened reference paths ------------------------------------------------------------------------------
 * A further additive part of ABI version 7: one struct and one function; nothing above changes.  The path of
 * scp_reference_paths is a lattice path: it minimises the number of moves, takes straight moves before diagonal ones, and
 * passes through the centres of the start and the goal block.  scp_shorten_paths keeps only the nodes that cannot be skipped
 * and places the K + 1 reference points evenly by chord length.  Grid, cell lookup, the summed-table range count, lattice,
 * node ids, blocks and block centres are those of scp_lattice_edges / scp_reference_paths.  Integers everywhere except
 * "lengths" and "reference points", which are doubles with every operation rounded on its own (no contraction).
 * tests/shorten_ref.py restates every rule in numpy / plain Python.
 *
 * Visibility clear(A, B) of two lattice nodes, with stride s and clearance c.  X^A, X^B the node coordinates, d = X^B - X^A,
 *   n = max over the coordinates q < D of |d_q|.  n = 0 is clear.  For each step k = 0 .. n-1 and coordinate q < D:
 *     u0 = X^A_q n + d_q k,  u1 = u0 + d_q  (both >= 0),  lo_q = min(u0, u1) div n,  hi_q = (max(u0, u1) + n - 1) div n;
 *   the step's cell range is [lo_q s - c, hi_q s + s - 1 + c], clipped to the grid (z: [0, 0] in 2-D).  clear holds iff no
 *   step's range holds an occupied cell: one summed-table query per step.  Evaluation may stop at the first occupied step.
 *   A node id outside the lattice is clear of nothing.  Consequences: clear is symmetric (step k of (B, A) has the range of
 *   step n-1-k of (A, B)); for lattice neighbours it equals the edge bit of scp_lattice_edges made with the same (s, c);
 *   every point of the segment between the two block centres lies in the un-grown range of some step (at parameter
 *   (k + x) / n, 0 <= x <= 1, coordinate q of the centre line is (u0 + x d_q) / n + 1/2 blocks, inside [lo_q, hi_q + 1]), so
 *   every cell within c cells of the segment is free; and the same holds with one or both centres replaced by any point of
 *   that end's block, which moves every point of the segment by at most s / 2 cells per coordinate while the un-grown step
 *   ranges extend s / 2 beyond the centre line.
 * Kept nodes, for a vehicle with status 0 and path node_0 .. node_{m-1}: t_0 = 0; while t_i < m - 1, t_{i+1} is the LARGEST t
 *   in (t_i, m-1] with clear(node_{t_i}, node_t).  It exists where the path was made with the same (s, c): t_i + 1 is a
 *   neighbour over a set edge (where no t is clear -- a path of other parameters -- t_i + 1 is taken).  The kept list t_0 <
 *   .. < t_{n-1} = m - 1 has n = n_kept >= 1 entries (m = 1: n = 1) and does not depend on how the candidates are scheduled.
 * Vertices.  nv = max(n, 2); W_0 = p0, W_{nv-1} = pf, and for 0 < i < n-1 W_i = the centre of node_{t_i} (the block-centre
 *   formula of scp_reference_paths).  The centres of the start block and of the goal block are NOT vertices.
 * Lengths.  len_i = sqrt(sum over d < D, in order, of (W_{i+1,d} - W_{i,d})^2), the sum starting from 0.0; S_0 = 0, S_{i+1} =
 *   S_i + len_i; length = S_{nv-1}.  length_before is the same sum over V_0 .. V_{m+1} of scp_reference_paths.
 * Reference points by chord length.  State 0 is W_0, state K is W_{nv-1}.  For 0 < j < K: target = ((double)j / (double)K) *
 *   length; i = the smallest index with S_{i+1} >= target; if len_i == 0 the point is W_i, otherwise w = min((target - S_i) /
 *   len_i, 1.0) and the point is W_i + w * (W_{i+1} - W_i).  Only coordinates d < D are written.
 * A vehicle whose status is not 0 keeps its rows of `ref`; its kept row is all -1 and its record all zeros.  kept[i][e] = t_e
 * for e < n_kept (an index into the vehicle's path row), -1 beyond.
 * Why it serves as a corridor reference: consecutive reference points are at most length / K apart along the polyline,
 * hence in every coordinate, so their cells differ by at most delta = floor(length / (K cell)) + 1 per coordinate.  Both
 * points lie on one edge of the polyline or on two adjacent ones; if c >= delta, their seed range of scp_corridor_boxes lies
 * inside a step range grown by c, which was found free: no segment of that vehicle is blocked.  With c = s that holds for
 * every path shorter than K block edges.
 *
 * ONE wave per vehicle: the lanes test 64 candidates t at a time from the goal's end, the first block of 64 in which a lane
 * sees the anchor ends the anchor's search (the largest t by ballot); the lanes then sum the lengths and write the points side
 * by side.  No LDS, no barrier, no workgroup waits for another; every loop is bounded: anchors <= m, blocks <= ceil(m / 64)
 * per anchor, steps <= max L_d per candidate.  The outputs do not depend on the launch geometry.  kept = NULL: the list lives in
 * the context's workspace.  Supported: N, K >= 1, 1 <= max_path <= nodes, clearance >= 0 (beyond the grid's widest dimension
 * it is that dimension), path / info as scp_reference_paths wrote them with the same stride and max_path.  Argument checks,
 * enqueue on the ctx's stream, no host read, timing through scp_ctx_last_pair_ms. */
typedef struct scp_shorten_info { /* DEVICE, one per vehicle, 24 bytes */
  int32_t n_kept;       /* n; 0 unless the vehicle's status == 0 */
  int32_t n_vertices;   /* nv; 0 likewise */
  double length;        /* of the shortened polyline */
  double length_before; /* of p0, the block centres, pf */
} scp_shorten_info;
int scp_shorten_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* sat, int stride,
                      int clearance, const double* p0, const double* pf /* DEVICE [N][D] */, int max_path,
                      const int32_t* path /* DEVICE [N][max_path], required */, const scp_path_info* info /* DEVICE [N] */,
                      double* ref /* DEVICE [N][K+1][D], in/out */, int32_t* kept /* DEVICE [N][max_path] or NULL */,
                      scp_shorten_info* out /* DEVICE [N] */);

/* ---- static obstacles: distance field and clearance ---------------------------------------------------------------------------
 * A further additive part of ABI version 7: one struct and two functions; nothing above changes.  Everything above helps a
 * plan avoid the map; these two judge a plan against it, whatever made the plan: how close does every vehicle come to the
 * occupied cells, where and when -- the counterpart of scp_clearance_profile with the map in place of the other vehicles.
 * Grid, cell lookup f_d, "inside", occ and sat are those of scp_occupancy_prepare / scp_corridor_boxes; the kinematics of a
 * segment and the min / max rule are those of scp_check_corridor.  Integers everywhere except "pieces" and "cell range",
 * whose doubles are evaluated with every operation rounded on its own (no contraction).  tests/obstacle_distance_ref.py
 * restates every rule in numpy / plain Python.
 *
 * scp_obstacle_distance (once per map and gap; independent of the vehicles).  For every cell c = (c_x, c_y, c_z)
 *     field[(c_z ny + c_y) nx + c_x] = min over the occupied cells o of  sum over q < D of max(|c_q - o_q| - gap, 0)^2,
 *   in integers; a map without an occupied cell gives UINT32_MAX everywhere.  gap = 0 is the squared Euclidean distance
 *   transform between cells (in cells).  gap = 1 is the squared distance, in cells, between the CLOSED cubes of c and o; it
 *   equals the gap = 0 field of the map dilated by one cell per coordinate (a cell is occupied if a cell within one step per
 *   coordinate is).  Guarantee of gap = 1: for any point x whose cell lookup gives c, the distance from x to the union of the
 *   closed occupied cells is at least cell * sqrt(field[c]) (x lies in the closed cube of c up to the rounding of the lookup,
 *   and the distance between two sets bounds the distance from a point of one to the other).
 *   Supported: the grids scp_occupancy_prepare supports with every dims_d <= 32768, so that a coordinate contributes less than
 *   2^30 and no sum wraps; gap 0 or 1; anything else returns SCP_ERR_INVALID with a message.  A row, column or plane without
 *   an occupied cell is an ordinary case (its cells take their values from the other coordinates).
 *   The transform is separable: a pass along x (one wave per row: two sweeps with a carry leave the squared gap distance to the
 *   nearest occupied cell of the row, UINT32_MAX without one), then along y and, in 3-D, along z one lower-envelope pass
 *   out[c] = min over n' of in[c with c_q = n'] + max(|c_q - n'| - gap, 0)^2, entries UINT32_MAX skipped: one thread per cell, x
 *   fastest, which starts from its own value, looks delta = 1, 2, .. cells to both sides and stops as soon as max(delta - gap,
 *   0)^2 reaches the best so far -- every loop is bounded by a grid dimension.  A pass reads one buffer and writes another; the
 *   second buffer (4 bytes per cell) lives in the context's workspace.  No LDS, no barrier, no workgroup waits for another;
 *   the result does not depend on the launch geometry.  Launches are enqueued on the ctx's stream, no host read, timing
 *   through scp_ctx_last_pair_ms. */
int scp_obstacle_distance(scp_ctx* ctx, int D, const scp_occupancy_grid* grid,
                          const uint8_t* occ /* DEVICE [nz][ny][nx], nonzero = occupied */, int gap /* 0 or 1 */,
                          uint32_t* field /* DEVICE [nz][ny][nx] */);

/* scp_obstacle_clearance: the guaranteed clearance of every vehicle of a plan from the occupied cells.  `field` is the gap = 1
 * field of the same grid, `sat` its summed table.
 *   Pieces.  Segment g of vehicle i is cut into `pieces` = P pieces, 1 <= P <= SCP_OBSTACLE_MAX_PIECES; piece s = 0 .. P-1 runs
 *     over [t_s, t_{s+1}] with t_s = h * ((double)s / (double)P).  Per coordinate d < D the candidates are t_s, t_{s+1} and
 *     t* = -v / a if a != 0 and t_s < t* < t_{s+1}; the value at t is p + (t * v + ((0.5 * t) * t) * a); lo_v = the min, hi_v =
 *     the max over the candidates in that order (the min / max rule above).
 *   Cell range.  flo = f_d(lo_v), fhi = f_d(hi_v), as doubles.  The piece is OFF the map, and counts in n_off, if for some
 *     d < D either value is not finite, fhi < 0 or flo >= dims_d.  Otherwise its range is [max(flo, 0), min(fhi, dims_d - 1)]
 *     per coordinate, [0, 0] along z in 2-D.  A piece whose range holds more than SCP_OBSTACLE_MAX_RANGE cells is WIDE: it
 *     counts in n_wide and is not judged (so no lane loops over the grid; a finer cut makes the pieces narrower).
 *   Judging.  The value of a judged piece is the minimum of `field` over its range, attained at the lowest linear cell index
 *     among ties.  The piece TOUCHES, and counts in n_touch, if its range holds an occupied cell (one summed-table query).
 *   Per vehicle: the smallest value over its judged pieces, the (segment, piece) and the cell where it is attained; ties keep
 *     the lowest (segment, piece), then the lowest cell.  A value of UINT32_MAX (an empty map) is never "attained": the record
 *     of a vehicle without a judged piece, or on an empty map, reads min_sq = segment = piece = UINT32_MAX, cell = -1.
 *   Per time step: step_min[g] = min over the vehicles i with a judged piece in segment g of
 *     ((smallest value over the judged pieces of segment g of vehicle i) << 32) | i,
 *     UINT64_MAX where no piece of the step was judged: a 64-bit unsigned atomic minimum, so ties go to the lowest vehicle and
 *     the array does not depend on the order of the updates.  The call initialises the array itself.
 *   Guarantee.  Every point of a judged piece lies, up to the rounding of the cell lookup, in a cell of its range (per
 *     coordinate the piece stays between lo_v and hi_v, and the lookup is monotone), so by the guarantee of the gap = 1 field
 *     the piece keeps at least cell * sqrt(value) from every occupied cell; the vehicle keeps cell * sqrt(min_sq) over all its
 *     judged pieces.  The bound is a lower bound: 0 says "may touch", and it tightens with more pieces and finer cells.  A piece
 *     that is off the map or wide carries no statement.
 * One wave per vehicle: a lane owns the segments lane, lane + 64, .. and walks their pieces, one atomic per judged segment;
 * the records are reduced by shuffles under the tie rule.  No LDS, no barrier, no workgroup waits for another; loops are
 * bounded by K, P and SCP_OBSTACLE_MAX_RANGE; the result does not depend on the launch geometry.  Supported: N, K >= 1, finite
 * h > 0, finite trajectories, the grids of scp_obstacle_distance.  Enqueued on the ctx's stream, no host read, timing through
 * scp_ctx_last_pair_ms. */
#define SCP_OBSTACLE_MAX_PIECES 16
#define SCP_OBSTACLE_MAX_RANGE 4096
typedef struct scp_obstacle_stats { /* DEVICE, one per vehicle, 32 bytes */
  uint32_t min_sq;  /* squared clearance in cells; UINT32_MAX: nothing judged, or an empty map */
  uint32_t segment; /* where: the lowest (segment, piece) on ties; UINT32_MAX: none */
  uint32_t piece;
  int32_t cell;     /* the linear index of the cell of the range that attains it (the lowest on ties); -1: none */
  uint32_t n_touch; /* judged pieces whose range holds an occupied cell */
  uint32_t n_off;   /* pieces off the map (not judged) */
  uint32_t n_wide;  /* pieces whose range holds more than SCP_OBSTACLE_MAX_RANGE cells (not judged) */
  uint32_t reserved;
} scp_obstacle_stats;
int scp_obstacle_clearance(scp_ctx* ctx, int N, int K, int D, double h, const scp_occupancy_grid* grid, const int32_t* sat,
                           const uint32_t* field /* DEVICE [nz][ny][nx], gap = 1 */, int pieces /* 1 .. 16 */,
                           const double* pos, const double* vel, const double* acc /* DEVICE [N][K][D] */,
                           scp_obstacle_stats* out /* DEVICE [N] */, uint64_t* step_min /* DEVICE [K] */);

/* ---- static obstacles: weighted search ------------------------------------------------------------------------------------------
 * A further additive part of ABI version 7: three functions; nothing above changes.  scp_reference_paths counts lattice moves,
 * a diagonal one like a straight one, and cannot tell a node beside a wall from one in open space.  These calls search the
 * same lattice by LENGTH (move weights) and, optionally, by CLEARANCE (node penalties read from the gap = 1 distance field).
 * Grid, cell lookup, lattice, node ids, blocks, direction codes, DIRECTION ORDER, edge masks and "passable" are those of
 * scp_lattice_edges / scp_reference_paths.  Everything new is integer arithmetic.  tests/weighted_path_ref.py restates every
 * rule in numpy / plain Python.
 *
 * Move weights.  W[1] = 70, W[2] = 99, W[3] = 121, indexed by len = |dx| + |dy| + |dz| of the move (99 / 70 and 121 / 70 are
 *   within 0.3 % of sqrt 2 and sqrt 3).
 * Node penalties (scp_lattice_penalties).  From `field`, the gap = 1 field of scp_obstacle_distance of the same grid (squared
 *   cells, UINT32_MAX on an empty map), the stride s, prefer >= 0 (cells) and weight >= 0:
 *     m[node]   = the minimum of field over the cells of the node's block,
 *     rho[node] = the largest integer t with t^2 <= m[node] (exact: the rounded square root corrected in integers),
 *     pen[node] = weight * (prefer - min(rho[node], prefer)),  uint32 [nodes].
 *   Supported: weight * prefer <= SCP_PENALTY_MAX_PRODUCT; anything else returns SCP_ERR_INVALID with a message.  With that a
 *   path of 32767 edges costs at most 32767 * (242 + 65536) < 2^32 - 1: costs never wrap and 0xFFFFFFFF is free to mean
 *   "unreached".  One thread per node while s^D < 64, one wave per node with a wave minimum from there on.
 * Edge cost.  w(u, v) = 2 W[len(u -> v)] + pen[u] + pen[v]: symmetric and at least 140, so a search from the goal gives the
 *   costs of a search from the start.  pen = NULL means every penalty is zero.
 * Cost field of an origin.  cost[origin] = 0; every other node holds the minimum over all walks along set edge bits of the sum
 *   of w, uint32, 0xFFFFFFFF = unreached.  The field is always COMPLETE: the search runs to its fixed point (a cheaper path
 *   may have more moves than the first one found).  The field is unique, so nothing depends on how the search is scheduled.
 *
 * scp_reference_paths_weighted: the arguments of scp_reference_paths, and pen, path_cost, cost_out.  Status 1 and 2 as there.
 *   The field is computed from the GOAL node.  STATUS 3 if cost[start] is unreached.  Path: node_0 = start; node_{t+1} = the
 *   first neighbour nb of node_t, in direction order, whose edge bit is set and for which cost[nb] + w(node_t, nb) ==
 *   cost[node_t]; costs fall strictly along the path, so the walk ends at the goal.  STATUS 4 if the goal has not been reached
 *   after max_path nodes.  m, the path row, scp_path_info, the reference points, the treatment of a vehicle with status != 0
 *   (ref untouched, path row all -1, n_nodes 0) and *n_failed follow the rules of scp_reference_paths exactly, so
 *   scp_shorten_paths consumes the outputs unchanged.  path_cost[i] = cost[start], 0xFFFFFFFF unless status 0.  cost_out (for
 *   tests): all 0xFFFFFFFF with status 1 or 2, otherwise the complete field, also when the start node is the goal node.
 * scp_lattice_costs: the arguments of scp_lattice_distances, and pen.  costs[a][b] = cost_a[dst_node[b]], the field of source
 *   a; 0xFFFFFFFF if either node is -1 or the destination is unreached; 0 on the same node.  cost_out: every source's field.
 *
 * ONE workgroup per vehicle / source and no workgroup waits for another; the field lives in the workgroup's LDS as uint32:
 * 32 KiB for lattices of at most 8192 nodes, 128 KiB of the CU's 160 KiB beyond (static; one workgroup per CU).  Sweeps in
 * pull form: a thread owns the nodes it writes, reads their neighbours and stores min(own, cost[nb] + w); every stored value
 * is the cost of a real walk and values only fall, so a racing read sees an older or a newer upper bound and the sweep that
 * changes nothing ends the search at the shortest-cost field.  One barrier per sweep, at most `nodes` sweeps, within the
 * growing box of scp_reference_paths' level sweep.  Both searches call one copy of the sweep.  Edge masks and penalties are
 * read from global memory.  The workgroup width follows "ref_path_threads".  Supported: what scp_reference_paths /
 * scp_lattice_distances support; pen made with the same stride.  Argument checks, enqueue on the ctx's stream, no host read,
 * timing through scp_ctx_last_pair_ms. */
#define SCP_PENALTY_MAX_PRODUCT 32768
int scp_lattice_penalties(scp_ctx* ctx, int D, const scp_occupancy_grid* grid,
                          const uint32_t* field /* DEVICE [nz][ny][nx], gap = 1 */, int stride, int prefer, int weight,
                          uint32_t* pen /* DEVICE [nodes] */);
int scp_reference_paths_weighted(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                 const uint32_t* edges, const uint32_t* pen /* DEVICE [nodes] or NULL */,
                                 const double* p0, const double* pf /* DEVICE [N][D] */, int max_path,
                                 double* ref /* DEVICE [N][K+1][D], in/out */,
                                 int32_t* path /* DEVICE [N][max_path] or NULL; entries beyond n_nodes are -1 */,
                                 scp_path_info* info /* DEVICE [N] */,
                                 uint32_t* path_cost /* DEVICE [N]; 0xFFFFFFFF unless status 0 */,
                                 uint32_t* cost_out /* DEVICE [N][nodes] or NULL, for tests */, uint64_t* n_failed /* DEVICE */);
int scp_lattice_costs(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                      const uint32_t* pen /* DEVICE [nodes] or NULL */, int n_src, const double* src /* DEVICE [n_src][D] */,
                      int n_dst, const double* dst /* DEVICE [n_dst][D] */, uint32_t* costs /* DEVICE [n_src][n_dst] */,
                      int32_t* src_node /* DEVICE [n_src] */, int32_t* dst_node /* DEVICE [n_dst] */,
                      uint32_t* cost_out /* DEVICE [n_src][nodes] or NULL */);

/* ---- static obstacles: shared paths ---------------------------------------------------------------------------------------------
 * A further additive part of ABI version 7: three functions; nothing above changes.  scp_reference_paths_weighted finds every
 * vehicle's path as if it were alone on the map, so all vehicles on one side of a wall take the same cheapest doorway.  These
 * calls make the nodes that OTHER vehicles' paths use cost extra, re-route the fleet in groups and keep the least crowded set
 * of paths (negotiated routing).  Lattice, node ids, edge masks, DIRECTION ORDER, move weights, statuses, the walk rule, the
 * reference points and scp_path_info are those of scp_lattice_edges / scp_reference_paths_weighted.  Integers only, except the
 * reference points (scp_reference_paths', bit for bit).  tests/shared_path_ref.py restates every rule in numpy / plain Python.
 *
 * Path set.  The path / info pair of N vehicles.  nodes_i = the first n_nodes entries of row i if status == 0, otherwise
 *   empty.  A path never visits a node twice (costs fall strictly along it).
 * Load and overuse (scp_path_load), capacity >= 1:
 *     load[u] = the number of vehicles i with u in nodes_i (uint32),  overuse = sum over u of max(0, load[u] - capacity) (uint64).
 *   Both are written, not accumulated.  The array is zeroed, then one thread per path entry adds 1 with an integer atomic
 *   (order-independent, so exact); one thread per node then takes its excess, a wave sum, and one 64-bit atomic add per
 *   workgroup.  An entry that is no node id of the lattice is not counted.
 * Shared penalty of vehicle i, share_weight in 0 .. SCP_PENALTY_MAX_PRODUCT:
 *     others_i[u] = load[u] - [u in nodes_i],
 *     pen_i[u] = min(pen[u] + share_weight * max(0, others_i[u] + 1 - capacity), SCP_PENALTY_MAX_PRODUCT),
 *   evaluated as if in unbounded integers (the kernel uses 64 bits and clamps before anything can wrap); pen = NULL means
 *   zeros.  The edge cost is w_i(u, v) = 2 W[len] + pen_i[u] + pen_i[v]: an edge still costs at most 242 + 65536, so the
 *   no-wrap argument of the weighted search holds unchanged and 0xFFFFFFFF stays "unreached".
 * Re-routing vehicle i (scp_reference_paths_shared).  The complete cost field from its goal node under w_i; the walk from the
 *   start by the weighted search's rule with w_i; path_cost[i] = cost_i[start]; path row, info and reference points as there.
 *   A vehicle whose info[i].status != 0 ON ENTRY is skipped: nothing of it is written (penalties cannot change what can be
 *   reached).  A vehicle whose new walk has not reached the goal after max_path nodes KEEPS its path row, info, ref rows and
 *   path_cost entirely and counts in *n_kept (written, not accumulated).  Every active vehicle reads the load of the set on
 *   entry and nobody updates it during the call, so the result does not depend on scheduling.  Statuses never change, so
 *   the call has no n_failed.  path is required: on entry it holds the set `load` was made from.  cost_out (for tests): the
 *   field of every active vehicle that was not skipped (a keeping one included); other rows are untouched.
 * Groups.  Vehicle i is ACTIVE in a call iff i mod groups == group; the four outputs of an inactive vehicle are not touched.
 * Negotiation (scp_negotiate_paths).  Round 0 is scp_reference_paths_weighted; overuse_out[0] is its overuse.  Round r = 1 ..
 *   rounds: the load of the current set; group (r - 1) mod groups is re-routed; overuse_out[r] is the overuse of the new set.
 *   The outputs are the set of the round with the smallest overuse, the earliest one on ties (*best_round).  *n_failed is
 *   round 0's; *n_kept is summed over the rounds.  rounds == 0 is the weighted search bit for bit; with share_weight == 0
 *   every round reproduces round 0, so *best_round == 0.  (Why groups: if every vehicle re-routes at once the fleet swings
 *   from one doorway to the other and back.  Why the best round: overuse is not monotone over the rounds even so.)
 *
 * scp_reference_paths_shared: ONE workgroup per active vehicle (i = group + b * groups) and no workgroup waits for another;
 * the kernel, the sweep, the walk and the reference points are those of scp_reference_paths_weighted (a third field type
 * whose penalty lookup is per vehicle).  On entry the workgroup marks its own path row in an LDS bitmap of nodes / 32 words
 * (at most 4 KiB beside the 32 KiB / 128 KiB field) before anything overwrites the row; pen and load are read from global
 * memory and pen_i is formed on the fly.  The walk goes to a row of the context's workspace and is copied over the path row
 * only once it has reached the goal.  The workgroup width follows "ref_path_threads".
 * scp_negotiate_paths: everything is enqueued on the ctx's stream with NO host read between the rounds.  The current set
 * lives in the context's workspace, the best one in the outputs; after every round one kernel compares overuse_out[r] with
 * the smallest earlier entry and its workgroups copy the current set over the outputs or return (a uniform branch).  Per
 * round: the shared search, the load (a clear and two kernels) and the keep kernel.
 * Supported: what scp_reference_paths_weighted supports; capacity >= 1; 0 <= share_weight <= SCP_PENALTY_MAX_PRODUCT; 1 <=
 * groups <= N; 0 <= group < groups; 0 <= rounds <= SCP_NEGOTIATE_MAX_ROUNDS; scp_path_load: N, max_path >= 1, 1 <= nodes <=
 * SCP_LATTICE_MAX_NODES.  Anything else returns SCP_ERR_INVALID with a message.  Argument checks, enqueue on the ctx's stream,
 * no host read, timing through scp_ctx_last_pair_ms, which for scp_negotiate_paths covers all its launches. */
#define SCP_NEGOTIATE_MAX_ROUNDS 64
int scp_path_load(scp_ctx* ctx, int N, int max_path, int nodes, const int32_t* path /* DEVICE [N][max_path] */,
                  const scp_path_info* info /* DEVICE [N] */, int capacity, uint32_t* load /* DEVICE [nodes] */,
                  uint64_t* overuse /* DEVICE */);
int scp_reference_paths_shared(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                               const uint32_t* edges, const uint32_t* pen /* DEVICE [nodes] or NULL */,
                               const double* p0, const double* pf /* DEVICE [N][D] */, int max_path,
                               double* ref /* DEVICE [N][K+1][D], in/out */,
                               int32_t* path /* DEVICE [N][max_path], in/out, required */,
                               scp_path_info* info /* DEVICE [N], in/out */, uint32_t* path_cost /* DEVICE [N], in/out */,
                               uint32_t* cost_out /* DEVICE [N][nodes] or NULL, for tests */,
                               const uint32_t* load /* DEVICE [nodes]: scp_path_load of path / info */, int share_weight,
                               int capacity, int groups, int group, uint64_t* n_kept /* DEVICE */);
int scp_negotiate_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                        const uint32_t* pen /* DEVICE [nodes] or NULL */, const double* p0,
                        const double* pf /* DEVICE [N][D] */, int max_path, double* ref /* DEVICE [N][K+1][D], in/out */,
                        int32_t* path /* DEVICE [N][max_path] or NULL */, scp_path_info* info /* DEVICE [N] */,
                        uint32_t* path_cost /* DEVICE [N] */, uint64_t* n_failed /* DEVICE */, int share_weight, int capacity,
                        int groups, int rounds, uint64_t* overuse_out /* DEVICE [rounds + 1] */,
                        int32_t* best_round /* DEVICE */, uint64_t* n_kept /* DEVICE */);

/* ---- static obstacles: shapes into an occupancy grid ---------------------------------------------------------------------------
 * A further additive part of ABI version 7: one struct and one function; nothing above changes.  scp_rasterize_shapes makes
 * the occupancy grid that scp_occupancy_prepare and everything after it consume, on the device, from spheres (discs in 2-D),
 * axis-aligned boxes, capsules (a segment with a radius: oblique walls, beams, pipes) and polygons (in 3-D: prisms over a
 * height range).  tests/rasterize_ref.py restates every rule below in numpy over all cells of the grid.
 *
 * Grid: that of scp_occupancy_prepare.  In coordinate d the closed cell c is [lo_d, hi_d], lo_d = origin_d + cell * (double)c_d,
 * hi_d = origin_d + cell * ((double)c_d + 1.0): one product and one sum each.  Every product, quotient, sum and difference
 * below is rounded on its own (no contraction).  margin >= 0 is the body radius of a vehicle.  A cell is OCCUPIED (occ = 1)
 * if the predicate of at least one shape holds for it, otherwise occ = 0: shapes combine by OR, so the grid depends neither on
 * their order nor on how the work is split.  "sq(g)" below is ((0 + g_x g_x) + g_y g_y) (+ g_z g_z), summed in that order.
 *
 * SPHERE (kind 0): centre c = p[0 .. D), radius r = p[6] >= 0.  g_d = max(max(lo_d - c_d, c_d - hi_d), 0), g2 = sq(g),
 *   reach = r + margin.  Occupied if g2 < reach * reach.
 * BOX (kind 1): bmin = p[0 .. D), bmax = p[3 .. 3 + D), bmin_d <= bmax_d.  g_d = max(max(lo_d - bmax_d, bmin_d - hi_d), 0),
 *   g2 = sq(g).  Occupied if g2 < margin * margin or g2 == 0.
 *   (These two are the rules of the host rasteriser scenarios.obstacles.rasterize and give its bits.)
 * CAPSULE (kind 2): the segment a -> b, a = p[0 .. D), b = p[3 .. 3 + D), radius r = p[6] >= 0.  With e = b - a,
 *   x_d(t) = a_d + t * e_d and f(t) = sq(g(t)), g_d(t) = max(max(lo_d - x_d(t), x_d(t) - hi_d), 0), g2 is the minimum of f
 *   over a finite SET of t (v replaces the minimum so far if v < it; the minimum starts at +infinity):
 *     - 0 and 1;
 *     - every breakpoint (lo_d - a_d) / e_d and (hi_d - a_d) / e_d, d < D with e_d != 0, that lies strictly inside (0, 1);
 *     - for every pair t0 < t1 of consecutive members of the sorted set so far, the stationary point of the quadratic that
 *       f is on [t0, t1], clamped: with tm = 0.5 * (t0 + t1), coordinate d is ACTIVE if x_d(tm) < lo_d (then c_d = a_d - lo_d)
 *       or x_d(tm) > hi_d (then c_d = a_d - hi_d); num = sum of c_d * e_d and den = sum of e_d * e_d over the active
 *       coordinates in the order x, y, z, from 0; t* = -num / den, replaced by t0 if t* < t0 and then by t1 if t* > t1.  If
 *       den == 0, f is constant on the interval and the pair adds tm itself: a segment that passes through the cell has
 *       f(tm) = 0 exactly between its entry and its exit, where the two breakpoints may carry a rounding error of an ulp
 *       squared -- without this member the touch rule g2 == 0 would miss cells a thin segment runs through.
 *   A minimum over a set needs no order among its members: only the set is normative, not how it is sorted.  f is convex
 *   and piecewise quadratic with exactly these breakpoints, so in exact arithmetic g2 is the squared distance between the
 *   segment and the closed cell.  reach = r + margin.  Occupied if g2 < reach * reach or g2 == 0.  a == b gives the set
 *   {0, 1} and the SPHERE's g2 bit for bit.
 * POLYGON (kind 3; a PRISM in 3-D): the vertices v_0 .. v_{n-1} = vertices[first_vertex .. first_vertex + n_vertices) in the
 *   xy plane, 3 <= n <= SCP_RASTER_MAX_POLYGON, with the closing edge v_{n-1} -> v_0; in 3-D the height range z0 = p[0] <=
 *   z1 = p[1].  Even-odd rule: the winding direction does not matter, non-convex polygons are allowed.  gz = max(max(lo_z -
 *   z1, z0 - hi_z), 0) in 3-D, 0 in 2-D.  Occupied if (i) or (ii):
 *     (i)  some edge v_i -> v_{i+1} has g2 = g2xy + gz * gz with g2 < margin * margin or g2 == 0, g2xy being the CAPSULE's g2
 *          of that edge in the two coordinates x, y;
 *     (ii) the cell's centre is inside the polygon and gz * gz < margin * margin or gz == 0.  Centre: cx = origin_x + cell *
 *          ((double)c_x + 0.5), cy likewise.  An edge p -> q is CROSSED if (p_y <= cy) != (q_y <= cy) and cx < p_x + ((cy -
 *          p_y) * (q_x - p_x)) / (q_y - p_y); the centre is inside if the integer count of crossed edges is odd.
 *   Why this is the distance rule of the solid: cell and prism are both products of a planar set and an interval, so dist^2 =
 *   dist_xy^2 + dist_z^2; the planar distance is 0 if an edge touches the cell's rectangle or the rectangle lies inside the
 *   polygon -- a rectangle no edge touches lies wholly inside or wholly outside, so its centre decides -- and otherwise it
 *   is the minimum over the edges.
 *
 * Invalid (SCP_ERR_INVALID with a message, nothing enqueued): a kind other than the four, a parameter the kind reads that is
 * not finite, r < 0, bmax_d < bmin_d, z1 < z0 (3-D), n_vertices outside 3 .. SCP_RASTER_MAX_POLYGON, a vertex range outside
 * [0, n_vertices of the call), n_shapes outside 0 .. SCP_RASTER_MAX_SHAPES, n_vertices of the call outside 0 ..
 * SCP_RASTER_MAX_VERTICES, a margin that is negative or not finite, a grid scp_occupancy_prepare rejects.  Fields a kind
 * does not read (and `reserved`) are ignored.
 *
 * How it runs.  The host side computes per shape a conservative inclusive CELL RANGE -- per coordinate floor((min_d - reach -
 * origin_d) / cell) - 2 .. floor((max_d + reach - origin_d) / cell) + 2 from the shape's extremes (reach = margin for BOX and
 * POLYGON), clipped to the grid -- and cuts every range into WORK ITEMS of at most "raster_item_cells" cells (scp_ctx_set_option;
 * default 1024; doubled for a call until there are at most 2^18 items), rows along x first.  The range only prunes: the
 * predicate decides, and a shape whose range is empty costs nothing.  Shapes, vertices and items travel in one copy; occ is
 * cleared; then ONE launch, a workgroup per item (the shape is uniform across it: scalar registers), a thread per cell, x
 * fastest, stores 1 where the predicate holds (byte stores of the same value: no atomics).  A polygon's vertices are staged in
 * LDS in blocks; every lane reads the same edge.  No workgroup waits for another, every loop is bounded by a count.  The
 * work of a shape is proportional to its own range, and one large shape spreads over the whole GPU.  n_shapes = 0 gives an
 * all-free grid.  Enqueued on the ctx's stream, no host read (the host arrays are copied before the call returns), timing
 * through scp_ctx_last_pair_ms. */
#define SCP_SHAPE_SPHERE 0
#define SCP_SHAPE_BOX 1
#define SCP_SHAPE_CAPSULE 2
#define SCP_SHAPE_POLYGON 3
#define SCP_RASTER_MAX_SHAPES 65536
#define SCP_RASTER_MAX_VERTICES 1048576
#define SCP_RASTER_MAX_POLYGON 4096
typedef struct scp_obstacle_shape { /* [host], 72 bytes */
  int32_t kind;         /* SCP_SHAPE_* */
  int32_t first_vertex; /* POLYGON: its first vertex in `vertices` */
  int32_t n_vertices;   /* POLYGON: 3 .. SCP_RASTER_MAX_POLYGON */
  int32_t reserved;
  double p[7];          /* SPHERE c, -, r; BOX bmin, bmax, -; CAPSULE a, b, r (three slots per point, D used); POLYGON z0, z1 */
} scp_obstacle_shape;
int scp_rasterize_shapes(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int n_shapes,
                         const scp_obstacle_shape* shapes /* [host] [n_shapes] */, int n_vertices,
                         const double* vertices /* [host] [n_vertices][2] */, double margin,
                         uint8_t* occ /* DEVICE out [nz][ny][nx], 0 / 1 */);

/* ---- test hooks (dense K-dimension products used by the QP; exercised by tests/test_kernels_gpu.py::test_gemm_f64) ------
 * Y[R][C] = alpha * A[R][M] X[M][C] + beta * Y, row-major, device pointers. */
int scp_gemm_f64(scp_ctx* ctx, int use_mfma, int R, int M, int C, double alpha, const double* A,
                 const double* X, double beta, double* Y);
/* Copy one internal array of the solver (time-major device layout) to `out` (device, capacity `cap` doubles);
 * *n_out [host] = its length.  name: "x" [K][C], "zf" / "yf" / "fx" [4K-1][C] (fx = carried F x), "lf" / "uf" [4K-1][C] (the
 * bounds of the fixed rows; tests/test_corridor_gpu.py), "qx" [K][C] (carried S0 x),
 * "zc" / "yc" per working row, "gval" per incidence-list entry; "Hf" / "Minv" / "T" [K][K] row-major: the blocks of the
 * current rho (H_f, its inverse, T = S0 H_f^-1; tests/test_pipeline_iterates_gpu.py).  tests/test_qp_gpu.py compares the
 * state the persistent and the three-launch pipelines leave behind. */
int scp_qp_peek(scp_qp* qp, const char* name, double* out, int64_t cap, int64_t* n_out);
/* "persist_fault" = n: the next n persistent launches wait for a workgroup that does not exist, so their bounded spins time
 * out (the give-up path: nothing written back, the solve continues on the three-launch pipeline); "persist_off": read
 * (value < 0) or set whether the solver has fallen back; "persist_host_lists" = 1: the host builds the incidence lists and
 * the row values before every persistent launch and the kernel loads its slice, instead of building its own entry tables
 * (tests/test_persist_lists_gpu.py; the QP objects inside scp_solver take the starting value from SCP_PERSIST_HOST_LISTS
 * in the environment); "reset_form": 1 (default) = scp_qp_reset's one-launch form runs as the tiled kernel that fills the
 * chip wherever its LDS tile fits, 0 = as the 16-column kernel (same bits; tests/test_reset_forms_gpu.py).  Returns the
 * value in effect. */
int scp_qp_debug_set(scp_qp* qp, const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* SCP_HIP_H */
