// Internal declarations shared by the translation units of libscp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "scp_hip.h"

// mapped host copy of the stats of the latest pass that produced a row list (written by its last kernel, seq last)
struct scp_stats_mirror {
  scp_pair_stats stats;
  unsigned long long n_spec;  // small-problem violations pass from a solution: rows of its speculative selection
  double pts[6];   // small-problem select pass from a QP solution: the two positions of the first violating pair
  double rel[64];  // small-problem violations pass: the partial sums of scp_rel_step(x_new, x_prev), block by block
  volatile unsigned long long seq;
};

constexpr int SCP_SMALL_MAX_WG = 2048;  // workgroups of a small-problem pairwise pass (the whole pass in one launch)

struct scp_ctx {
  int device;
  int n_cu;  // compute units of the device (resident-workgroup limit of the persistent kernels)
  hipStream_t stream;
  char err[512];
  // small device scratch for reductions / host read-back
  double* d_scratch;      // 72 doubles
  double* h_scratch;      // pinned, 72 doubles
  double* h_scratch_dev;  // its device address (kernels that hand a few numbers to the host write there directly)
  hipEvent_t ev0, ev1;
  hipEvent_t pair_ev0, pair_ev1;  // bracket the most recent pairwise kernel (scp_ctx_last_pair_ms)
  bool pair_timed;
  bool pair_ran;
  bool last_pass_small;  // the latest pairwise pass ran as ONE launch and published its stats in the host mirror (also a check pass)
  double* tm_scratch;     // time-major copy of a trajectory array for the pairwise passes (grown on demand)
  size_t tm_bytes;
  uint32_t* cmp_map;      // scratch bitmap of the violations pass (self-cleaning), grown on demand
  size_t cmp_map_bytes;
  uint32_t* cmp_tot;      // per-block totals / offsets of the bitmap compaction
  size_t cmp_tot_bytes;
  scp_stats_mirror* h_mirror;  // mapped host memory and its device address
  scp_stats_mirror* d_mirror;
  unsigned long long mirror_seq;  // sequence number of the latest compaction launch
  unsigned long long* wg_part;    // [SCP_SMALL_MAX_WG][4] per-workgroup partials of a small-problem pairwise pass
  uint32_t* wg_rows;              // [workgroups][8192] per-workgroup sub-lists of its marked rows (grown on demand)
  size_t wg_rows_bytes;
  unsigned* d_ticket;             // its last-workgroup-done counter (zero between launches): word 0 of a 64-byte block of
                                  // device words that lives as long as the ctx ([1], [2]: the QP's tickets; [3]: the
                                  // violations pass's "not finite" word; [4, 8): the two words of scp_schedule_starts_batch; [8, 10): `lag_solved`; [10, 12): `delay_solved`;
                                  // [12, 16): `solved`)
  int timing;                     // HIP events around the pairwise kernels and the QP solves (scp_ctx_set_option; default on)
  int small_pass;                 // one-launch pairwise passes for small problems (scp_ctx_set_option; default on)
  int fused_step_prep;            // large problems: the prep launch of a pass derives the positions it stages from the
                                  // accelerations / the QP's solution itself (scp_ctx_set_option; default on)
  unsigned long long rel_seq;     // of the latest scp_rel_step (completion word: h_scratch[64]; partials: h_scratch[0..64))
  void* gen_ws;                   // device workspace of scp_generate_grid_swap (grown on demand)
  size_t gen_ws_bytes;
  void* sep_ws;                   // device workspace of the continuous-time passes: scp_check_separation, scp_list_conflicts,
  size_t sep_ws_bytes;            // scp_clearance_profile, scp_delay_margins, scp_lag_conflicts (time-major records + each call's own arrays; grown on demand)
  unsigned long long* solved;     // [2] segments of the latest check / of the latest profile that reached the quartic (in
                                  // the d_ticket block: a workspace that grows frees its old place, these words stay)
  bool solved_ran[2];             // that call has run on this ctx
  unsigned long long* delay_solved;  // the same figure of the latest scp_delay_margins (in the d_ticket block too)
  bool delay_solved_ran;
  int delay_lag_chunk, delay_time_chunk;  // lags / global segments per workgroup of scp_delay_margins; 0: chosen by the call
                                  // (scp_ctx_set_option; developer switches, results never depend on them)
  unsigned long long* lag_solved;  // the same figure of the latest scp_lag_conflicts (in the d_ticket block too)
  bool lag_solved_ran;
  int lagc_lag_chunk, lagc_time_chunk;  // the same two switches of scp_lag_conflicts
  int stg_batch_threads;          // threads per workgroup of scp_schedule_starts_batch: 0 chosen by the call, 256 or 1024
  int stg_batch_transposed;       // it reads the masks' columns from a transposed copy it makes in sep_ws: -1 chosen by the
                                  // call (from 16 candidates on), 0 never, 1 always
  int ref_path_threads;           // threads per workgroup of scp_reference_paths, scp_reference_paths_weighted, scp_reference_paths_shared, scp_lattice_distances and scp_lattice_costs: 0 chosen by the call, 64, 256, 512 or 1024
  int shorten_threads;            // threads per workgroup of scp_shorten_paths: 0 chosen by the call, 64, 128 or 256
  int raster_item_cells;          // cells per work item of scp_rasterize_shapes: 0 chosen by the call (1024), or 64 .. 2^24
  void* rast_ws;                  // its device copy of shapes, vertices and work items (grown on demand) ...
  size_t rast_ws_bytes;
  void* rast_host;                // ... and the pinned host buffer the copy starts from (grown on demand);
  size_t rast_host_bytes;
  hipEvent_t rast_copied;         // recorded behind the copy: the next call waits for it before it refills the buffer
  int* h_gen_flag;                // mapped host word "a block was flagged in this sweep" and its device address
  int* d_gen_flag;
  void* asg_ws;                   // device workspace of scp_straight_line_check (per-workgroup partials; grown on demand)
  size_t asg_ws_bytes;
  void* asgw_ws;                  // device workspace of scp_assign_goals_wide (per-scenario auction state + control blocks;
  size_t asgw_ws_bytes;           // grown on demand)
  int asgw_min_bidders;           // its rounds with at least this many bidders run on the whole chip; 0: chosen by the call
  int asgw_prices_in_lds;         // its narrow runs keep the prices in LDS: -1 auto, 0 never, 1 where they fit
  int asgw_control_threads;       // threads of its control workgroup: 0 chosen by the call (256 up to N = 512, else 1024)
                                  // (scp_ctx_set_option; developer switches, results never depend on them)
  int near_pass;                  // near form of the recomputing violations pass: 0 off, 1 auto, 2 force (scp_ctx_set_near_pass)
  unsigned near_call_no;          // number of the latest recomputing violations pass (what its prep kernel leaves in
                                  // d_ticket[3] when a staged value is not finite)
  unsigned long long near_ran, near_fell_back;  // near passes of this ctx / those followed by the exhaustive pass
};

static inline int scp_fail(scp_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define SCP_HIP_CHECK(ctx, call)                                                                     \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return scp_fail((ctx), SCP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),    \
                      __FILE__, __LINE__);                                                           \
  } while (0)

#define SCP_REQUIRE(ctx, cond, ...)                                   \
  do {                                                                \
    if (!(cond)) return scp_fail((ctx), SCP_ERR_INVALID, __VA_ARGS__); \
  } while (0)

static inline int64_t scp_pairs(int N) { return (int64_t)N * (N - 1) / 2; }
static inline int scp_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// At least `need` bytes behind one of the ctx's grown-on-demand buffers (tm_scratch, cmp_map, ...): `buf` and `have` are
// the addresses of its pointer and size fields.  Drains the ctx stream before it frees the old buffer.  (scp_ctx.hip)
int scp_ctx_ensure_bytes(scp_ctx* ctx, void** buf, size_t* have, size_t need);

// Raise a kernel's dynamic-LDS limit to at least `bytes` (gfx950: up to 160 KiB per workgroup).  The attribute belongs to
// the (device, kernel) pair and is only ever raised, so concurrent solves of different sizes cannot lower each other's
// limit.  Thread safe.
hipError_t scp_raise_lds_limit(int device, const void* kernel, size_t bytes);

// Wait until a mapped host word takes the value `seq` (written by the last kernel of a check / by the persistent kernel).
// mode 0 (default): spin -- lowest latency, one host core per waiting thread; mode 1 (scp_set_host_wait): spin for
// ~20 us, then poll every ~20 us from a sleep, for many solver threads on few cores (compute-trajectories-batch).
// Returns false after `timeout_s` seconds.
bool scp_wait_host_word(volatile unsigned long long* word, unsigned long long seq, int timeout_s);

// ---- the near form of the recomputing violations pass (scp_near.hip; chosen and followed up in scp_kernels.hip: pair_pass) ----
// Rows whose bound  R - dist + |dP_i| + |dP_j|  lies below -SCP_NEAR_TAU are not examined.  The bound is a sum of four
// numbers of the arena's size (<= 1e2): its fp64 rounding, the inflation of |dP| and the squared comparison included, stays
// below 1e-12.  1e-6 is six orders above that and still six below the distances that decide anything (R ~ 1, feas_tol
// 1e-6 .. 1e-4): at 1024 x 50 the examined rows are 6 445 of 26 188 800.  The caller trusts a near pass whose maximum is at
// least -SCP_NEAR_TAU / 2: every unexamined row is then smaller than the maximum and, being negative, not violated.
constexpr double SCP_NEAR_TAU = 1e-6;
constexpr double SCP_NEAR_MAX_ABS = 1e100;  // staged values beyond this count as not finite (their squares must not overflow)
struct ScpNearArgs {
  int N, K, D;
  double R, feas_tol;
  int64_t q_begin, q_end;
  const double* P_tm;      // [K][N][D] linearisation point, time-major
  const double* dP_tm;     // [K][N][D] P_new - P_prev
  const uint32_t* bitmap;  // working-set membership
  uint32_t* mark;          // scratch map the violated rows outside the working set are marked in
  scp_pair_stats* stats;   // max_violation (initialised by the prep kernel)
  const unsigned* unbounded;  // == call_no: a staged value of this call was not finite, nothing is examined
  unsigned call_no;
};
inline unsigned* scp_near_unbounded_word(scp_ctx* ctx) { return ctx->d_ticket + 3; }
// the tables of one time step fit the LDS of a workgroup; *lds_bytes: their size
bool scp_near_fits(int N, int D, size_t* lds_bytes);
// the near kernel, between the two events scp_ctx_last_pair_ms reads
int scp_launch_near_violations(scp_ctx* ctx, const ScpNearArgs& a, size_t lds_bytes);

// shape / pair-range validation shared by every pairwise pass (scp_kernels.hip)
int scp_check_pair_range(scp_ctx* ctx, int N, int K, int D, int64_t q_begin, int64_t q_end);

// Stats of the latest scp_linearize_pairs / scp_collision_violations[_at] call of this ctx, from the host mirror: waits for
// that pass's last kernel only (no stream drain, no copy launch).  (scp_ctx.hip)
int scp_ctx_wait_stats(scp_ctx* ctx, scp_pair_stats* out);

// scp_qp_get_solution + scp_kinematics + scp_collision_violations_at of a small problem in one launch (scp_kernels.hip)
int scp_violations_from_solution(scp_ctx* ctx, int N, int K, int D, double R, double h, int64_t q_begin, int64_t q_end,
                                 const double* pos_prev, const double* x_tm, const double* p0, const double* v0, double* x_out,
                                 double* pos_out, double feas_tol, int64_t* new_rows, int64_t new_cap, uint32_t* sel_bitmap,
                                 scp_pair_stats* stats, const double* rel_prev /* [N][K][D] or NULL */,
                                 int64_t* spec_rows /* or NULL: + the selection around the new positions */, int64_t spec_cap,
                                 uint32_t* spec_bitmap, double spec_margin, int* form);
// ... *form: nothing was launched | the one-launch pass of a small problem (stats, relative-step sums and the speculative
// selection in the mirror) | the multi-launch pass with a prep launch that derived x_out / pos_out ("fused_step_prep")
enum { SCP_FROM_SOLUTION_NONE = 0, SCP_FROM_SOLUTION_SMALL = 1, SCP_FROM_SOLUTION_LARGE = 2 };
// scp_kinematics(acc) -> pos_out + scp_linearize_pairs (eta_out != NULL) / scp_select_pairs at pos_out with one prep launch
// for both, where the pass runs as several launches ("fused_step_prep"; scp_kernels.hip)
int scp_pairs_from_acc(scp_ctx* ctx, int N, int K, int D, double R, double h, int64_t q_begin, int64_t q_end, const double* acc,
                       const double* p0, const double* v0, double* pos_out, double* eta_out, double* l_out, double margin,
                       int64_t* sel_rows, int64_t sel_cap, uint32_t* sel_bitmap, scp_pair_stats* stats, bool* fused);
// scp_rel_step's numbers from the sums that pass left in the mirror (after its stats have arrived)  (scp_ctx.hip)
void scp_ctx_mirror_rel(scp_ctx* ctx, int64_t n, double* out);
// scp_qp_get_solution + scp_kinematics + scp_check_avoidance + scp_select_pairs of a small problem in one launch
int scp_select_from_solution(scp_ctx* ctx, int N, int K, int D, double R, double h, int64_t q_begin, int64_t q_end,
                             const double* x_tm, const double* p0, const double* v0, double* x_out, double* pos_out,
                             double margin, int64_t* sel_rows, int64_t sel_cap, uint32_t* sel_bitmap, scp_pair_stats* stats,
                             bool* fused);
// scp_kinematics + a copy of `acc` to acc_copy in the same launch (scp_traj.hip)
int scp_launch_kinematics_copy(scp_ctx* ctx, int N, int K, int D, double h, const double* acc, const double* p0,
                               const double* v0, double* pos_out, double* vel_out, double* acc_copy);
// scp_rel_step(a_new, a_prev) + a copy of a_new to copy_out (NULL: none) in the same launch (scp_traj.hip); copy_out must not
// overlap a_prev
int scp_launch_rel_step_copy(scp_ctx* ctx, int64_t n, const double* a_new, const double* a_prev, double* out, double* copy_out);
// the QP's current iterate in its own layout ([K][N D], device pointer)
const double* scp_qp_solution_tm(const scp_qp* qp);

// scp_qp_reset(x0) + scp_qp_add_rows_at(rows): one launch when the problem is small, the two calls otherwise (same bits)
int scp_qp_reset_add_rows_at(scp_qp* qp, const double* x0, int64_t n, const int64_t* rows, const double* pos_prev,
                             const double* p0, const double* v0, double R);
// scp_gather_rows + scp_qp_add_rows in one launch: eta / l_col are the outputs of scp_linearize_pairs over [q_begin, q_end)
int scp_qp_add_rows_from_pass(scp_qp* qp, int64_t n, const int64_t* rows, const double* eta, const double* l_col,
                              int64_t q_begin, int64_t q_end);

// working rows [base, base + n) of a QP with eta / l recomputed from the linearisation point (scp_qp_add_rows_at)
int scp_launch_add_rows_at(scp_ctx* ctx, int N, int K, int D, int64_t base, int64_t n, const int64_t* rows,
                           const double* pos_prev, const double* p0, const double* v0, double R, double h, const double* Qx,
                           int64_t* w_row, int* wk, int* wi, int* wj, double* weta, double* wl, double* zc, double* yc);

// the launch of scp_qp_set_position_boxes: rows [3K-1, 4K-2) of lf / uf from the boxes lo / hi [N][K][D] by state; space6 =
// {min_0 .. min_2, max_0 .. max_2} and states = [p0 | v0 | pf | vf] as scp_qp keeps them (scp_corridor.hip)
int scp_launch_position_boxes(scp_ctx* ctx, int N, int K, int D, double h, const double* space6, const double* states,
                              const double* lo, const double* hi, double* lf, double* uf);

// ---- internal launchers (time-major device layout [K][C], C = N*D) --------------------------------
// Y[R][C] = alpha * A[R][M] X[M][C] + beta * Y   (row-major; A small and L2 resident)  (scp_gemm.hip)
int scp_launch_gemm(scp_ctx* ctx, int use_mfma, int R, int M, int C, double alpha, const double* A,
                    const double* X, double beta, double* Y);
// [N][K][D] <-> [K][N*D]  (scp_traj.hip)
int scp_launch_to_time_major(scp_ctx* ctx, int N, int K, int D, const double* src, double* dst);
int scp_launch_from_time_major(scp_ctx* ctx, int N, int K, int D, const double* src, double* dst);
// fixed-row bounds in time-major stacked layout: rows [0,K-1) jerk, [K-1,2K-1) acc, [2K-1,3K-1) vel,
// [3K-1,4K-1) pos, each row C = N*D wide.  (scp_traj.hip)
int scp_launch_bounds_time_major(scp_ctx* ctx, int N, int K, int D, double h, const double* limits_host,
                                 const double* space_host, const double* p0, const double* v0,
                                 const double* pf, const double* vf, double* l_tm, double* u_tm,
                                 double* states_out /* [4][N][D] = p0, v0, pf, vf, or NULL */);
