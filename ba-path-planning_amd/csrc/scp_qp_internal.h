// Declarations shared by the translation units of the joint QP, one block per owning file:
//   scp_qp.hip          the solver object, the C-ABI, reset / add rows, the choice of the pipeline and the solve loop
//   scp_qp_kkt.hip      the blocks rebuilt per rho and their cache
//   scp_qp_generic.hip  the generic pipeline (one product per launch)
//   scp_qp_rows.hip     the working rows and their incidence lists
//   scp_qp_columns.hip  the column-block kernels: single-step pipeline, QP#0, fused termination check
//   scp_qp_persist.hip, scp_qp_persist16.hip  the persistent kernels
// then the one launch helper of these files and, at the end, the QpDerived transitions.
#pragma once
#include "scp_common.h"

#define QP_CHECK(call)            \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != SCP_OK) return rc_; \
  } while (0)

// ---- scp_qp_kkt.hip: the rho-dependent blocks and their cache -----------------------------------------------------------------
constexpr int SCP_KKT_SLOTS = 6;       // cached rho values per solver object: at least this many ...
constexpr int SCP_KKT_SLOTS_MAX = 32;  // ... and up to this many while the pool stays below SCP_KKT_POOL_BYTES
constexpr size_t SCP_KKT_POOL_BYTES = (size_t)48 << 20;
constexpr int SCP_INV_LDS_MAX_K = 96;  // [H_f | I] (K x 2K doubles) resident in LDS for the Gauss-Jordan inverse
static inline size_t scp_packed_count(int R, int M) { return (size_t)((R + 15) / 16) * ((M + 3) / 4) * 64; }
size_t scp_qp_kkt_pool_doubles(int K);    // doubles behind QpDev::kkt_pool: every slot of this K
void scp_qp_kkt_init_slots(scp_qp* qp);  // points the slots into the pool, all empty (scp_qp_create)
int scp_qp_build_g0(scp_qp* qp);          // G0 = F^T w F, once per object (scp_qp_create)
// d.Hf / HS / Minv / T / pMinv / pT of the current (rho, sigma): the cached slot, or built into the least recently used one
int scp_qp_build_kkt(scp_qp* qp);

// ---- scp_qp.hip: the solver object ---------------------------------------------------------------------------------------
enum Slot {  // device scalar slots (doubles)
  SL_RZ0 = 0, SL_RZ1 = 1,
  SL_RP = 8, SL_NAX = 9, SL_NZ = 10, SL_RD = 11, SL_NPX = 12, SL_NATY = 13,
  SL_NDY = 14, SL_SUPP = 15, SL_NATDY = 16,
  SL_COUNT = 32
};

struct QpDev {
  // constant blocks
  double *F, *Ft, *S0, *S0t, *HS, *Hf, *Minv, *aug, *wrow;
  double* gj_tmp;  // [3K]: pivot row and column of the per-pivot Gauss-Jordan launches (K > SCP_INV_LDS_MAX_K)
  double* G0;  // [K][K]: F^T w F (constant; H_f = (2 + sigma) I + rho G0)
  // H_f^{-1} in MFMA A-operand order for the column kernels (packed by scp_qp_kkt.hip):
  // [row tile][k step][lane] = A[16 tile + (lane & 15)][4 step + (lane >> 4)], zero beyond the matrix, so that one
  // wave-wide operand load is 512 contiguous bytes
  double* pMinv;
  double *T, *pT;  // T = S0 H_f^{-1} (K x K, rebuilt with H_f^{-1}) and its packed form: S0 p = T r without waiting for p
  // fixed rows
  double *lf, *uf, *zf, *yf, *wf, *tf;
  double* states;  // [4][N][D]: p0, v0, pf, vf of the latest scp_qp_set_problem (the lean persistent kernel re-derives the bounds)
  // x-space vectors [K][C]
  double *x, *xt, *rhs, *r, *p, *zz, *G;
  double* HQ;  // [2K][C]: rows [0,K) = H v, rows [K,2K) = S0 v
  // working rows
  int64_t* w_row;
  int *w_k, *w_i, *w_j;
  double *w_eta, *w_l, *zc, *yc;
  // scalars
  double* scal;   // SL_COUNT, followed by SCP_RESID_CAP partial results of a termination check
  double* part;   // 2 * SCP_PART_CAP
  double* s0p;    // [K][C]: S0 p of the single-step pipeline (scp_qp_peek "qp")
  double* fx;     // [Rf][C]: F x carried by the single-step pipeline (F p goes to tf)
  double* dyf;    // [Rf][C]: snapshot of y_f, then delta-y (primal infeasibility certificate)
  double* dyc;    // [cap]  : same for the working rows
  // deterministic row -> column transfer (single-step pipeline): incidence lists per (time step, agent) cell
  int* cell_ptr;  // [N*K + 1] exclusive offsets into the entry arrays
  int* cell_cur;  // [N*K]     fill cursors (build time)
  int* scan_tot;  // [N*K / 4096 + 2] per-workgroup totals of the offset scan
  int* ent_code;  // [2 cap]   2 n + side, sorted inside every cell (side 0: agent i, +eta; side 1: agent j, -eta)
  double* coef;   // [2 cap][D] signed eta of the entry
  double* gval;   // [2 cap]   per-entry row value, written by the row kernels (no atomics)
  double* gval2;  // [2 cap]   row vectors of a termination check: yc ...
  double* gval3;  // [2 cap]   ... and delta-yc (gval keeps the pipeline's values across a check)
  int *pos_i, *pos_j;  // [cap] entry positions of row n
  double* grow;        // [cap] row values per ROW: what a persistent kernel that built its own entry tables leaves at its exit
  int* own_code;       // [SCP_PERSIST_MAX_WG + 1][SCP_PERSIST_CAP_MAX] the sorted entry codes of each of its workgroups
  double* kkt_pool;  // scp_kkt_slots(K) cache slots of the rho-dependent blocks
  unsigned long long* sync_words;  // SCP_SYNC_WORDS: give-up word of the persistent kernel, scratch
  unsigned long long* cells;       // [K][N][D][2] tagged granules: S0 p cells published by the persistent kernel
  unsigned long long* gpart;       // SCP_GPART_WORDS tagged granules: line-search partials, two alternating buffers
  unsigned long long* gcheck;      // SCP_GCHECK_WORDS tagged granules: termination-check partials
};

// Which derived device state still matches the primary state (x, z / y, the working rows, rho).  Only the qp_on_*
// transitions at the end of this header write it.
struct QpDerived {
  bool lists = false;       // the incidence lists (cell_ptr, ent_code, coef, pos_i / pos_j) match the working set
  bool qx = false;          // the S0 x half of HQ and the F x slab are exact for x
  int qx_half = 0;          // which half of HQ holds S0 x: 0 -> rows [K, 2K), 1 -> [0, K) (swapped by every single step)
  double vals_rho_c = 0.0;  // > 0: the small install built lists and row values with the latest rows, at this column rho
  bool carried = false;     // the single-step pipeline's carried state (S0 x, F x, row values) matches (x, zc, yc, rho)
  // (with carried) where the row values are: false -> gval, per entry of the incidence lists; true -> grow, per row, left by a
  // persistent kernel that built its own entry tables (gval is stale then, and so are the lists unless `lists` says otherwise)
  bool vals_by_row = false;
};

struct scp_qp {
  scp_ctx* ctx;
  int N, K, D, Rf;
  int64_t C;
  double h;
  scp_qp_settings st;
  int64_t row_cap, nW;
  bool problem_set, reset_done;
  bool has_boxes;  // scp_qp_set_position_boxes has rewritten position rows of lf / uf since the latest scp_qp_set_problem: the
                   // lean persistent kernels, which re-derive the bounds from space / states, do not run this QP
  QpDerived dv;
  double rho;
  QpDev d;
  // rho-dependent blocks (H_f, [H_f; S0], H_f^{-1}, T and the packed H_f^{-1}, T) are cached per rho: adaptive rho is
  // snapped to a geometric grid and every solve starts from settings.rho, so the same few values recur from QP to QP and
  // the 48 us single-workgroup inverse is paid once per value.  d.Hf / HS / Minv / T / pMinv / pT point into the active slot.
  struct KktSlot {
    double rho, sigma;
    unsigned long long used;  // LRU stamp, 0 = empty
    double *Hf, *HS, *Minv, *T, *pMinv, *pT;
  } kkt[SCP_KKT_SLOTS_MAX];
  int n_kkt;  // slots in use for this K (scp_kkt_slots)
  unsigned long long kkt_clock;
  double* h_scal;  // pinned, SL_COUNT + SCP_RESID_CAP doubles + the completion flag of a fused check
  double* h_scal_dev;  // the same memory as the device sees it: the check kernels write their partials straight to it
  unsigned long long check_seq;  // value the flag takes when the current check has finished
  // persistent single-step kernel (scp_qp_persist.hip)
  double space[6];                   // {min_0.., max_0..} of the latest scp_qp_set_problem
  double lim[6];                     // {vel, acc, jerk} x {min, max} of the latest scp_qp_set_problem (the lean persistent kernel
                                     // takes the jerk / acceleration bounds as scalars)
  int64_t steps_since_reset;         // ADMM steps since scp_qp_reset: the lean persistent kernels keep one double per fixed row
                                     // (v = z~ + y / rho), which presumes z = Pi(v) -- true after any ADMM update, not for the
                                     // unprojected z = A x0 of a reset: their first step of a QP takes z = v (y = 0 then)
  int persist_variant;               // of the latest persistent launch: 0 = 8 (4 in 3-D) agents per workgroup, 1 = lean, 16
  int persist_fault;                 // test hook: the next n persistent launches wait for a workgroup that does not exist
  bool persist_host_lists;           // test hook: the host builds lists and row values for every persistent launch
  int reset_form;                    // scp_qp_reset's one-launch kernel: 1 = tiled over the whole chip (default), 0 = 16-column
  bool persist_off;                  // a launch gave up (workgroups not co-resident): three-launch pipeline until the next
                                     // scp_qp_reset / scp_qp_set_problem re-arms the persistent path
  bool persist_skip_solve;           // the CUs for a persistent launch were not free: this scp_qp_solve call stays on the
                                     // three-launch pipeline (cleared at the start of every call)
  int persist_gave_up_total;         // give-ups over the life of the object (scp_qp_debug_set "persist_gave_up_total")
  int64_t persist_cap_nW;            // working-set size that overflowed the LDS entry tables (-1: none): not tried again
  int persist_cap;                   // LDS entry capacity per workgroup (all the LDS that is left)
  unsigned long long persist_epoch;  // ADMM steps run by persistent launches so far: the step tags of the granules never repeat
  unsigned* h_persist;               // mapped host words written by the kernel: [0] exit code, [1] iterations done, [2] rho switches
  int persist_rho_switches;          // of the latest persistent launch: adaptive-rho updates the kernel made by itself ...
  double persist_rho;                // ... and the rho it ended with
  unsigned* h_persist_dev;
};

// Steps between two termination checks once the residuals are close to the tolerances (settings.check_fine), or 0: the
// cadence stays fixed.  The fine cadence applies when it divides the coarse one, to QPs with collision rows (QP#0 keeps the
// fixed cadence: its 20 surplus steps are cheap, and a better converged starting point saves the first joint QP of large
// problems far more: 250 instead of 400 steps at 1024 x 50), and up to SCP_FINE_MAX_COLUMNS columns: beyond, it measured
// slower (4096 x 50: 195 instead of 200 steps, but 0.27 ms more in every repetition; profiles/r03_check_cadence.txt,
// r03_check_cost.txt).  The host loop of scp_qp_solve and the persistent kernels both follow this rule.
constexpr int64_t SCP_FINE_MAX_COLUMNS = 4096;
inline int scp_qp_fine_cadence(const scp_qp* qp) {
  const scp_qp_settings& st = qp->st;
  const bool fine = st.check_fine > 0 && st.check_fine < st.check_termination && st.check_termination % st.check_fine == 0 &&
                    qp->nW > 0 && qp->C <= SCP_FINE_MAX_COLUMNS;
  return fine ? st.check_fine : 0;
}

// ---- the one way these files launch a kernel -------------------------------------------------------------------------------
inline dim3 grid1(int64_t n) { return dim3(scp_cdiv(n, 256)); }  // 256-thread workgroups over n items
// Launches `kernel` on the qp's stream and returns the hipGetLastError check.  The instantiations of one kernel template
// share a signature, so a call site picks one with `qp->D == 2 ? kern<2> : kern<3>` and writes the arguments once.  Dynamic
// LDS beyond 64 KiB (the column tiles from K = 51) needs the limit raised per (device, kernel): scp_raise_lds_limit
// remembers what it has raised.  Up to 64 KiB the launch makes no other runtime call.
template <typename... P, typename... A>
int qp_launch(scp_qp* qp, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A&&... args) {
  if (lds > 64 * 1024)
    SCP_HIP_CHECK(qp->ctx, scp_raise_lds_limit(qp->ctx->device, reinterpret_cast<const void*>(kernel), lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, qp->ctx->stream, static_cast<P>(args)...);
  SCP_HIP_CHECK(qp->ctx, hipGetLastError());
  return SCP_OK;
}

// ---- scp_qp_generic.hip: the generic pipeline ---------------------------------------------------------------------------------
constexpr int NPART = 128;  // partial sums of a dot product (fixed -> deterministic summation order)
int scp_qp_generic_iteration(scp_qp* qp, int* cg_count);  // one ADMM iteration: cg_iters PCG steps on the x-update
// residuals -> qp->h_scal[SL_RP..SL_NATY]; with_dy: also delta-y = y - snapshot (dyf / dyc, in place), its max norm and
// support value (SL_NDY, SL_SUPP).  Synchronises the stream.
int scp_qp_generic_residuals(scp_qp* qp, bool with_dy);
// second half of the certificate: || A^T dy ||_inf -> h_scal[SL_NATDY] (synchronises)
int scp_qp_generic_certificate_atdy(scp_qp* qp);
// S0 x exact for x, formed into rows [K, 2K) of HQ unless the carried copy is exact; with_fx: F x too
int scp_qp_exact_qx(scp_qp* qp, bool with_fx);
// the half of HQ that holds S0 x; other: the half the next single step writes
inline double* scp_qp_qx(const scp_qp* qp, bool other = false) {
  return (qp->dv.qx_half != 0) != other ? qp->d.HQ : qp->d.HQ + (int64_t)qp->K * qp->C;
}

// ---- scp_qp_rows.hip: the working rows and their incidence lists -------------------------------------------------------------
// append working rows [nW, nW + n): decode (k, i, j), copy eta / l, z = max(A x, l), y = 0.  eta_stride == 0: eta / l are
// gathered [n][D] / [n] arrays; > 0: the arrays of the pairwise pass over the pair range [q_begin, q_begin + nq)
int scp_qp_append_rows(scp_qp* qp, int64_t n, const int64_t* rows, const double* eta, const double* l, int64_t eta_stride,
                       int64_t q_begin, int64_t nq, const double* Qx);
// the incidence lists of the working set, built when they are stale
int scp_qp_csr_ensure(scp_qp* qp);
// Deterministic A_W^T g into the G slab: mode 0: g = rho_c zc - yc, 1: g = yc, 2: g = vec[n].  Two launches, no atomics.
int scp_qp_csr_scatter(scp_qp* qp, int mode, const double* vec);
// G = A_W^T g, g = rho A_W v with Q = S0 v: deterministic (gather over the incidence lists)
int scp_qp_rows_gather(scp_qp* qp, const double* Q);
// the lists (when stale) and the first row values g = (rho_c zc - yc) - rho_c eta.d(S0 x) of the single-step pipeline,
// Qx = S0 x exact: nothing, one workgroup's launch, or scp_qp_csr_ensure + one row launch (for scp_qp_cg1_prepare)
int scp_qp_rows_first_values(scp_qp* qp, const double* Qx);
// the carried row values from grow (per row) into gval (per entry), the lists built when stale: scp_qp_csr_ensure + one launch
int scp_qp_rows_values_to_entries(scp_qp* qp);
// the row vectors of a fused termination check into the entry arrays: gval2 = yc and, with_dy, gval3 = delta-yc
int scp_qp_rows_check_values(scp_qp* qp, bool with_dy);
// small problems: working rows [nW, nW + n) recomputed from the linearisation point (scp_qp_add_rows_at) AND the incidence
// lists + row values of all nW + n rows in ONE launch; *done = false: not eligible, nothing was launched
int scp_qp_install_rows_small(scp_qp* qp, int64_t n, const int64_t* rows, const double* pos_prev, const double* p0,
                              const double* v0, double R, const double* Qx, bool* done);
// small problems: scp_qp_reset(x0) AND the installation of the QP's first n rows in ONE launch (launch only: reset_impl in
// scp_qp.hip keeps the host-side state); *done = false: not eligible, nothing was launched
int scp_qp_reset_install_small(scp_qp* qp, const double* x0, int64_t n, const int64_t* rows, const double* pos_prev,
                               const double* p0, const double* v0, double R, double* Qx, bool* done);

// ---- scp_qp_columns.hip: the column kernels of the single-step pipeline, QP#0 and the termination check (use_mfma = 1) ----
constexpr int SCP_RESID_STRIDE = 12;  // doubles per workgroup in the partial results of a fused termination check
constexpr int SCP_RESID_CAP = (4096 / 2 + 128) * SCP_RESID_STRIDE;  // (SCP_PART_CAP / 2 column blocks + row blocks)
constexpr int SCP_BIGK_MAX_K = 1024;  // single-step pipeline with one workgroup per column and one thread per time step
constexpr int SCP_FUSED_MAX_K = 120;  // the 16-column workgroups of scp_qp_columns.hip (wave scans of up to 128 time steps)
constexpr int SCP_PART_CAP = 4096;  // capacity of each partial-sum array (column blocks of the single-step pipeline)
// single-PCG-step pipeline (cg_iters == 1 and a non-empty working set): 3 launches per ADMM step
int scp_qp_cg1_iteration(scp_qp* qp, int* cg_count, bool emit_dy);
// nW == 0: `nit` complete ADMM iterations in one launch (everything is column-local)
int scp_qp_qp0_iterations(scp_qp* qp, int nit, double* dy_out);
// the single-step pipeline's carried state (S0 x, F x, row values), brought in line with (x, zc, yc, rho) when it is not
int scp_qp_cg1_prepare(scp_qp* qp);
// Termination-check quantities of the single-step pipeline in 3 launches (row values, column blocks, rows):
// fills qp->h_scal[SL_RP .. SL_SUPP] like scp_qp_generic_residuals and leaves S0 x and F x in their slabs.  Synchronises.
// with_dy: dyf / dyc hold delta-y of the last iteration (cg1_update_kernel); also fills h_scal[SL_NATDY].
int scp_qp_fused_residuals(scp_qp* qp, bool with_dy);

// ---- scp_qp_persist.hip, scp_qp_persist16.hip: the persistent kernels ----------------------------------------------------------
constexpr int SCP_SYNC_WORDS = 16;  // u64: give-up word | scratch
// Workgroups of a persistent launch: at most one per CU (all resident), and the exchange buffers below are sized for
// exactly this many (+1: the fault-injection hook announces one workgroup more than it launches).
constexpr int SCP_PERSIST_MAX_WG = 256;
// No kernel's entry tables hold more rows than this: 160 KiB of LDS over the smallest entry (68 B, lean kernel in 2-D)
constexpr int SCP_PERSIST_CAP_MAX = 2432;
constexpr int SCP_GPART_WORDS = 2 * (SCP_PERSIST_MAX_WG + 1) * 4;  // two buffers x workgroups x two doubles as granule pairs
constexpr int SCP_GCHECK_WORDS = (SCP_PERSIST_MAX_WG + 1) * 9 * 2;  // nine check results per workgroup as granule pairs
bool scp_qp_persist_eligible(const scp_qp* qp);
// Compute units claimed by the persistent launches in flight on one device of THIS process (solver threads on several
// streams, compute-trajectories-batch): a launch needs all its workgroups resident at once, so it first claims one CU per
// workgroup.  scp_persist_claim waits up to `wait_ms` for the claim to fit (returns false otherwise: the caller runs this
// batch of iterations on the three-launch pipeline instead of discovering the shortage through a spin timeout).
bool scp_persist_claim(int device, int n_cu_total, int n_wg, int wait_ms);
void scp_persist_release(int device, int n_wg);
constexpr int SCP_PERSIST_GAVE_UP = 2;  // exit code of the persistent kernel: a spin timed out, nothing was written back
int scp_qp_cg1_persist(scp_qp* qp, int it0, int cad0, int* ran, int* code, int* it_done);  // cad0: steps to the next check

// ---- the only writers of QpDerived: one transition per event that happens to the primary state ---------------------------
// x set by a reset or a clone; qx: the reset's own launch formed S0 x (into rows [K, 2K) of HQ) and F x
inline void qp_on_x_set(scp_qp* qp, bool qx) {
  QpDerived& v = qp->dv;
  v.lists = v.carried = false; v.vals_rho_c = 0.0; v.qx = qx;
  if (qx) v.qx_half = 0;
}
// rows added; small_install: by the small install, which built the lists and every row value at the current rho
inline void qp_on_rows_added(scp_qp* qp, bool small_install) {
  qp->dv.lists = small_install; qp->dv.vals_rho_c = small_install ? qp->rho * qp->st.rho_col_scale : 0.0;
  qp->dv.carried = false;
}
// rho changed: the row values depend on it (in_kernel: the persistent kernel's own switch recomputed the carried ones)
inline void qp_on_rho_changed(scp_qp* qp, bool in_kernel) { qp->dv.vals_rho_c = 0.0; qp->dv.carried &= in_kernel; }
inline void qp_on_solve_start(scp_qp* qp) { qp->dv.carried = false; }  // (the settings may have changed)
// a check other than CG1's fused one: it and the generic iterations before it used G, gval and HQ as scratch
inline void qp_on_scratch_used(scp_qp* qp) { qp->dv.carried = qp->dv.qx = false; qp->dv.vals_rho_c = 0.0; }
inline void qp_on_fused_check(scp_qp* qp) { qp->dv.qx = true; }  // (S0 x and F x refreshed, the carried state kept)
inline void qp_on_cg1_step(scp_qp* qp) { qp->dv.qx = false; qp->dv.qx_half ^= 1; }
// a persistent launch ended: its last check left S0 x and F x exact.  After a give-up a workgroup may still have written
// back (the kernel's exit decision closes that window but cannot exclude it): the carried slabs may not match x / z / y.
// own_lists: the kernel built its own entry tables and row values and left the values per row -- gval (and the lists, where
// nobody has built them) do not belong to this state; whoever needs them goes through scp_qp_cg1_prepare.
inline void qp_on_persist_exit(scp_qp* qp, int code, bool own_lists) {
  qp->dv.qx = code != SCP_PERSIST_GAVE_UP;
  if (code == SCP_PERSIST_GAVE_UP) qp->dv.carried = false;
  else if (own_lists) qp->dv.carried = qp->dv.vals_by_row = true;
}
// what the rebuilds made (the iterations after scp_qp_cg1_prepare carry its row values on)
inline void qp_on_qx_built(scp_qp* qp, bool with_fx) { qp->dv.qx_half = 0; qp->dv.qx = with_fx; }
inline void qp_on_lists_built(scp_qp* qp) { qp->dv.lists = true; }
inline void qp_on_cg1_prepared(scp_qp* qp) {
  qp->dv.lists = qp->dv.carried = true; qp->dv.vals_by_row = false; qp->dv.vals_rho_c = 0.0;
}
inline void qp_on_vals_to_entries(scp_qp* qp) { qp->dv.vals_by_row = false; }  // (scp_qp_rows_values_to_entries)
