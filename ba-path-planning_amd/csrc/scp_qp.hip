// Joint QP of the SCP iteration on gfx950 (rows a3 / a6 / a9 of SURVEY.md section 8).
//
//   min ||x||^2   s.t.   l_f <= F x <= u_f  (jerk, acc, vel, pos rows; scp.py:182-257, :332-358)
//                        A_W x >= l_W       (working set of collision rows; scp.py:453-557)
//
// replaces osqp.OSQP().setup/warm_start/solve (scp.py:326-367, :441-449).  The algorithm is OSQP's ADMM
// (rho / sigma / alpha, rho x 1e3 on equality rows, adaptive rho, termination test every 25 iterations on the
// unscaled inf-norm residuals) with an indirect x-update, as OSQP's own GPU backend does:
//
//   ((2 + sigma) I + F^T R_f F + A_W^T R_c A_W) x~ = sigma x + F^T (R_f z_f - y_f) + A_W^T (R_c z_c - y_c)
//
// is solved by PCG.  The fixed part H_f = (2+sigma) I + F^T R_f F is the same K x K block for EVERY
// (agent, axis) column, so its exact inverse (one small dense factorisation per rho) is the
// preconditioner and is applied to all N*D columns at once as a [K x K] x [K x N*D] product on the fp64 MFMA
// units; A_W is never formed: row (k, i, j) is  eta . ((S0 x_i)[k] - (S0 x_j)[k]).
//
// Device layout: every vector lives time-major, [rows][C] with C = N*D columns (c = i*D + d).  Fixed rows are
// stacked as  [0,K-1) jerk | [K-1,2K-1) acc | [2K-1,3K-1) vel | [3K-1,4K-1) pos.
// oracle/qp_oracle.py:admm_structured is the line-by-line CPU statement of the solve.
//
// This file owns the solver object: the C-ABI (scp_qp_* of include/scp_hip.h), lifecycle and settings, the workspace
// carving, the host logic of reset / add rows, the choice of the ADMM pipeline and the scp_qp_solve loop, and the
// clone / get / peek / debug hooks.  The kernels live with their owners: scp_qp_generic.hip (one product per launch),
// scp_qp_columns.hip (column-block kernels), scp_qp_rows.hip (working rows, incidence lists), scp_qp_kkt.hip (per rho),
// scp_qp_persist*.hip (persistent kernels).  The one kernel here is the reset's own launch.
#include "scp_qp_internal.h"
#include "scp_reset_device.h"

#include <chrono>
#include <cmath>
#include <vector>

// scp_qp_reset in one launch (K <= SCP_FUSED_MAX_K): x0 in reference order [N][K][D] (null: zeros) -> x (time-major),
// z_f = F x, the carried F x and S0 x of the single-step pipeline (exact), y_f = 0.  16 columns per workgroup (256 columns
// of a 128-agent problem still make 16 workgroups), the x tile in LDS, thread = (column, one sixteenth of the rows).
__global__ __launch_bounds__(256) void qp_reset_kernel(int N, int K, int D, int Rf, const double* __restrict__ x0,
                                                        const double* __restrict__ F, const double* __restrict__ S0,
                                                        double* __restrict__ x, double* __restrict__ zf,
                                                        double* __restrict__ fx, double* __restrict__ Qx,
                                                        double* __restrict__ yf) {
  extern __shared__ double reset_xs[];  // [K][RESET_COLS]
  qp_reset_body<false>(threadIdx.x, true, reset_xs, N, K, D, Rf, x0, F, S0, x, zf, fx, Qx, yf);
}

// ... and the same outputs from a (column tile) x (row slab) grid that fills the chip (scp_reset_device.h): the reset's
// default form wherever its LDS tile fits ("reset_form" of scp_qp_debug_set: 0 = the kernel above)
__global__ __launch_bounds__(256) void qp_reset_tiled_kernel(int N, int K, int D, int Rf, const double* __restrict__ x0,
                                                              const double* __restrict__ F, const double* __restrict__ S0,
                                                              double* __restrict__ x, double* __restrict__ zf,
                                                              double* __restrict__ fx, double* __restrict__ Qx,
                                                              double* __restrict__ yf) {
  extern __shared__ double reset_tile[];  // [K][RESET_TILE] x tile | [RESET_SLAB][K] rows of F | S0
  qp_reset_tiled_body(reset_tile, N, K, D, Rf, x0, F, S0, x, zf, fx, Qx, yf);
}

// ----------------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------------
namespace {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct Carver {
  char* base;
  size_t off;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(count * sizeof(T));
    return p;
  }
};

size_t carve(QpDev& d, void* ws, int K, int64_t C, int64_t cap, int D) {
  const int Rf = 4 * K - 1;
  Carver c{static_cast<char*>(ws), 0};
  d.F = c.take<double>((size_t)Rf * K);
  d.Ft = c.take<double>((size_t)Rf * K);
  d.S0 = c.take<double>((size_t)K * K);
  d.S0t = c.take<double>((size_t)K * K);
  d.HS = d.Hf = d.Minv = nullptr;  // rho-dependent blocks live in the cache slots (scp_qp_kkt_init_slots), set by scp_qp_build_kkt
  d.aug = c.take<double>((size_t)2 * K * K);
  d.gj_tmp = c.take<double>((size_t)3 * K);
  d.wrow = c.take<double>((size_t)Rf);
  d.G0 = c.take<double>((size_t)K * K);
  d.pMinv = d.T = d.pT = nullptr;
  d.kkt_pool = c.take<double>(scp_qp_kkt_pool_doubles(K));
  const size_t nf = (size_t)Rf * C, nx = (size_t)K * C;
  d.lf = c.take<double>(nf);
  d.uf = c.take<double>(nf);
  d.zf = c.take<double>(nf);
  d.yf = c.take<double>(nf);
  d.wf = c.take<double>(nf);
  d.tf = c.take<double>(nf);
  d.states = c.take<double>((size_t)4 * C);
  d.x = c.take<double>(nx);
  d.xt = c.take<double>(nx);
  d.rhs = c.take<double>(nx);
  d.r = c.take<double>(nx);
  d.p = c.take<double>(nx);
  d.zz = c.take<double>(nx);
  d.G = c.take<double>(nx);
  d.HQ = c.take<double>(2 * nx);
  d.w_row = c.take<int64_t>((size_t)cap);
  d.w_k = c.take<int>((size_t)cap);
  d.w_i = c.take<int>((size_t)cap);
  d.w_j = c.take<int>((size_t)cap);
  d.w_eta = c.take<double>((size_t)cap * D);
  d.w_l = c.take<double>((size_t)cap);
  d.zc = c.take<double>((size_t)cap);
  d.yc = c.take<double>((size_t)cap);
  d.scal = c.take<double>(SL_COUNT + SCP_RESID_CAP);
  d.part = c.take<double>(2 * SCP_PART_CAP);
  d.s0p = c.take<double>(nx);
  d.fx = c.take<double>(nf);
  d.dyf = c.take<double>(nf);
  d.dyc = c.take<double>((size_t)cap);
  const size_t ncell = (size_t)(C / D) * K;
  d.cell_ptr = c.take<int>(ncell + 1);
  d.cell_cur = c.take<int>(ncell);
  d.scan_tot = c.take<int>(ncell / 4096 + 2);
  d.ent_code = c.take<int>((size_t)2 * cap);
  d.coef = c.take<double>((size_t)2 * cap * D);
  d.gval = c.take<double>((size_t)2 * cap);
  d.gval2 = c.take<double>((size_t)2 * cap);
  d.gval3 = c.take<double>((size_t)2 * cap);
  d.pos_i = c.take<int>((size_t)cap);
  d.pos_j = c.take<int>((size_t)cap);
  d.grow = c.take<double>((size_t)cap);
  d.own_code = c.take<int>((size_t)(SCP_PERSIST_MAX_WG + 1) * SCP_PERSIST_CAP_MAX);
  d.sync_words = c.take<unsigned long long>(SCP_SYNC_WORDS);
  d.cells = c.take<unsigned long long>((size_t)2 * nx);
  d.gpart = c.take<unsigned long long>(SCP_GPART_WORDS);
  d.gcheck = c.take<unsigned long long>(SCP_GCHECK_WORDS);
  return c.off;
}

}  // namespace

// ----------------------------------------------------------------------------------------------------
// C-ABI
// ----------------------------------------------------------------------------------------------------
extern "C" void scp_qp_default_settings(scp_qp_settings* s) {
  if (!s) return;
  s->rho = 0.1;
  s->sigma = 1e-6;
  s->alpha = 1.6;
  s->rho_eq_scale = 1e3;
  s->eps_abs = 1e-3;
  s->eps_rel = 1e-3;
  s->max_iter = 4000;
  s->check_termination = 25;
  s->check_fine = 5;
  s->check_fine_ratio = 2.0;
  s->adaptive_rho = 1;
  // OSQP's own default is a wall-clock rule (the first update once the iterations have cost a fraction of the setup time, i.e.
  // after some multiple of check_termination): not reproducible, and with no factorisation to amortise there is no setup time
  // to measure.  50 is a measured choice (profiles/r03_rho_interval_sweep.txt: 11 problems, 10 ... 4096 agents): the estimate
  // after 25 steps overshoots on the large problems (1024 x 50: rho 0.1 -> 0.011, 500 steps; after 50 steps: 250), 75 / 100
  // cost the small ones.  Total ADMM steps over the sweep 17 225 (25) / 15 500 (50) / 15 500 (75) / 15 950 (100).
  s->adaptive_rho_interval = 50;
  s->adaptive_rho_tolerance = 5.0;
  s->cg_iters = 1;
  s->use_mfma = 1;
  s->rho_col_scale = 10.0;
  s->eps_prim_inf = 1e-4;
  s->persistent = 1;
}

extern "C" size_t scp_qp_workspace_bytes(int N, int K, int D, int64_t row_capacity) {
  if (N <= 0 || K <= 1 || (D != 2 && D != 3) || row_capacity < 0) return 0;
  QpDev d;
  return carve(d, nullptr, K, (int64_t)N * D, row_capacity, D);
}

static int check_settings(scp_ctx* ctx, const scp_qp_settings* s) {
  SCP_REQUIRE(ctx, s->rho > 0 && s->sigma > 0 && s->alpha > 0 && s->alpha < 2 && s->rho_eq_scale > 0 &&
                       s->rho_col_scale > 0,
              "qp settings: rho/sigma/alpha out of range");
  SCP_REQUIRE(ctx, s->max_iter > 0 && s->check_termination > 0 && s->cg_iters >= 1, "qp settings: bad iteration counts");
  SCP_REQUIRE(ctx, s->check_fine >= 0 && s->check_fine_ratio >= 1.0, "qp settings: check_fine >= 0, check_fine_ratio >= 1");
  return SCP_OK;
}

extern "C" int scp_qp_create(scp_ctx* ctx, int N, int K, int D, double h, const scp_qp_settings* s, void* workspace,
                             size_t workspace_bytes, int64_t row_capacity, scp_qp** out) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, out && s && workspace, "qp_create: null pointer");
  SCP_REQUIRE(ctx, N > 0 && K > 1 && (D == 2 || D == 3) && h > 0 && row_capacity >= 0, "qp_create: bad shape");
  SCP_REQUIRE(ctx, (uintptr_t)workspace % 256 == 0, "qp_create: workspace must be 256-byte aligned");
  int rc = check_settings(ctx, s);
  if (rc) return rc;
  const size_t need = scp_qp_workspace_bytes(N, K, D, row_capacity);
  if (workspace_bytes < need)
    return scp_fail(ctx, SCP_ERR_CAPACITY, "qp_create: workspace %zu < %zu bytes", workspace_bytes, need);
  scp_qp* qp = new scp_qp();
  qp->ctx = ctx;
  qp->N = N; qp->K = K; qp->D = D; qp->Rf = 4 * K - 1; qp->C = (int64_t)N * D; qp->h = h;
  qp->st = *s;
  qp->row_cap = row_capacity;
  qp->nW = 0;
  qp->problem_set = qp->reset_done = false;
  qp->has_boxes = false;
  qp->rho = s->rho;
  carve(qp->d, workspace, K, qp->C, row_capacity, D);
  scp_qp_kkt_init_slots(qp);
  qp->check_seq = 0;
  qp->persist_off = false;
  qp->persist_skip_solve = false;
  qp->persist_gave_up_total = 0;
  qp->persist_variant = 0;
  qp->steps_since_reset = 0;
  memset(qp->lim, 0, sizeof(qp->lim));
  qp->persist_fault = 0;
  qp->reset_form = 1;
  {  // (the environment sets the hook's starting value: the QP objects inside scp_solver have no handle of their own)
    const char* e = getenv("SCP_PERSIST_HOST_LISTS");
    qp->persist_host_lists = e && atoi(e) != 0;
  }
  qp->persist_cap_nW = -1;
  qp->persist_cap = 0;
  qp->persist_epoch = 0;
  if (hipHostMalloc(&qp->h_scal, (SL_COUNT + SCP_RESID_CAP + 4) * sizeof(double),
                    hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void**)&qp->h_scal_dev, qp->h_scal, 0) != hipSuccess) {
    delete qp;
    return scp_fail(ctx, SCP_ERR_HIP, "qp_create: hipHostMalloc failed");
  }
  memset(qp->h_scal, 0, (SL_COUNT + SCP_RESID_CAP + 4) * sizeof(double));  // incl. the completion flag
  qp->h_persist = (unsigned*)(qp->h_scal + SL_COUNT + SCP_RESID_CAP + 1);  // status word of the persistent kernel
  qp->h_persist_dev = (unsigned*)(qp->h_scal_dev + SL_COUNT + SCP_RESID_CAP + 1);
  // constant blocks (scp.py:10-28, :198-203, :227-232, :489-491), built on the host once per (K, h)
  const int Rf = qp->Rf;
  std::vector<double> F((size_t)Rf * K, 0.0), Ft((size_t)Rf * K, 0.0), S0((size_t)K * K, 0.0), S0t((size_t)K * K, 0.0),
      w(Rf, 1.0);
  const double hh = h * h;
  for (int k = 0; k < K - 1; ++k) {  // jerk
    F[(size_t)k * K + k] = -1.0 / h;
    F[(size_t)k * K + k + 1] = 1.0 / h;
  }
  for (int k = 0; k < K; ++k) {
    F[(size_t)(K - 1 + k) * K + k] = 1.0;                                           // acc
    for (int m = 0; m <= k; ++m) F[(size_t)(2 * K - 1 + k) * K + m] = h;              // vel (state k+1)
    for (int m = 0; m <= k; ++m) F[(size_t)(3 * K - 1 + k) * K + m] = hh * (k - m + 0.5);  // pos (state k+1)
    for (int m = 0; m < k; ++m) S0[(size_t)k * K + m] = hh * (k - m - 0.5);           // stored sample k
  }
  for (int r = 0; r < Rf; ++r)
    for (int m = 0; m < K; ++m) Ft[(size_t)m * Rf + r] = F[(size_t)r * K + m];
  for (int k = 0; k < K; ++k)
    for (int m = 0; m < K; ++m) S0t[(size_t)m * K + k] = S0[(size_t)k * K + m];
  w[2 * K - 1 + K - 1] = s->rho_eq_scale;  // final velocity equality (scp.py:223-224)
  w[3 * K - 1 + K - 1] = s->rho_eq_scale;  // final position equality (scp.py:256-257)
  hipStream_t st = ctx->stream;
  const QpDev& d = qp->d;
  bool ok = hipMemcpyAsync(d.F, F.data(), F.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.Ft, Ft.data(), Ft.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.S0, S0.data(), S0.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.S0t, S0t.data(), S0t.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d.wrow, w.data(), w.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess;
  if (!ok) {
    (void)hipHostFree(qp->h_scal);
    delete qp;
    return scp_fail(ctx, SCP_ERR_HIP, "qp_create: constant upload failed");
  }
  if (scp_qp_build_g0(qp) != SCP_OK) {
    (void)hipHostFree(qp->h_scal);
    delete qp;
    return scp_fail(ctx, SCP_ERR_HIP, "qp_create: launch failed");
  }
  *out = qp;
  return SCP_OK;
}

extern "C" void scp_qp_destroy(scp_qp* qp) {
  if (!qp) return;
  (void)hipStreamSynchronize(qp->ctx->stream);
  (void)hipHostFree(qp->h_scal);
  delete qp;
}

extern "C" int scp_qp_update_settings(scp_qp* qp, const scp_qp_settings* s) {
  if (!qp || !s) return SCP_ERR_INVALID;
  int rc = check_settings(qp->ctx, s);
  if (rc) return rc;
  SCP_REQUIRE(qp->ctx, s->rho_eq_scale == qp->st.rho_eq_scale, "qp_update_settings: rho_eq_scale is fixed at create");
  qp->st = *s;
  return SCP_OK;
}

extern "C" int scp_qp_set_problem(scp_qp* qp, const double* limits, const double* space, const double* p0,
                                  const double* v0, const double* pf, const double* vf) {
  if (!qp) return SCP_ERR_INVALID;
  SCP_REQUIRE(qp->ctx, limits && space && p0 && v0 && pf && vf, "qp_set_problem: null pointer");
  QP_CHECK(scp_launch_bounds_time_major(qp->ctx, qp->N, qp->K, qp->D, qp->h, limits, space, p0, v0, pf, vf, qp->d.lf,
                                        qp->d.uf, qp->d.states));
  memcpy(qp->lim, limits, sizeof(qp->lim));
  for (int d = 0; d < 3; ++d) {
    qp->space[d] = d < qp->D ? space[d] : 0.0;
    qp->space[3 + d] = d < qp->D ? space[qp->D + d] : 0.0;
  }
  qp->problem_set = true;
  qp->has_boxes = false;  // (the launch above rewrote every bound)
  qp->reset_done = false;
  qp->persist_off = false;  // a give-up is a property of the moment (another kernel held the CUs), not of the object
  return SCP_OK;
}

extern "C" int scp_qp_set_position_boxes(scp_qp* qp, const double* lo, const double* hi) {
  if (!qp) return SCP_ERR_INVALID;
  if (!lo && !hi) return SCP_OK;
  SCP_REQUIRE(qp->ctx, lo && hi, "qp_set_position_boxes: lo and hi are both given or both NULL");
  if (!qp->problem_set) return scp_fail(qp->ctx, SCP_ERR_STATE, "qp_set_position_boxes: call scp_qp_set_problem first");
  QP_CHECK(scp_launch_position_boxes(qp->ctx, qp->N, qp->K, qp->D, qp->h, qp->space, qp->d.states, lo, hi, qp->d.lf, qp->d.uf));
  qp->has_boxes = true;
  return SCP_OK;
}

// eta_stride == 0: gathered rows (the public entry point); > 0: eta / l are the arrays of the pairwise pass over the pair
// range [q_begin, q_begin + nq), gathered by the kernel; at != nullptr: no stored rows at all, eta / l are recomputed from
// the linearisation point
struct RowsAt {
  const double *pos_prev, *p0, *v0;
  double R;
};

// scp_qp_reset; with `at`: the QP's first rows (recomputed from the linearisation point, scp_qp_add_rows_at) are installed
// by the SAME launch when the problem is small (*installed; otherwise only the reset has happened)
static int reset_impl(scp_qp* qp, const double* x0, int64_t n, const int64_t* rows, const RowsAt* at, bool* installed) {
  scp_ctx* ctx = qp->ctx;
  if (installed) *installed = false;
  if (!qp->problem_set) return scp_fail(ctx, SCP_ERR_STATE, "qp_reset: call scp_qp_set_problem first");
  const QpDev& d = qp->d;
  const int64_t nx = (int64_t)qp->K * qp->C, nf = (int64_t)qp->Rf * qp->C;
  const bool one_launch = qp->st.use_mfma == 1 && qp->K <= SCP_FUSED_MAX_K;
  qp->rho = qp->st.rho;
  bool with_rows = false;
  if (one_launch && at && ctx->small_pass && qp->st.cg_iters == 1 && n > 0 && n <= qp->row_cap)
    QP_CHECK(scp_qp_reset_install_small(qp, x0, n, rows, at->pos_prev, at->p0, at->v0, at->R, d.HQ + nx, &with_rows));
  if (with_rows) {
    // (the install launch did the reset too)
  } else if (one_launch) {
    // z = A x (primal warm start, scp.py:443), y = 0 and the single-step pipeline's carried F x, S0 x in one launch
    const size_t tiled_lds = qp_reset_tiled_lds_bytes(qp->K);
    if (qp->reset_form == 1 && tiled_lds <= 64 * 1024)
      QP_CHECK(qp_launch(qp, qp_reset_tiled_kernel,
                         dim3((unsigned)scp_cdiv(qp->C, RESET_TILE), (unsigned)scp_cdiv(qp->Rf + qp->K, RESET_SLAB)), dim3(256),
                         tiled_lds, qp->N, qp->K, qp->D, qp->Rf, x0, d.F, d.S0, d.x, d.zf, d.fx, d.HQ + nx, d.yf));
    else
      QP_CHECK(qp_launch(qp, qp_reset_kernel, dim3(scp_cdiv(qp->C, RESET_COLS)), dim3(256),
                         (size_t)qp->K * RESET_COLS * sizeof(double), qp->N, qp->K, qp->D, qp->Rf, x0, d.F, d.S0, d.x, d.zf,
                         d.fx, d.HQ + nx, d.yf));
  } else {
    if (x0) QP_CHECK(scp_launch_to_time_major(ctx, qp->N, qp->K, qp->D, x0, d.x));
    else SCP_HIP_CHECK(ctx, hipMemsetAsync(d.x, 0, nx * sizeof(double), ctx->stream));
    // z = A x  (primal warm start, scp.py:443)
    QP_CHECK(scp_launch_gemm(ctx, qp->st.use_mfma, qp->Rf, qp->K, (int)qp->C, 1.0, d.F, d.x, 0.0, d.zf));
    SCP_HIP_CHECK(ctx, hipMemsetAsync(d.yf, 0, nf * sizeof(double), ctx->stream));
  }
  qp->nW = with_rows ? n : 0;
  qp->persist_cap_nW = -1;
  qp->persist_off = false;  // every new QP tries the persistent path again
  qp->steps_since_reset = 0;
  qp_on_x_set(qp, one_launch);
  if (with_rows) qp_on_rows_added(qp, true);
  QP_CHECK(scp_qp_build_kkt(qp));
  qp->reset_done = true;
  if (installed) *installed = with_rows;
  return SCP_OK;
}

extern "C" int scp_qp_reset(scp_qp* qp, const double* x0) {
  if (!qp) return SCP_ERR_INVALID;
  return reset_impl(qp, x0, 0, nullptr, nullptr, nullptr);
}

extern "C" int scp_qp_set_rho(scp_qp* qp, double rho) {
  if (!qp) return SCP_ERR_INVALID;
  if (!qp->reset_done) return scp_fail(qp->ctx, SCP_ERR_STATE, "qp_set_rho: call scp_qp_reset first");
  SCP_REQUIRE(qp->ctx, rho >= 1e-6 && rho <= 1e6, "qp_set_rho: rho out of range");
  qp->rho = rho;
  qp_on_rho_changed(qp, false);
  return scp_qp_build_kkt(qp);
}

static int add_rows_impl(scp_qp* qp, int64_t n, const int64_t* rows, const double* eta, const double* l, int64_t eta_stride,
                         int64_t q_begin, int64_t nq, const RowsAt* at = nullptr) {
  scp_ctx* ctx = qp->ctx;
  if (!qp->reset_done) return scp_fail(ctx, SCP_ERR_STATE, "qp_add_rows: call scp_qp_reset first");
  if (n <= 0) return SCP_OK;
  SCP_REQUIRE(ctx, rows && (at || (eta && l)), "qp_add_rows: null pointer");
  if (qp->nW + n > qp->row_cap)
    return scp_fail(ctx, SCP_ERR_CAPACITY, "qp_add_rows: %lld + %lld rows exceed the capacity %lld",
                    (long long)qp->nW, (long long)n, (long long)qp->row_cap);
  const QpDev& d = qp->d;
  QP_CHECK(scp_qp_exact_qx(qp, false));  // S0 x for z_c = max(A_c x, l)
  const double* Qx = scp_qp_qx(qp);
  if (at) {
    bool installed = false;
    if (qp->st.use_mfma == 1 && qp->st.cg_iters == 1 && qp->K <= SCP_FUSED_MAX_K)  // (the single-step pipelines' lists)
      QP_CHECK(scp_qp_install_rows_small(qp, n, rows, at->pos_prev, at->p0, at->v0, at->R, Qx, &installed));
    if (installed) {
      qp->nW += n;
      qp->persist_cap_nW = -1;
      qp_on_rows_added(qp, true);
      return SCP_OK;
    }
    QP_CHECK(scp_launch_add_rows_at(ctx, qp->N, qp->K, qp->D, qp->nW, n, rows, at->pos_prev, at->p0, at->v0, at->R, qp->h, Qx,
                                    d.w_row, d.w_k, d.w_i, d.w_j, d.w_eta, d.w_l, d.zc, d.yc));
  } else {
    QP_CHECK(scp_qp_append_rows(qp, n, rows, eta, l, eta_stride, q_begin, nq, Qx));
  }
  qp->nW += n;
  qp->persist_cap_nW = -1;
  qp_on_rows_added(qp, false);
  return SCP_OK;
}

extern "C" int scp_qp_add_rows(scp_qp* qp, int64_t n, const int64_t* rows, const double* w_eta, const double* w_l) {
  if (!qp) return SCP_ERR_INVALID;
  return add_rows_impl(qp, n, rows, w_eta, w_l, 0, 0, 1);
}

extern "C" int scp_qp_add_rows_at(scp_qp* qp, int64_t n, const int64_t* rows, const double* pos_prev, const double* p0,
                                  const double* v0, double R) {
  if (!qp) return SCP_ERR_INVALID;
  SCP_REQUIRE(qp->ctx, n <= 0 || (pos_prev && p0 && v0), "qp_add_rows_at: null pointer");
  const RowsAt at{pos_prev, p0, v0, R};
  return add_rows_impl(qp, n, rows, nullptr, nullptr, 0, 0, 1, &at);
}

// scp_qp_reset(x0) followed by scp_qp_add_rows_at(rows): one launch for small problems (used by the native SCP loop), the
// two calls otherwise.  Same state, same bits either way.
int scp_qp_reset_add_rows_at(scp_qp* qp, const double* x0, int64_t n, const int64_t* rows, const double* pos_prev,
                             const double* p0, const double* v0, double R) {
  if (!qp) return SCP_ERR_INVALID;
  SCP_REQUIRE(qp->ctx, n <= 0 || (rows && pos_prev && p0 && v0), "qp_reset_add_rows_at: null pointer");
  const RowsAt at{pos_prev, p0, v0, R};
  bool installed = false;
  QP_CHECK(reset_impl(qp, x0, n, rows, &at, &installed));
  if (installed) return SCP_OK;
  return add_rows_impl(qp, n, rows, nullptr, nullptr, 0, 0, 1, &at);
}

// scp_gather_rows + scp_qp_add_rows in one launch (used by the native SCP loop): eta / l_col are the outputs of
// scp_linearize_pairs over the pair range [q_begin, q_end)
int scp_qp_add_rows_from_pass(scp_qp* qp, int64_t n, const int64_t* rows, const double* eta, const double* l_col,
                              int64_t q_begin, int64_t q_end) {
  if (!qp) return SCP_ERR_INVALID;
  SCP_REQUIRE(qp->ctx, q_begin >= 0 && q_end > q_begin && q_end <= scp_pairs(qp->N), "qp_add_rows_from_pass: bad pair range");
  return add_rows_impl(qp, n, rows, eta, l_col, scp_eta_stride(qp->K, q_end - q_begin), q_begin, q_end - q_begin);
}

// The ADMM pipeline of a solve.  Its inputs (settings, K, C, nW) do not change within a scp_qp_solve call.
enum class QpPipe {
  QP0,       // fixed rows only (everything is column-local): every iteration up to the next check in ONE launch
  CG1,       // single PCG step with collision rows: the persistent kernel where it runs, else the three launches
  CG1_BIGK,  // the same three launches with cg1_colK_kernel as the column kernel (K in 121..1024, e.g. the reference's
             // demo K = 500); its termination check is the generic one (snapshot of the duals)
  GENERIC    // one product per launch: cg_iters > 1, use_mfma 0 / 2, and shapes beyond the column kernels
};

static QpPipe choose_pipeline(const scp_qp* qp) {
  const scp_qp_settings& st = qp->st;
  if (st.use_mfma != 1) return QpPipe::GENERIC;
  const bool cols_fit = qp->K <= SCP_FUSED_MAX_K && (qp->C + 15) / 16 <= SCP_PART_CAP / 2;  // 16-column workgroups
  if (qp->nW == 0) return cols_fit ? QpPipe::QP0 : QpPipe::GENERIC;
  if (st.cg_iters != 1) return QpPipe::GENERIC;
  if (cols_fit) return QpPipe::CG1;
  if (qp->K > SCP_FUSED_MAX_K && qp->K <= SCP_BIGK_MAX_K && qp->C <= SCP_PART_CAP / 2) return QpPipe::CG1_BIGK;
  return QpPipe::GENERIC;
}

extern "C" int scp_qp_solve(scp_qp* qp, scp_qp_info* info) {
  if (!qp) return SCP_ERR_INVALID;
  scp_ctx* ctx = qp->ctx;
  if (!qp->reset_done) return scp_fail(ctx, SCP_ERR_STATE, "qp_solve: call scp_qp_reset first");
  SCP_REQUIRE(ctx, info, "qp_solve: null info");
  const scp_qp_settings& st = qp->st;
  const QpPipe pipe = choose_pipeline(qp);
  // QP0 and CG1 run their own termination check (scp_qp_fused_residuals), which also forms delta-y and |A^T dy|
  const bool own_check = pipe == QpPipe::QP0 || pipe == QpPipe::CG1;
  static constexpr int persist_pipe[] = {SCP_PIPE_PERSIST, SCP_PIPE_PERSIST16, SCP_PIPE_PERSIST8L};  // by persist_variant
  memset(info, 0, sizeof(*info));
  info->status_val = -2;  // OSQP_MAX_ITER_REACHED
  qp_on_solve_start(qp);
  qp->persist_skip_solve = false;
  const auto wall0 = std::chrono::steady_clock::now();
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int cg_total = 0, it = 0;
  int pipes = 0;
  double rp = INFINITY, rd = INFINITY;
  int cad = st.check_termination;  // steps between two checks (settings.check_fine: shorter once the residuals are close)
  const int fine = scp_qp_fine_cadence(qp);
  while (it < st.max_iter) {
    // the persistent single-step kernel runs the checks itself, returning only when the host has something to decide
    // (solved, infeasible, iteration limit, a rho update)
    bool persist_done = false;
    if (pipe == QpPipe::CG1 && !qp->persist_skip_solve && scp_qp_persist_eligible(qp)) {
      int ran = 0, code = 0, it_done = it;
      QP_CHECK(scp_qp_cg1_persist(qp, it, cad, &ran, &code, &it_done));
      if (ran && code == SCP_PERSIST_GAVE_UP) {
        // its workgroups were not all resident at once (e.g. the device is shared with another process's kernels): nothing
        // was written back, so the solve goes on from the same state on the three-launch pipeline and stays there until
        // the next scp_qp_reset re-arms the persistent path
        qp->persist_off = true;
        qp->persist_epoch = 0;
        ++info->persist_gave_up;
      } else if (ran) {
        ++info->persist_launches;
        info->rho_switches_in_kernel += qp->persist_rho_switches;
        pipes |= 1 << persist_pipe[qp->persist_variant];
        cg_total += it_done - it;
        qp->steps_since_reset += it_done - it;
        it = it_done;
        persist_done = true;
        if (qp->persist_rho_switches > 0) {
          // adaptive-rho updates whose blocks were cached happened inside the kernel (same test, same values as below):
          // adopt the result; scp_qp_build_kkt finds the slot and points d.* at it
          qp->rho = qp->persist_rho;
          qp_on_rho_changed(qp, true);
          info->rho_updates += qp->persist_rho_switches;
          QP_CHECK(scp_qp_build_kkt(qp));
        }
      }
    }
    int n_it = 1;
    if (!persist_done && pipe == QpPipe::QP0) {
      n_it = cad - it % cad;
      if (it + n_it > st.max_iter) n_it = st.max_iter - it;
    }
    if (!persist_done) {
      it += n_it;
      qp->steps_since_reset += n_it;
    }
    const bool will_check = persist_done || it % cad == 0 || it >= st.max_iter;
    const bool with_dy = will_check && st.eps_prim_inf > 0.0;
    if (!persist_done) {
      if (with_dy && !own_check) {  // snapshot of the duals: delta-y of this iteration feeds the certificate
        SCP_HIP_CHECK(ctx, hipMemcpyAsync(qp->d.dyf, qp->d.yf, (size_t)qp->Rf * qp->C * sizeof(double),
                                          hipMemcpyDeviceToDevice, ctx->stream));
        if (qp->nW > 0)
          SCP_HIP_CHECK(ctx, hipMemcpyAsync(qp->d.dyc, qp->d.yc, (size_t)qp->nW * sizeof(double),
                                            hipMemcpyDeviceToDevice, ctx->stream));
      }
      switch (pipe) {  // (CG1's update kernel emits delta-y itself)
        case QpPipe::QP0: QP_CHECK(scp_qp_qp0_iterations(qp, n_it, with_dy ? qp->d.dyf : nullptr)); pipes |= 1 << SCP_PIPE_QP0; break;
        case QpPipe::CG1: QP_CHECK(scp_qp_cg1_iteration(qp, &cg_total, with_dy)); pipes |= 1 << SCP_PIPE_CG1; break;
        case QpPipe::CG1_BIGK: QP_CHECK(scp_qp_cg1_iteration(qp, &cg_total, false)); pipes |= 1 << SCP_PIPE_CG1_BIGK; break;
        case QpPipe::GENERIC: QP_CHECK(scp_qp_generic_iteration(qp, &cg_total)); pipes |= 1 << SCP_PIPE_GENERIC; break;
      }
    }
    if (will_check) {
      if (persist_done) {
        // (the kernel left the nine check results in h_scal)
      } else if (own_check) {
        QP_CHECK(scp_qp_fused_residuals(qp, with_dy));
      } else {
        QP_CHECK(scp_qp_generic_residuals(qp, with_dy));
      }
      // QP0 takes the generic check's rule although its fused check refreshes S0 x and F x: rows added after QP#0 go in
      // by the general installation
      if (pipe != QpPipe::CG1) qp_on_scratch_used(qp);
      const double* hs = qp->h_scal;
      rp = hs[SL_RP];
      rd = hs[SL_RD];
      const double np = fmax(hs[SL_NAX], hs[SL_NZ]);
      const double nd = fmax(hs[SL_NPX], hs[SL_NATY]);
      const double tol_p = st.eps_abs + st.eps_rel * np, tol_d = st.eps_abs + st.eps_rel * nd;
      if (rp <= tol_p && rd <= tol_d) {
        info->status_val = 1;
        break;
      }
      if (fine)  // close to the tolerances: look again soon (the persistent kernels take the same decision)
        cad = (rp < st.check_fine_ratio * tol_p && rd < st.check_fine_ratio * tol_d) ? fine : st.check_termination;
      // OSQP at max_iter: the same test with ten times the tolerances -> "solved inaccurate" (status 2), which the
      // reference accepts like "solved" (scp.py:363, :446)
      if (it >= st.max_iter && rp <= 10.0 * (st.eps_abs + st.eps_rel * np) && rd <= 10.0 * (st.eps_abs + st.eps_rel * nd))
        info->status_val = 2;
      if (with_dy) {  // OSQP's is_primal_infeasible on the unscaled problem
        const double ndy = hs[SL_NDY], supp = hs[SL_SUPP];
        if (ndy > st.eps_prim_inf && supp < -st.eps_prim_inf * ndy) {
          if (!own_check) QP_CHECK(scp_qp_generic_certificate_atdy(qp));  // the fused check has |A^T dy| already
          if (qp->h_scal[SL_NATDY] < st.eps_prim_inf * ndy) {
            info->status_val = -3;
            break;
          }
        }
      }
      if (st.adaptive_rho && st.adaptive_rho_interval > 0 && it % st.adaptive_rho_interval == 0) {
        const double prim = rp / fmax(np, 1e-10);
        const double dual = rd / fmax(nd, 1e-10);
        double nr = qp->rho * std::sqrt(prim / fmax(dual, 1e-10));
        nr = fmin(fmax(nr, 1e-6), 1e6);
        // snapped to a geometric grid (steps of 2^(1/4)): the estimate is a ratio of small residuals; without the
        // grid 1e-13 of fp noise (atomics order, MFMA vs scalar sums) becomes a percent-level difference in rho and
        // an iterate path that differs from the oracle's at the 1e-4 level although both are valid solutions
        nr = std::exp2(std::round(4.0 * std::log2(nr)) / 4.0);
        if (nr > qp->rho * st.adaptive_rho_tolerance || nr < qp->rho / st.adaptive_rho_tolerance) {
          qp->rho = nr;
          qp_on_rho_changed(qp, false);
          QP_CHECK(scp_qp_build_kkt(qp));
          ++info->rho_updates;
          if (fine) cad = fine;  // (the residuals usually fall below the tolerances within a few steps)
        }
      }
    }
  }
  float ms = 0.f;
  if (ctx->timing) {
    SCP_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    SCP_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    SCP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  } else {  // (every exit of the loop above has read the solve's last check on the host: the device work is done)
    ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  info->iter = it;
  info->cg_iters_total = cg_total;
  info->working_rows = qp->nW;
  info->r_prim = rp;
  info->r_dual = rd;
  info->rho = qp->rho;
  info->solve_ms = ms;
  info->pipeline = pipes;
  return SCP_OK;
}

extern "C" int scp_qp_clone_state(scp_qp* dst, const scp_qp* src) {
  if (!dst || !src) return SCP_ERR_INVALID;
  scp_ctx* ctx = dst->ctx;
  SCP_REQUIRE(ctx, dst->N == src->N && dst->K == src->K && dst->D == src->D && dst->h == src->h,
              "qp_clone_state: shapes differ");
  if (!src->reset_done) return scp_fail(ctx, SCP_ERR_STATE, "qp_clone_state: source has no state");
  if (src->nW > dst->row_cap)
    return scp_fail(ctx, SCP_ERR_CAPACITY, "qp_clone_state: %lld rows exceed the capacity %lld", (long long)src->nW,
                    (long long)dst->row_cap);
  hipStream_t s = ctx->stream;
  const size_t nf = (size_t)src->Rf * src->C * sizeof(double), nx = (size_t)src->K * src->C * sizeof(double);
  const size_t nw = (size_t)src->nW;
  const QpDev &a = src->d, &b = dst->d;
#define CP(field, bytes) SCP_HIP_CHECK(ctx, hipMemcpyAsync(b.field, a.field, (bytes), hipMemcpyDeviceToDevice, s))
  CP(lf, nf); CP(uf, nf); CP(zf, nf); CP(yf, nf); CP(x, nx);
  CP(states, (size_t)4 * src->C * sizeof(double));
  // S0 x and F x as the source's last check left them travel along: formed again from x (scp_qp_exact_qx) they would differ
  // in the last bits, and the solve in the larger workspace would no longer be the solve that did not have to grow
  const bool qx = src->dv.qx;
  if (qx) {
    SCP_HIP_CHECK(ctx, hipMemcpyAsync(b.HQ + (int64_t)src->K * src->C, scp_qp_qx(src), nx, hipMemcpyDeviceToDevice, s));
    CP(fx, nf);
  }
  if (nw) {
    CP(w_row, nw * sizeof(int64_t)); CP(w_k, nw * sizeof(int)); CP(w_i, nw * sizeof(int)); CP(w_j, nw * sizeof(int));
    CP(w_eta, nw * src->D * sizeof(double)); CP(w_l, nw * sizeof(double)); CP(zc, nw * sizeof(double));
    CP(yc, nw * sizeof(double));
  }
#undef CP
  memcpy(dst->lim, src->lim, sizeof(dst->lim));
  memcpy(dst->space, src->space, sizeof(dst->space));
  dst->steps_since_reset = src->steps_since_reset;
  dst->nW = src->nW;
  dst->persist_cap_nW = -1;
  dst->rho = src->rho;
  dst->st = src->st;
  dst->problem_set = true;
  dst->has_boxes = src->has_boxes;  // (lf / uf were copied)
  qp_on_x_set(dst, qx);
  QP_CHECK(scp_qp_build_kkt(dst));
  dst->reset_done = true;
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // src's workspace may be released by the caller right after
  return SCP_OK;
}

extern "C" int scp_qp_get_solution(scp_qp* qp, double* x_out) {
  if (!qp) return SCP_ERR_INVALID;
  SCP_REQUIRE(qp->ctx, x_out, "qp_get_solution: null pointer");
  if (!qp->reset_done) return scp_fail(qp->ctx, SCP_ERR_STATE, "qp_get_solution: no solve yet");
  return scp_launch_from_time_major(qp->ctx, qp->N, qp->K, qp->D, qp->d.x, x_out);
}

const double* scp_qp_solution_tm(const scp_qp* qp) { return qp->d.x; }

extern "C" int scp_qp_get_duals(scp_qp* qp, double* y_fixed, double* y_col) {
  if (!qp) return SCP_ERR_INVALID;
  scp_ctx* ctx = qp->ctx;
  if (!qp->reset_done) return scp_fail(ctx, SCP_ERR_STATE, "qp_get_duals: no solve yet");
  const int N = qp->N, K = qp->K, D = qp->D;
  const int64_t C = qp->C;
  if (y_fixed) {
    // blocks back to the reference stacking order (scp.py:342-358)
    QP_CHECK(scp_launch_from_time_major(ctx, N, K - 1, D, qp->d.yf, y_fixed));
    int64_t src = (int64_t)(K - 1) * C, dst = (int64_t)N * (K - 1) * D;
    for (int b = 0; b < 3; ++b) {
      QP_CHECK(scp_launch_from_time_major(ctx, N, K, D, qp->d.yf + src, y_fixed + dst));
      src += (int64_t)K * C;
      dst += (int64_t)N * K * D;
    }
  }
  if (y_col && qp->nW > 0)
    SCP_HIP_CHECK(ctx, hipMemcpyAsync(y_col, qp->d.yc, qp->nW * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return SCP_OK;
}

// test hook: copy one internal array of the solver to `out` (device pointer, capacity `cap` doubles); *n_out [host] = its
// length.  names: "fx" (carried F x, [4K-1][C]), "qx" (carried S0 x, [K][C]), "gval" (row value per incidence entry),
// "zf", "yf", "lf", "uf" ([4K-1][C]; lf / uf: the bounds of the fixed rows), "zc", "yc" (per working row), "x" ([K][C]);
// "Hf", "Minv", "T" (K x K, row-major): the blocks of
// the current rho (H_f, its inverse, T = S0 H_f^{-1}) in the active cache slot.
extern "C" int scp_qp_peek(scp_qp* qp, const char* name, double* out, int64_t cap, int64_t* n_out) {
  if (!qp) return SCP_ERR_INVALID;
  scp_ctx* ctx = qp->ctx;
  SCP_REQUIRE(ctx, name && out && n_out, "qp_peek: null pointer");
  const QpDev& d = qp->d;
  const int64_t nf = (int64_t)qp->Rf * qp->C, nx = (int64_t)qp->K * qp->C;
  const double* src = nullptr;
  int64_t n = 0;
  if (!strcmp(name, "fx")) { src = d.fx; n = nf; }
  else if (!strcmp(name, "qx")) { src = scp_qp_qx(qp); n = nx; }
  else if (!strcmp(name, "gval")) {
    if (qp->dv.carried && qp->dv.vals_by_row) QP_CHECK(scp_qp_rows_values_to_entries(qp));
    src = d.gval; n = 2 * qp->nW;
  }
  else if (!strcmp(name, "zf")) { src = d.zf; n = nf; }
  else if (!strcmp(name, "lf")) { src = d.lf; n = nf; }
  else if (!strcmp(name, "uf")) { src = d.uf; n = nf; }
  else if (!strcmp(name, "yf")) { src = d.yf; n = nf; }
  else if (!strcmp(name, "zc")) { src = d.zc; n = qp->nW; }
  else if (!strcmp(name, "yc")) { src = d.yc; n = qp->nW; }
  else if (!strcmp(name, "x")) { src = d.x; n = nx; }
  else if (!strcmp(name, "w_eta")) { src = d.w_eta; n = qp->nW * qp->D; }
  else if (!strcmp(name, "w_l")) { src = d.w_l; n = qp->nW; }
  else if (!strcmp(name, "p")) { src = d.p; n = nx; }
  else if (!strcmp(name, "qp")) { src = d.s0p; n = nx; }
  else if (!strcmp(name, "Hf")) { src = d.Hf; n = (int64_t)qp->K * qp->K; }
  else if (!strcmp(name, "Minv")) { src = d.Minv; n = (int64_t)qp->K * qp->K; }
  else if (!strcmp(name, "T")) { src = d.T; n = (int64_t)qp->K * qp->K; }
  else return scp_fail(ctx, SCP_ERR_INVALID, "qp_peek: unknown array %s", name);
  *n_out = n;
  if (n > cap) return scp_fail(ctx, SCP_ERR_CAPACITY, "qp_peek: %lld doubles needed", (long long)n);
  if (n > 0) SCP_HIP_CHECK(ctx, hipMemcpyAsync(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return SCP_OK;
}

// test hook: "persist_fault" = n makes the next n persistent launches wait for a workgroup that does not exist (exercises
// the give-up path); "persist_off" reads (value < 0) or sets whether the solver has fallen back to the three-launch
// pipeline; "persist_host_lists" = 1: the host builds the incidence lists and the row values before every persistent launch
// and the kernel loads its slice of them, instead of building its own tables (SCP_PERSIST_HOST_LISTS=1 in the environment:
// every QP object starts with it set); "reset_form" = 0: scp_qp_reset's one-launch form runs as the 16-column kernel
// (qp_reset_kernel), 1 (default): as the tiled kernel where its LDS fits.  Returns the value in effect, or SCP_ERR_INVALID.
extern "C" int scp_qp_debug_set(scp_qp* qp, const char* key, int value) {
  if (!qp || !key) return SCP_ERR_INVALID;
  if (!strcmp(key, "persist_fault")) {
    if (value >= 0) qp->persist_fault = value;
    return qp->persist_fault;
  }
  if (!strcmp(key, "persist_host_lists")) {
    if (value >= 0) qp->persist_host_lists = value != 0;
    return qp->persist_host_lists ? 1 : 0;
  }
  if (!strcmp(key, "reset_form")) {
    if (value >= 0) qp->reset_form = value != 0 ? 1 : 0;
    return qp->reset_form;
  }
  if (!strcmp(key, "persist_off")) {
    if (value >= 0) qp->persist_off = value != 0;
    return qp->persist_off ? 1 : 0;
  }
  if (!strcmp(key, "persist_gave_up_total")) return qp->persist_gave_up_total;  // (read only)
  return scp_fail(qp->ctx, SCP_ERR_INVALID, "qp_debug_set: unknown key %s", key);
}
