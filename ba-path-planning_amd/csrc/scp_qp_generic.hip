// The generic pipeline of the joint QP: one product per launch.  It runs cg_iters > 1, use_mfma = 0 / 2 and the shapes
// beyond the column kernels (choose_pipeline in scp_qp.hip), and is the plain statement of the algorithm described at the
// top of scp_qp.hip.  This file owns its elementwise / PCG / residual kernels and what launches them: one ADMM iteration,
// the termination check, the second half of the infeasibility certificate, and the exact S0 x / F x products.
#include "scp_qp_device.h"

#include <algorithm>

// ----------------------------------------------------------------------------------------------------
// kernels
// ----------------------------------------------------------------------------------------------------
__device__ inline double sum_partials(const double* part) {
  double s = 0.0;
  for (int b = 0; b < NPART; ++b) s += part[b];
  return s;
}

// part[b] = sum over this block's grid-stride share of a.b (fixed tree, deterministic)
__global__ __launch_bounds__(256) void dot_partial_kernel(int64_t n, const double* __restrict__ a,
                                                           const double* __restrict__ b, double* __restrict__ part) {
  __shared__ double s[4];
  double acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)NPART * 256) acc += a[t] * b[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// wf = rho * w[row] * zf - yf   (Rf x C);  rhs = sigma * x  (K x C, first K*C threads)
__global__ __launch_bounds__(256) void admm_rhs_prep_kernel(int64_t nf, int64_t nx, int64_t C, double rho, double sigma,
                                                             const double* __restrict__ wrow,
                                                             const double* __restrict__ zf,
                                                             const double* __restrict__ yf, double* __restrict__ wf,
                                                             const double* __restrict__ x, double* __restrict__ rhs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nf) wf[t] = rho * wrow[t / C] * zf[t] - yf[t];
  if (t < nx) rhs[t] = sigma * x[t];
}

enum RowMode { ROW_RHS = 0, ROW_HMUL = 1, ROW_Y = 2, ROW_VEC = 3 };

// r = rhs - Hx
__global__ __launch_bounds__(256) void cg_residual_kernel(int64_t n, const double* __restrict__ rhs,
                                                           const double* __restrict__ Hx, double* __restrict__ r) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) r[t] = rhs[t] - Hx[t];
}

// p = zz ; scal[SL_RZ0] = sum(part)
__global__ __launch_bounds__(256) void cg_start_kernel(int64_t n, const double* __restrict__ zz, double* __restrict__ p,
                                                        const double* __restrict__ part, double* __restrict__ scal) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) p[t] = zz[t];
  if (t == 0) scal[SL_RZ0] = sum_partials(part);
}

// alpha = rz / pHp ; xt += alpha p ; r -= alpha Hp
__global__ __launch_bounds__(256) void cg_update_kernel(int64_t n, int slot, const double* __restrict__ scal,
                                                         const double* __restrict__ part_pHp,
                                                         const double* __restrict__ p, const double* __restrict__ Hp,
                                                         double* __restrict__ xt, double* __restrict__ r) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double rz = scal[slot];
  const double pHp = sum_partials(part_pHp);
  const double alpha = (pHp > 0.0 && rz != 0.0) ? rz / pHp : 0.0;
  if (t < n) {
    xt[t] += alpha * p[t];
    r[t] -= alpha * Hp[t];
  }
}

// beta = rz_new / rz ; p = zz + beta p ; scal[slot^1] = rz_new
__global__ __launch_bounds__(256) void cg_direction_kernel(int64_t n, int slot, double* __restrict__ scal,
                                                            const double* __restrict__ part_rz,
                                                            const double* __restrict__ zz, double* __restrict__ p) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double rz = scal[slot];
  const double rz_new = sum_partials(part_rz);
  const double beta = rz != 0.0 ? rz_new / rz : 0.0;
  if (t < n) p[t] = zz[t] + beta * p[t];
  if (t == 0) scal[slot ^ 1] = rz_new;
}

// fixed rows: relaxation, projection, dual update (OSQP steps 4-6);  x = alpha xt + (1-alpha) x
__global__ __launch_bounds__(256) void admm_fixed_update_kernel(int64_t nf, int64_t nx, int64_t C, double rho,
                                                                 double alpha, const double* __restrict__ wrow,
                                                                 const double* __restrict__ tf,
                                                                 const double* __restrict__ lf,
                                                                 const double* __restrict__ uf, double* __restrict__ zf,
                                                                 double* __restrict__ yf, const double* __restrict__ xt,
                                                                 double* __restrict__ x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nf) {
    const double rr = rho * wrow[t / C];
    double zn, yn;
    scpdev::admm_project(alpha * tf[t] + (1.0 - alpha) * zf[t], yf[t], rr, lf[t], uf[t], zn, yn);
    yf[t] = yn;
    zf[t] = zn;
  }
  if (t < nx) x[t] = alpha * xt[t] + (1.0 - alpha) * x[t];
}

// collision rows: same update with u = +inf
template <int D>
__global__ __launch_bounds__(256) void admm_row_update_kernel(int64_t nW, int64_t C, double rho, double alpha,
                                                               const int* __restrict__ wk, const int* __restrict__ wi,
                                                               const int* __restrict__ wj,
                                                               const double* __restrict__ weta,
                                                               const double* __restrict__ wl,
                                                               const double* __restrict__ Q, double* __restrict__ zc,
                                                               double* __restrict__ yc) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= nW) return;
  const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
  const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
  double tc = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) tc += weta[n * D + d] * (Q[bi + d] - Q[bj + d]);
  double zn, yn;
  scpdev::admm_project(alpha * tc + (1.0 - alpha) * zc[n], yc[n], rho, wl[n], zn, yn);
  yc[n] = yn;
  zc[n] = zn;
}

__device__ inline void atomic_max_nonneg(double* addr, double v) {
  atomicMax((unsigned long long*)addr, (unsigned long long)__double_as_longlong(v));
}

__device__ inline double block_max(double v) {
  __shared__ double s[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const double m = fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
  __syncthreads();
  return m;
}

// primal residual pieces over the fixed rows: max|Fx - z|, max|Fx|, max|z|
__global__ __launch_bounds__(256) void resid_fixed_kernel(int64_t nf, const double* __restrict__ tf,
                                                           const double* __restrict__ zf, double* __restrict__ scal) {
  double rp = 0.0, na = 0.0, nz = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nf; t += (int64_t)gridDim.x * 256) {
    const double a = tf[t], z = zf[t];
    rp = fmax(rp, fabs(a - z));
    na = fmax(na, fabs(a));
    nz = fmax(nz, fabs(z));
  }
  rp = block_max(rp);
  na = block_max(na);
  nz = block_max(nz);
  if (threadIdx.x == 0) {
    atomic_max_nonneg(scal + SL_RP, rp);
    atomic_max_nonneg(scal + SL_NAX, na);
    atomic_max_nonneg(scal + SL_NZ, nz);
  }
}

template <int D>
__global__ __launch_bounds__(256) void resid_rows_kernel(int64_t nW, int64_t C, const int* __restrict__ wk,
                                                          const int* __restrict__ wi, const int* __restrict__ wj,
                                                          const double* __restrict__ weta,
                                                          const double* __restrict__ Q, const double* __restrict__ zc,
                                                          double* __restrict__ scal) {
  double rp = 0.0, na = 0.0, nz = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nW; n += (int64_t)gridDim.x * 256) {
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
    double a = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) a += weta[n * D + d] * (Q[bi + d] - Q[bj + d]);
    const double z = zc[n];
    rp = fmax(rp, fabs(a - z));
    na = fmax(na, fabs(a));
    nz = fmax(nz, fabs(z));
  }
  rp = block_max(rp);
  na = block_max(na);
  nz = block_max(nz);
  if (threadIdx.x == 0) {
    atomic_max_nonneg(scal + SL_RP, rp);
    atomic_max_nonneg(scal + SL_NAX, na);
    atomic_max_nonneg(scal + SL_NZ, nz);
  }
}

// dual residual pieces: max|2x + ATy|, max|2x|, max|ATy|
__global__ __launch_bounds__(256) void resid_dual_kernel(int64_t nx, const double* __restrict__ x,
                                                          const double* __restrict__ aty, double* __restrict__ scal) {
  double rd = 0.0, npx = 0.0, nat = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nx; t += (int64_t)gridDim.x * 256) {
    const double px = 2.0 * x[t], a = aty[t];
    rd = fmax(rd, fabs(px + a));
    npx = fmax(npx, fabs(px));
    nat = fmax(nat, fabs(a));
  }
  rd = block_max(rd);
  npx = block_max(npx);
  nat = block_max(nat);
  if (threadIdx.x == 0) {
    atomic_max_nonneg(scal + SL_RD, rd);
    atomic_max_nonneg(scal + SL_NPX, npx);
    atomic_max_nonneg(scal + SL_NATY, nat);
  }
}

// primal infeasibility certificate, fixed rows: dy = y - snapshot (in place), max |dy|, sum u dy+ + l dy-
__global__ __launch_bounds__(256) void dy_fixed_kernel(int64_t nf, const double* __restrict__ yf,
                                                        const double* __restrict__ lf, const double* __restrict__ uf,
                                                        double* __restrict__ dyf, double* __restrict__ scal) {
  __shared__ double ssum[4];
  double mx = 0.0, sup = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nf; t += (int64_t)gridDim.x * 256) {
    const double d = yf[t] - dyf[t];
    dyf[t] = d;
    mx = fmax(mx, fabs(d));
    sup += uf[t] * fmax(d, 0.0) + lf[t] * fmin(d, 0.0);
  }
  mx = block_max(mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sup += __shfl_xor(sup, o);
  if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = sup;
  __syncthreads();
  if (threadIdx.x == 0) {
    atomic_max_nonneg(scal + SL_NDY, mx);
    atomicAdd(scal + SL_SUPP, (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]));
  }
}

// collision rows (u = +inf): dy = min(y - snapshot, 0)
__global__ __launch_bounds__(256) void dy_rows_kernel(int64_t nW, const double* __restrict__ yc,
                                                       const double* __restrict__ wl, double* __restrict__ dyc,
                                                       double* __restrict__ scal) {
  __shared__ double ssum[4];
  double mx = 0.0, sup = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nW; n += (int64_t)gridDim.x * 256) {
    const double d = fmin(yc[n] - dyc[n], 0.0);
    dyc[n] = d;
    mx = fmax(mx, fabs(d));
    sup += wl[n] * d;
  }
  mx = block_max(mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sup += __shfl_xor(sup, o);
  if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = sup;
  __syncthreads();
  if (threadIdx.x == 0) {
    atomic_max_nonneg(scal + SL_NDY, mx);
    atomicAdd(scal + SL_SUPP, (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]));
  }
}

__global__ __launch_bounds__(256) void max_abs_kernel(int64_t n, const double* __restrict__ v, double* __restrict__ slot) {
  double mx = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) mx = fmax(mx, fabs(v[t]));
  mx = block_max(mx);
  if (threadIdx.x == 0) atomic_max_nonneg(slot, mx);
}

// ----------------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------------
namespace {

int gemm(scp_qp* qp, int R, int M, double alpha, const double* A, const double* X, double beta, double* Y) {
  return scp_launch_gemm(qp->ctx, qp->st.use_mfma, R, M, (int)qp->C, alpha, A, X, beta, Y);
}

// G = A_W^T g over the working rows, g by mode (a gather over the sorted incidence lists: fixed summation order; the
// round-1 version scattered with atomics):
//   ROW_RHS : rho zc - yc            (right-hand side of the x-update)
//   ROW_HMUL: rho eta.(Q_i - Q_j)    (A_W^T R_c A_W v, Q = S0 v)
//   ROW_Y   : yc                     (A_W^T y for the dual residual)
//   ROW_VEC : vec                    (an arbitrary row vector)
template <int MODE>
int row_scatter(scp_qp* qp, const double* Q, const double* vec = nullptr) {
  if (MODE == ROW_HMUL) return scp_qp_rows_gather(qp, Q);
  return scp_qp_csr_scatter(qp, MODE == ROW_RHS ? 0 : (MODE == ROW_Y ? 1 : 2), vec);
}

// HQ[0:K] = H v = Hf v + A_W^T R_c A_W v ; HQ[K:2K] = S0 v
int hmul(scp_qp* qp, const double* v) {
  const QpDev& d = qp->d;
  const int K = qp->K;
  QP_CHECK(gemm(qp, 2 * K, K, 1.0, d.HS, v, 0.0, d.HQ));
  if (qp->nW > 0) {
    QP_CHECK(row_scatter<ROW_HMUL>(qp, d.HQ + (size_t)K * qp->C));
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0t, d.G, 1.0, d.HQ));
  }
  return SCP_OK;
}

int dot_partial(scp_qp* qp, const double* a, const double* b, double* part) {
  return qp_launch(qp, dot_partial_kernel, dim3(NPART), dim3(256), 0, (int64_t)qp->K * qp->C, a, b, part);
}

// grid of the grid-stride row kernels of a check: one workgroup per 256 rows, 256 at the most
inline dim3 row_blocks(int64_t nW) { return dim3((unsigned)std::min<int64_t>((nW + 255) / 256, 256)); }

}  // namespace

int scp_qp_generic_iteration(scp_qp* qp, int* cg_count) {
  const QpDev& d = qp->d;
  scp_ctx* ctx = qp->ctx;
  hipStream_t s = ctx->stream;
  const int K = qp->K, Rf = qp->Rf;
  const int64_t C = qp->C, nf = (int64_t)Rf * C, nx = (int64_t)K * C;
  const dim3 b256(256);
  // rhs = sigma x + F^T (R_f z_f - y_f) + A_W^T (R_c z_c - y_c)
  QP_CHECK(qp_launch(qp, admm_rhs_prep_kernel, grid1(nf), b256, 0, nf, nx, C, qp->rho, qp->st.sigma, d.wrow, d.zf, d.yf, d.wf,
                     d.x, d.rhs));
  QP_CHECK(gemm(qp, K, Rf, 1.0, d.Ft, d.wf, 1.0, d.rhs));
  if (qp->nW > 0) {
    QP_CHECK(row_scatter<ROW_RHS>(qp, nullptr));
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0t, d.G, 1.0, d.rhs));
    // PCG on H x~ = rhs, preconditioner Minv, warm start x~ = x
    SCP_HIP_CHECK(ctx, hipMemcpyAsync(d.xt, d.x, nx * sizeof(double), hipMemcpyDeviceToDevice, s));
    QP_CHECK(hmul(qp, d.xt));
    QP_CHECK(qp_launch(qp, cg_residual_kernel, grid1(nx), b256, 0, nx, d.rhs, d.HQ, d.r));
    QP_CHECK(gemm(qp, K, K, 1.0, d.Minv, d.r, 0.0, d.zz));
    QP_CHECK(dot_partial(qp, d.r, d.zz, d.part));
    QP_CHECK(qp_launch(qp, cg_start_kernel, grid1(nx), b256, 0, nx, d.zz, d.p, d.part, d.scal));
    int slot = SL_RZ0;
    for (int it = 0; it < qp->st.cg_iters; ++it) {
      QP_CHECK(hmul(qp, d.p));
      QP_CHECK(dot_partial(qp, d.p, d.HQ, d.part));
      QP_CHECK(qp_launch(qp, cg_update_kernel, grid1(nx), b256, 0, nx, slot, d.scal, d.part, d.p, d.HQ, d.xt, d.r));
      QP_CHECK(gemm(qp, K, K, 1.0, d.Minv, d.r, 0.0, d.zz));
      QP_CHECK(dot_partial(qp, d.r, d.zz, d.part + NPART));
      QP_CHECK(qp_launch(qp, cg_direction_kernel, grid1(nx), b256, 0, nx, slot, d.scal, d.part + NPART, d.zz, d.p));
      slot ^= 1;
      ++*cg_count;
    }
  } else {
    QP_CHECK(gemm(qp, K, K, 1.0, d.Minv, d.rhs, 0.0, d.xt));
  }
  // z~ = A x~, relaxation, projection, duals
  QP_CHECK(gemm(qp, Rf, K, 1.0, d.F, d.xt, 0.0, d.tf));
  if (qp->nW > 0) {
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0, d.xt, 0.0, d.HQ + nx));
    QP_CHECK(qp_launch(qp, qp->D == 2 ? admm_row_update_kernel<2> : admm_row_update_kernel<3>, grid1(qp->nW), b256, 0, qp->nW,
                       C, qp->rho * qp->st.rho_col_scale, qp->st.alpha, d.w_k, d.w_i, d.w_j, d.w_eta, d.w_l, d.HQ + nx, d.zc,
                       d.yc));
  }
  return qp_launch(qp, admm_fixed_update_kernel, grid1(nf), b256, 0, nf, nx, C, qp->rho, qp->st.alpha, d.wrow, d.tf, d.lf,
                   d.uf, d.zf, d.yf, d.xt, d.x);
}

int scp_qp_generic_residuals(scp_qp* qp, bool with_dy) {
  const QpDev& d = qp->d;
  scp_ctx* ctx = qp->ctx;
  hipStream_t s = ctx->stream;
  const int K = qp->K, Rf = qp->Rf;
  const int64_t C = qp->C, nf = (int64_t)Rf * C, nx = (int64_t)K * C;
  const dim3 b256(256);
  SCP_HIP_CHECK(ctx, hipMemsetAsync(d.scal + SL_RP, 0, 9 * sizeof(double), s));
  if (with_dy) {
    QP_CHECK(qp_launch(qp, dy_fixed_kernel, dim3(256), b256, 0, nf, d.yf, d.lf, d.uf, d.dyf, d.scal));
    if (qp->nW > 0) QP_CHECK(qp_launch(qp, dy_rows_kernel, row_blocks(qp->nW), b256, 0, qp->nW, d.yc, d.w_l, d.dyc, d.scal));
  }
  QP_CHECK(gemm(qp, Rf, K, 1.0, d.F, d.x, 0.0, d.tf));
  QP_CHECK(qp_launch(qp, resid_fixed_kernel, dim3(256), b256, 0, nf, d.tf, d.zf, d.scal));
  // ATy -> rhs (scratch)
  QP_CHECK(gemm(qp, K, Rf, 1.0, d.Ft, d.yf, 0.0, d.rhs));
  if (qp->nW > 0) {
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0, d.x, 0.0, d.HQ + nx));
    QP_CHECK(qp_launch(qp, qp->D == 2 ? resid_rows_kernel<2> : resid_rows_kernel<3>, row_blocks(qp->nW), b256, 0, qp->nW, C,
                       d.w_k, d.w_i, d.w_j, d.w_eta, d.HQ + nx, d.zc, d.scal));
    QP_CHECK(row_scatter<ROW_Y>(qp, nullptr));
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0t, d.G, 1.0, d.rhs));
  }
  QP_CHECK(qp_launch(qp, resid_dual_kernel, dim3(128), b256, 0, nx, d.x, d.rhs, d.scal));
  SCP_HIP_CHECK(ctx, hipMemcpyAsync(qp->h_scal, d.scal, SL_COUNT * sizeof(double), hipMemcpyDeviceToHost, s));
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return SCP_OK;
}

int scp_qp_generic_certificate_atdy(scp_qp* qp) {
  const QpDev& d = qp->d;
  scp_ctx* ctx = qp->ctx;
  hipStream_t s = ctx->stream;
  const int K = qp->K, Rf = qp->Rf;
  const int64_t nx = (int64_t)K * qp->C;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(d.scal + SL_NATDY, 0, sizeof(double), s));
  QP_CHECK(gemm(qp, K, Rf, 1.0, d.Ft, d.dyf, 0.0, d.rhs));
  if (qp->nW > 0) {
    QP_CHECK(row_scatter<ROW_VEC>(qp, nullptr, d.dyc));
    QP_CHECK(gemm(qp, K, K, 1.0, d.S0t, d.G, 1.0, d.rhs));
  }
  QP_CHECK(qp_launch(qp, max_abs_kernel, dim3(128), dim3(256), 0, nx, d.rhs, d.scal + SL_NATDY));
  SCP_HIP_CHECK(ctx, hipMemcpyAsync(qp->h_scal + SL_NATDY, d.scal + SL_NATDY, sizeof(double), hipMemcpyDeviceToHost, s));
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return SCP_OK;
}

int scp_qp_exact_qx(scp_qp* qp, bool with_fx) {
  if (qp->dv.qx) return SCP_OK;
  QP_CHECK(gemm(qp, qp->K, qp->K, 1.0, qp->d.S0, qp->d.x, 0.0, qp->d.HQ + (int64_t)qp->K * qp->C));
  if (with_fx) QP_CHECK(gemm(qp, qp->Rf, qp->K, 1.0, qp->d.F, qp->d.x, 0.0, qp->d.fx));
  qp_on_qx_built(qp, with_fx);
  return SCP_OK;
}
