// The working rows of the joint QP (the collision rows A_W x >= l_W) and their incidence lists.  A_W is never formed:
// row n = (k, i, j) acts on (S0 x_i)[k] - (S0 x_j)[k], and A_W^T g is a gather over the row entries of every (time step,
// agent) cell, sorted inside the cell: a fixed summation order without atomics.  This file owns the kernels that append
// rows, build the lists (six launches; one workgroup for small problems, also fused with the recomputation of new rows
// and with the reset of a QP), write row values into the entries and gather them, and the host entries of all of these.
#include "scp_qp_device.h"
#include "scp_pair_device.h"
#include "scp_reset_device.h"

#include <algorithm>

// append working rows: decode (k, i, j), copy eta / l, z = max(A x, l), y = 0
// eta_stride == 0: eta_in / l_in are the gathered [n][D] / [n] arrays of scp_gather_rows; otherwise they are the arrays of
// the pairwise pass itself (pair range [q_begin, q_begin + nq)) and the gather happens here.
__global__ __launch_bounds__(256) void add_rows_kernel(int N, int D, int64_t C, int64_t pairs, int64_t base, int64_t n,
                                                        const int64_t* __restrict__ rows,
                                                        const double* __restrict__ eta_in,
                                                        const double* __restrict__ l_in, int64_t eta_stride,
                                                        int64_t q_begin, int64_t nq, const double* __restrict__ Q,
                                                        int64_t* __restrict__ w_row, int* __restrict__ wk,
                                                        int* __restrict__ wi, int* __restrict__ wj,
                                                        double* __restrict__ weta, double* __restrict__ wl,
                                                        double* __restrict__ zc, double* __restrict__ yc) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t r = rows[t];
  const int64_t k = r / pairs, q = r % pairs;
  // lexicographic pair index -> (i, j)
  const double b = 2.0 * N - 1.0;
  int64_t ii = (int64_t)((b - sqrt(b * b - 8.0 * (double)q)) * 0.5);
  if (ii < 0) ii = 0;
  if (ii > N - 2) ii = N - 2;
  while (ii * (2LL * N - ii - 1) / 2 > q) --ii;
  while (ii < N - 2 && (ii + 1) * (2LL * N - ii - 2) / 2 <= q) ++ii;
  const int64_t jj = q - ii * (2LL * N - ii - 1) / 2 + ii + 1;
  const int64_t o = base + t;
  w_row[o] = r;
  wk[o] = (int)k;
  wi[o] = (int)ii;
  wj[o] = (int)jj;
  const int64_t lr = k * nq + (q - q_begin);
  double ax = 0.0;
  for (int d = 0; d < D; ++d) {
    const double e = eta_stride ? eta_in[(int64_t)d * eta_stride + lr] : eta_in[t * D + d];
    weta[o * D + d] = e;
    ax += e * (Q[k * C + ii * D + d] - Q[k * C + jj * D + d]);
  }
  const double lo = eta_stride ? l_in[lr] : l_in[t];
  wl[o] = lo;
  zc[o] = fmax(ax, lo);
  yc[o] = 0.0;
}

namespace {

using namespace scpdev;

// row values g written to BOTH incidence-list entries of a row (pos_i, pos_j); the per-cell gathers then need no atomics:
//   INIT: g = (rho zc - yc) - rho eta.(Q_i - Q_j)   right-hand side minus the collision part of H x (Q = S0 x); also the
//         first row values of the single-step pipeline after (x, zc, yc, rho) changed outside it
//   else: g = rho eta.(Q_i - Q_j)                   collision part of H v (Q = S0 v)
template <int D, bool INIT>
__global__ __launch_bounds__(256) void rows_value_kernel(int64_t nW, int64_t C, double rho, const int* __restrict__ wk,
                                                          const int* __restrict__ wi, const int* __restrict__ wj,
                                                          const double* __restrict__ weta, const double* __restrict__ Q,
                                                          const double* __restrict__ zc, const double* __restrict__ yc,
                                                          const int* __restrict__ pos_i, const int* __restrict__ pos_j,
                                                          double* __restrict__ gval) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= nW) return;
  const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
  const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
  double ax = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) ax += weta[n * D + d] * (Q[bi + d] - Q[bj + d]);
  const double g = INIT ? (rho * zc[n] - yc[n]) - rho * ax : rho * ax;
  gval[pos_i[n]] = g;
  gval[pos_j[n]] = g;
}

constexpr int CSR1_MAX_CELLS = 16384;
constexpr int64_t CSR1_MAX_ROWS = 1 << 18;
// rows [base, base + n) that the kernel recomputes from the linearisation point first (scp_qp_add_rows_at); n = 0: none
struct CsrNewRows {
  int64_t n, base;
  const int64_t* rows;
  const double *pos_prev, *p0, *v0;
  double R, h;
  int N;
  int64_t* w_row;
  double* wl;
};

// =====================================================================================================
// Incidence lists of the working rows per (time step, agent) cell: the deterministic replacement of the atomic
// row scatter.  Built once per change of the working set (count, scan, fill, sort inside the cells, finish).
// =====================================================================================================
__global__ __launch_bounds__(256) void csr_count_kernel(int64_t nW, int K, const int* __restrict__ wk,
                                                         const int* __restrict__ wi, const int* __restrict__ wj,
                                                         int* __restrict__ cnt) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= nW) return;
  atomicAdd(cnt + cell_of(wk[n], wi[n], K), 1);  // integer counts: order independent
  atomicAdd(cnt + cell_of(wk[n], wj[n], K), 1);
}

// exclusive scan of cnt[0..ncell) into ptr (in place: cnt and ptr are the same array), cursors = ptr.  Two launches that
// fill the chip instead of one workgroup walking the array (67 us at N K = 51 200, a fortieth of the benchmark step):
// (1) every workgroup scans its own 4096 cells and leaves their total, (2) every workgroup adds the totals before it.
constexpr int SCAN_SC = 16;                 // consecutive cells per thread
constexpr int SCAN_CELLS = 256 * SCAN_SC;   // per workgroup
__global__ __launch_bounds__(256) void csr_scan_local_kernel(int ncell, int* __restrict__ ptr, int* __restrict__ blk_tot) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SCAN_CELLS + SCAN_SC * (int)threadIdx.x;
  int v[SCAN_SC], tot = 0;
#pragma unroll
  for (int e = 0; e < SCAN_SC; ++e) {
    v[e] = c + e < ncell ? ptr[c + e] : 0;
    tot += v[e];
  }
  int incl = tot;
  incl += dpp_move<0x111, 0xF, false>(incl);
  incl += dpp_move<0x112, 0xF, false>(incl);
  incl += dpp_move<0x114, 0xF, false>(incl);
  incl += dpp_move<0x118, 0xF, false>(incl);
  incl += dpp_move<0x142, 0xA, false>(incl);
  incl += dpp_move<0x143, 0xC, false>(incl);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int run = incl - tot;
  for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
  for (int e = 0; e < SCAN_SC; ++e) {
    if (c + e < ncell) ptr[c + e] = run;
    run += v[e];
  }
  if (threadIdx.x == 255) blk_tot[blockIdx.x] = run;
}

__global__ __launch_bounds__(256) void csr_scan_add_kernel(int ncell, int nblk, int* __restrict__ ptr, int* __restrict__ cur,
                                                            const int* __restrict__ blk_tot) {
  int off = 0;
  for (int b = 0; b < (int)blockIdx.x; ++b) off += blk_tot[b];  // (wave-uniform: scalar loads)
  const int c = blockIdx.x * SCAN_CELLS + SCAN_SC * (int)threadIdx.x;
#pragma unroll
  for (int e = 0; e < SCAN_SC; ++e) {
    if (c + e < ncell) {
      const int v = ptr[c + e] + off;
      ptr[c + e] = v;
      cur[c + e] = v;
    }
  }
  if (blockIdx.x == nblk - 1 && threadIdx.x == 0) ptr[ncell] = off + blk_tot[nblk - 1];
}

__global__ __launch_bounds__(256) void csr_fill_kernel(int64_t nW, int K, const int* __restrict__ wk,
                                                        const int* __restrict__ wi, const int* __restrict__ wj,
                                                        int* __restrict__ cur, int* __restrict__ ent) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= nW) return;
  ent[atomicAdd(cur + cell_of(wk[n], wi[n], K), 1)] = (int)(2 * n);
  ent[atomicAdd(cur + cell_of(wk[n], wj[n], K), 1)] = (int)(2 * n + 1);
}

// entries of a cell arrive in atomic order: sort them (ascending code) so that every sum has a fixed order
__global__ __launch_bounds__(256) void csr_sort_kernel(int ncell, const int* __restrict__ ptr, int* __restrict__ ent) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncell) return;
  const int b = ptr[c], e = ptr[c + 1];
  for (int i = b + 1; i < e; ++i) {
    const int v = ent[i];
    int j = i - 1;
    while (j >= b && ent[j] > v) {
      ent[j + 1] = ent[j];
      --j;
    }
    ent[j + 1] = v;
  }
}

__global__ __launch_bounds__(256) void csr_finish_kernel(int64_t nent, int D, const int* __restrict__ ent,
                                                          const double* __restrict__ weta, double* __restrict__ coef,
                                                          int* __restrict__ pos_i, int* __restrict__ pos_j) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nent) return;
  const int code = ent[t];
  const int n = code >> 1, side = code & 1;
  for (int d = 0; d < D; ++d) coef[t * D + d] = side ? -weta[(int64_t)n * D + d] : weta[(int64_t)n * D + d];
  if (side) pos_j[n] = (int)t;
  else pos_i[n] = (int)t;
}

// Small problems (N K <= CSR1_MAX_CELLS cells, e.g. 128 agents x 50 steps): the whole build -- count, scan, fill, sort,
// finish -- and the first row values (rows_value_kernel<D, true>) in ONE workgroup; the cell counters live in LDS.  Same lists,
// same order as the five-launch build.
template <bool COH>
__device__ inline void csr_small_body(int* csr_cnt, int64_t nW, int K, int ncell, int D, int64_t C, double rho,
                                                          int* __restrict__ wk, int* __restrict__ wi,
                                                          int* __restrict__ wj, double* __restrict__ weta,
                                                          const double* __restrict__ Qx, double* __restrict__ zc,
                                                          double* __restrict__ yc, int* __restrict__ ptr,
                                                          int* __restrict__ ent, double* __restrict__ coef,
                                                          int* __restrict__ pos_i, int* __restrict__ pos_j,
                                                          double* __restrict__ gval, CsrNewRows nr) {
  // csr_cnt: [ncell] ints of LDS: counts, then exclusive offsets, then fill cursors (= end of each cell)
  __shared__ int wsum[16];
  constexpr int SC = CSR1_MAX_CELLS / 1024;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (nr.n > 0) {  // scp_qp_add_rows_at's kernel first: the new rows [base, base + n) from the linearisation point
    const int64_t pairs = (int64_t)nr.N * (nr.N - 1) / 2;
    for (int64_t t = tid; t < nr.n; t += 1024) {
      if (D == 2)
        add_row_at<2, COH>(t, nr.N, K, C, pairs, nr.base, nr.rows, nr.pos_prev, nr.p0, nr.v0, nr.R, nr.h, Qx, nr.w_row, wk, wi, wj,
                      weta, nr.wl, zc, yc);
      else
        add_row_at<3, COH>(t, nr.N, K, C, pairs, nr.base, nr.rows, nr.pos_prev, nr.p0, nr.v0, nr.R, nr.h, Qx, nr.w_row, wk, wi, wj,
                      weta, nr.wl, zc, yc);
    }
    __threadfence_block();
    __syncthreads();
  }
  for (int c = tid; c < ncell; c += 1024) csr_cnt[c] = 0;
  __syncthreads();
  for (int64_t n = tid; n < nW; n += 1024) {
    atomicAdd(&csr_cnt[cell_of(wk[n], wi[n], K)], 1);
    atomicAdd(&csr_cnt[cell_of(wk[n], wj[n], K)], 1);
  }
  __syncthreads();
  {  // exclusive scan, SC consecutive cells per thread
    int v[SC], tot = 0;
#pragma unroll
    for (int e = 0; e < SC; ++e) {
      v[e] = SC * tid + e < ncell ? csr_cnt[SC * tid + e] : 0;
      tot += v[e];
    }
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int run = incl - tot;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int e = 0; e < SC; ++e) {
      if (SC * tid + e < ncell) {
        csr_cnt[SC * tid + e] = run;
        ptr[SC * tid + e] = run;
      }
      run += v[e];
    }
    if (tid == 1023) ptr[ncell] = run;
  }
  __syncthreads();
  for (int64_t n = tid; n < nW; n += 1024) {
    ent[atomicAdd(&csr_cnt[cell_of(wk[n], wi[n], K)], 1)] = (int)(2 * n);
    ent[atomicAdd(&csr_cnt[cell_of(wk[n], wj[n], K)], 1)] = (int)(2 * n + 1);
  }
  __syncthreads();
  for (int c = tid; c < ncell; c += 1024) {  // the cursor of a cell now stands at its end = the next cell's begin
    const int b = c ? csr_cnt[c - 1] : 0, e = csr_cnt[c];
    for (int i = b + 1; i < e; ++i) {
      const int v = ent[i];
      int j = i - 1;
      while (j >= b && ent[j] > v) {
        ent[j + 1] = ent[j];
        --j;
      }
      ent[j + 1] = v;
    }
  }
  __syncthreads();
  for (int64_t t = tid; t < 2 * nW; t += 1024) {
    const int code = ent[t];
    const int n = code >> 1, side = code & 1;
    for (int d = 0; d < D; ++d) coef[t * D + d] = side ? -weta[(int64_t)n * D + d] : weta[(int64_t)n * D + d];
    if (side) pos_j[n] = (int)t;
    else pos_i[n] = (int)t;
  }
  __syncthreads();
  for (int64_t n = tid; n < nW; n += 1024) {  // rows_value_kernel<D, true>
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
    double ax = 0.0;
    for (int d = 0; d < D; ++d)
      ax += weta[n * D + d] * (COH ? load_coherent(Qx + bi + d) - load_coherent(Qx + bj + d) : Qx[bi + d] - Qx[bj + d]);
    const double g = (rho * zc[n] - yc[n]) - rho * ax;
    gval[pos_i[n]] = g;
    gval[pos_j[n]] = g;
  }
}

__global__ __launch_bounds__(1024) void csr_small_kernel(int64_t nW, int K, int ncell, int D, int64_t C, double rho,
                                                          int* __restrict__ wk, int* __restrict__ wi,
                                                          int* __restrict__ wj, double* __restrict__ weta,
                                                          const double* __restrict__ Qx, double* __restrict__ zc,
                                                          double* __restrict__ yc, int* __restrict__ ptr,
                                                          int* __restrict__ ent, double* __restrict__ coef,
                                                          int* __restrict__ pos_i, int* __restrict__ pos_j,
                                                          double* __restrict__ gval, CsrNewRows nr) {
  extern __shared__ int csr_cnt[];
  csr_small_body<false>(csr_cnt, nW, K, ncell, D, C, rho, wk, wi, wj, weta, Qx, zc, yc, ptr, ent, coef, pos_i, pos_j, gval, nr);
}

// scp_qp_reset AND the installation of the QP's first rows in ONE launch: every workgroup resets its 16 columns
// (qp_reset_body: its first 256 threads), S0 x written through; the LAST workgroup to finish (a ticket) then runs
// csr_small_body on all 1024 threads, reading S0 x past its L2.  Same values as the two launches.
struct ResetArgs {
  int N, Rf;
  const double *x0, *F, *S0;
  double *x, *zf, *fx, *yf;
};
__global__ __launch_bounds__(1024) void reset_install_kernel(ResetArgs ra, int64_t nW, int K, int ncell, int D, int64_t C,
                                                              double rho, int* __restrict__ wk, int* __restrict__ wi,
                                                              int* __restrict__ wj, double* __restrict__ weta,
                                                              double* __restrict__ Qx, double* __restrict__ zc,
                                                              double* __restrict__ yc, int* __restrict__ ptr,
                                                              int* __restrict__ ent, double* __restrict__ coef,
                                                              int* __restrict__ pos_i, int* __restrict__ pos_j,
                                                              double* __restrict__ gval, CsrNewRows nr,
                                                              unsigned* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) char ri_lds[];  // max([K][16] doubles, [ncell] ints)
  __shared__ int last_sh;
  qp_reset_body<true>(threadIdx.x, threadIdx.x < 256, reinterpret_cast<double*>(ri_lds), ra.N, K, D, ra.Rf, ra.x0, ra.F, ra.S0,
                      ra.x, ra.zf, ra.fx, Qx, ra.yf);
  wait_stores_performed();  // (S0 x, written through, is in place before the ticket is taken)
  __syncthreads();
  if (threadIdx.x == 0) last_sh = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (!last_sh) return;
  if (threadIdx.x == 0) *ticket = 0u;  // (the next launch on this stream starts after this kernel has ended)
  csr_small_body<true>(reinterpret_cast<int*>(ri_lds), nW, K, ncell, D, C, rho, wk, wi, wj, weta, Qx, zc, yc, ptr, ent, coef,
                       pos_i, pos_j, gval, nr);
}

// row values for the residual / certificate scatters
__global__ __launch_bounds__(256) void csr_rowval_kernel(int64_t nW, int mode, double rho, const double* __restrict__ zc,
                                                          const double* __restrict__ yc, const double* __restrict__ vec,
                                                          const int* __restrict__ pos_i, const int* __restrict__ pos_j,
                                                          double* __restrict__ gval, const double* __restrict__ vec2,
                                                          double* __restrict__ gval2) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= nW) return;
  if (gval2) {  // a second row vector for the same gather
    const double g2 = vec2[n];
    gval2[pos_i[n]] = g2;
    gval2[pos_j[n]] = g2;
  }
  const double g = mode == 0 ? rho * zc[n] - yc[n] : (mode == 1 ? yc[n] : vec[n]);
  gval[pos_i[n]] = g;
  gval[pos_j[n]] = g;
}

// G[k][col] = sum over the cell's entries of coef * gval
__global__ __launch_bounds__(256) void csr_gather_kernel(int K, int N, int D, const int* __restrict__ ptr,
                                                          const double* __restrict__ coef,
                                                          const double* __restrict__ gval, double* __restrict__ G) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t C = (int64_t)N * D;
  if (t >= C * K) return;
  const int k = (int)(t / C), col = (int)(t % C);
  const int agent = col / D, d = col - agent * D;
  const int cell = cell_of(k, agent, K);
  double acc = 0.0;
  const int t1 = ptr[cell + 1];
  for (int e = ptr[cell]; e < t1; ++e) acc += coef[(size_t)e * D + d] * gval[e];
  G[t] = acc;
}

// csr_small_kernel on all nW rows; nr: the rows among them that it recomputes first
int launch_csr_small(scp_qp* qp, int64_t nW, double rho_c, const double* Qx, const CsrNewRows& nr) {
  const QpDev& d = qp->d;
  const int ncell = qp->N * qp->K;
  return qp_launch(qp, csr_small_kernel, dim3(1), dim3(1024), (size_t)ncell * sizeof(int), nW, qp->K, ncell, qp->D, qp->C, rho_c,
                   d.w_k, d.w_i, d.w_j, d.w_eta, Qx, d.zc, d.yc, d.cell_ptr, d.ent_code, d.coef, d.pos_i, d.pos_j, d.gval, nr);
}

// the per-cell gather of gval into the G slab
int launch_gather(scp_qp* qp) {
  const QpDev& d = qp->d;
  return qp_launch(qp, csr_gather_kernel, grid1((int64_t)qp->K * qp->C), dim3(256), 0, qp->K, qp->N, qp->D, d.cell_ptr, d.coef,
                   d.gval, d.G);
}

}  // namespace

int scp_qp_append_rows(scp_qp* qp, int64_t n, const int64_t* rows, const double* eta, const double* l, int64_t eta_stride,
                       int64_t q_begin, int64_t nq, const double* Qx) {
  const QpDev& d = qp->d;
  return qp_launch(qp, add_rows_kernel, grid1(n), dim3(256), 0, qp->N, qp->D, qp->C, scp_pairs(qp->N), qp->nW, n, rows, eta, l,
                   eta_stride, q_begin, nq, Qx, d.w_row, d.w_k, d.w_i, d.w_j, d.w_eta, d.w_l, d.zc, d.yc);
}

int scp_qp_rows_first_values(scp_qp* qp, const double* Qx) {
  const QpDev& d = qp->d;
  const double rho_c = qp->rho * qp->st.rho_col_scale;
  if (qp->dv.vals_rho_c == rho_c) return SCP_OK;  // scp_qp_install_rows_small built lists and values already
  if (!qp->dv.lists && qp->nW > 0 && qp->nW <= CSR1_MAX_ROWS && qp->N * qp->K <= CSR1_MAX_CELLS)
    return launch_csr_small(qp, qp->nW, rho_c, Qx, CsrNewRows{});
  QP_CHECK(scp_qp_csr_ensure(qp));
  return qp_launch(qp, qp->D == 2 ? rows_value_kernel<2, true> : rows_value_kernel<3, true>, grid1(qp->nW), dim3(256), 0,
                   qp->nW, qp->C, rho_c, d.w_k, d.w_i, d.w_j, d.w_eta, Qx, d.zc, d.yc, d.pos_i, d.pos_j, d.gval);
}

int scp_qp_install_rows_small(scp_qp* qp, int64_t n, const int64_t* rows, const double* pos_prev, const double* p0,
                              const double* v0, double R, const double* Qx, bool* done) {
  *done = false;
  const QpDev& d = qp->d;
  const int64_t nW = qp->nW + n;
  if (!qp->dv.qx || n <= 0 || nW > CSR1_MAX_ROWS || qp->N * qp->K > CSR1_MAX_CELLS) return SCP_OK;
  const CsrNewRows nr{n, qp->nW, rows, pos_prev, p0, v0, R, qp->h, qp->N, d.w_row, d.w_l};
  QP_CHECK(launch_csr_small(qp, nW, qp->rho * qp->st.rho_col_scale, Qx, nr));
  *done = true;
  return SCP_OK;
}

// qp->rho is the QP's starting value
int scp_qp_reset_install_small(scp_qp* qp, const double* x0, int64_t n, const int64_t* rows, const double* pos_prev,
                               const double* p0, const double* v0, double R, double* Qx, bool* done) {
  *done = false;
  const QpDev& d = qp->d;
  const int K = qp->K;
  if (n <= 0 || n > CSR1_MAX_ROWS || qp->N * K > CSR1_MAX_CELLS) return SCP_OK;
  const int ncell = qp->N * K;
  const double rho_c = qp->rho * qp->st.rho_col_scale;
  const size_t lds = std::max((size_t)K * RESET_COLS * sizeof(double), (size_t)ncell * sizeof(int));
  const CsrNewRows nr{n, 0, rows, pos_prev, p0, v0, R, qp->h, qp->N, d.w_row, d.w_l};
  const ResetArgs ra{qp->N, qp->Rf, x0, d.F, d.S0, d.x, d.zf, d.fx, d.yf};
  QP_CHECK(qp_launch(qp, reset_install_kernel, dim3((unsigned)scp_cdiv(qp->C, RESET_COLS)), dim3(1024), lds, ra, n, K, ncell,
                     qp->D, qp->C, rho_c, d.w_k, d.w_i, d.w_j, d.w_eta, Qx, d.zc, d.yc, d.cell_ptr, d.ent_code, d.coef, d.pos_i,
                     d.pos_j, d.gval, nr, qp->ctx->d_ticket + 2));  // ([0], [1]: the passes, the checks)
  *done = true;
  return SCP_OK;
}

int scp_qp_csr_ensure(scp_qp* qp) {
  if (qp->dv.lists) return SCP_OK;
  const QpDev& d = qp->d;
  const int ncell = qp->N * qp->K;
  SCP_REQUIRE(qp->ctx, 2 * qp->nW < 0x3FFFFFFF, "csr_build: too many working rows for 32-bit entry codes");
  SCP_HIP_CHECK(qp->ctx, hipMemsetAsync(d.cell_ptr, 0, (size_t)(ncell + 1) * sizeof(int), qp->ctx->stream));
  if (qp->nW > 0) {
    const dim3 rgrid = grid1(qp->nW), b256(256);
    const int sblk = (ncell + SCAN_CELLS - 1) / SCAN_CELLS;
    QP_CHECK(qp_launch(qp, csr_count_kernel, rgrid, b256, 0, qp->nW, qp->K, d.w_k, d.w_i, d.w_j, d.cell_ptr));
    QP_CHECK(qp_launch(qp, csr_scan_local_kernel, dim3(sblk), b256, 0, ncell, d.cell_ptr, d.scan_tot));
    QP_CHECK(qp_launch(qp, csr_scan_add_kernel, dim3(sblk), b256, 0, ncell, sblk, d.cell_ptr, d.cell_cur, d.scan_tot));
    QP_CHECK(qp_launch(qp, csr_fill_kernel, rgrid, b256, 0, qp->nW, qp->K, d.w_k, d.w_i, d.w_j, d.cell_cur, d.ent_code));
    QP_CHECK(qp_launch(qp, csr_sort_kernel, grid1(ncell), b256, 0, ncell, d.cell_ptr, d.ent_code));
    QP_CHECK(qp_launch(qp, csr_finish_kernel, grid1(2 * qp->nW), b256, 0, 2 * qp->nW, qp->D, d.ent_code, d.w_eta, d.coef, d.pos_i,
                       d.pos_j));
  }
  qp_on_lists_built(qp);
  return SCP_OK;
}

int scp_qp_csr_scatter(scp_qp* qp, int mode, const double* vec) {
  QP_CHECK(scp_qp_csr_ensure(qp));
  const QpDev& d = qp->d;
  QP_CHECK(qp_launch(qp, csr_rowval_kernel, grid1(qp->nW), dim3(256), 0, qp->nW, mode, qp->rho * qp->st.rho_col_scale, d.zc, d.yc,
                     vec, d.pos_i, d.pos_j, d.gval, nullptr, nullptr));
  return launch_gather(qp);
}

int scp_qp_rows_values_to_entries(scp_qp* qp) {
  const QpDev& d = qp->d;
  QP_CHECK(scp_qp_csr_ensure(qp));
  QP_CHECK(qp_launch(qp, csr_rowval_kernel, grid1(qp->nW), dim3(256), 0, qp->nW, 2, 0.0, d.zc, d.yc, d.grow, d.pos_i, d.pos_j,
                     d.gval, nullptr, nullptr));
  qp_on_vals_to_entries(qp);
  return SCP_OK;
}

int scp_qp_rows_check_values(scp_qp* qp, bool with_dy) {
  const QpDev& d = qp->d;
  return qp_launch(qp, csr_rowval_kernel, grid1(qp->nW), dim3(256), 0, qp->nW, 1, 0.0, d.zc, d.yc, nullptr, d.pos_i, d.pos_j,
                   d.gval2, with_dy ? d.dyc : nullptr, with_dy ? d.gval3 : nullptr);
}

int scp_qp_rows_gather(scp_qp* qp, const double* Q) {
  const QpDev& d = qp->d;
  QP_CHECK(scp_qp_csr_ensure(qp));
  QP_CHECK(qp_launch(qp, qp->D == 2 ? rows_value_kernel<2, false> : rows_value_kernel<3, false>, grid1(qp->nW), dim3(256), 0,
                     qp->nW, qp->C, qp->rho * qp->st.rho_col_scale, d.w_k, d.w_i, d.w_j, d.w_eta, Q, d.zc, d.yc, d.pos_i,
                     d.pos_j, d.gval));
  return launch_gather(qp);
}
