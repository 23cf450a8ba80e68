// Column-block kernels of the joint QP (use_mfma = 1) and what launches them: the three launches of the single-step
// pipeline (K <= SCP_FUSED_MAX_K with 16 columns per workgroup, K <= SCP_BIGK_MAX_K with one workgroup per column), QP#0's
// column-local kernel and the fused termination check with its host reduction.
//
// Every operation of an ADMM step except the working-row gather/scatter is local to a column c = (agent, axis):
// the fixed rows, the K x K KKT block and the Toeplitz block S0 act along the time index only.
// One workgroup (16 waves) therefore owns 16 columns and keeps their K-vectors in LDS: F, F^T, S0 and S0^T are
// jerk stencils and cumulative sums (wave-wide scans), and the only dense product left, H_f^{-1}, runs on the fp64
// matrix cores (v_mfma_f64_16x16x4_f64, operand pre-packed in lane order by scp_qp_kkt.hip).  Kernel boundaries
// remain only where the algorithm needs the whole grid: the inner products and the row gather/scatter (scp_qp_rows.hip).
// cg_iters > 1 and use_mfma = 0 / 2 run on the generic pipeline of scp_qp_generic.hip (one product per launch).
// The blocks the kernels here share are in scp_qp_device.h: column_At (A^T v by reverse scans), column_forward (F p and
// S0 p by forward scans), admm_project (projection and dual update of a row).
#include "scp_qp_device.h"

namespace {

using namespace scpdev;
constexpr int FT = 1024;       // threads per workgroup (16 waves: one 16-row output tile per wave in most products)
constexpr int NWV = FT / 64;

// Developer build (make prof -> libscp_hip_prof.so): wall-clock stamps (100 MHz) of one workgroup's phases.
#ifdef SCP_PHASE_PROFILE
__device__ unsigned long long scp_phase_clk[64];
#define PHASE_MARK(slot)                                                                      \
  do {                                                                                        \
    if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) scp_phase_clk[slot] = wall_clock64(); \
  } while (0)
#else
#define PHASE_MARK(slot) ((void)0)
#endif

// =====================================================================================================
// Single-PCG-step pipeline (settings.cg_iters == 1, the default): 3 launches per ADMM step.
//
//   x~ = x + a p,  p = Minv r,  r = rhs - H x,  a = (r.p) / (p.H p),   p.H p = r.p + rho sum_rows (eta.dQp)^2
//
// (H_f p = r), so neither H p nor a second scatter is needed.  The slabs Qx = S0 x and Fx = F x are carried:
// x+ = x + alpha a p gives Qx+ = Qx + alpha a Qp, Fx+ = Fx + alpha a Fp (refreshed exactly at every termination
// check), which turns r into -2 x + F^T(rho w (z_f - Fx) - y_f) + S0^T G and everything after a into elementwise work:
//   cg1_col_kernel    : r (wave scans), p = Minv r (MFMA), Qp = S0 p, Fp = F p (wave scans), partials r.p
//   cg1_rows_sq_kernel: partials rho (eta.dQp)^2
//   cg1_update_kernel : a; fixed rows' z, y, Fx+; x+, Qx+ (other buffer); collision rows' z, y and the row values
//                       g = rho zc - yc - rho eta.dQx+ of the next right-hand side (gathered by cg1_col_kernel)
// =====================================================================================================
constexpr int SQ_BLOCKS = 128;
// Column kernel of the single-step pipeline (launch 1 of 3).  With F x carried like S0 x,
//   r = sigma x + A^T(rho z - y) - H x = -2 x + F^T W' + S0^T G,   W' = rho w (z_f - F x) - y_f,
// (H_f = (2 + sigma) I + rho F^T w F), then p = H_f^{-1} r, S0 p, F p.  F^T W' + S0^T G and S0 p, F p cost wave-wide
// scans instead of dense products: the only matrix left is H_f^{-1} (the KKT solve, MFMA).  This kernel spells out what
// column_At (with - 2 x folded in) and column_forward of scp_qp_device.h state, and the tile product of qp0_col_kernel:
// called from helpers each came out slower here (profiles/column_blocks_device_code.md, section 4).
// Streaming the dense blocks (220 KB per workgroup for 16 columns) from L2 was 7 us of this kernel's 16.
// One wave per column for the scans (E time steps per lane), waves [0, ceil(K/16)) for the MFMA tiles.
template <int E>
__global__ __launch_bounds__(FT) void cg1_col_kernel(int K, int Rf, int64_t C, double rho, double h,
                                                      const double* __restrict__ pMinv, const double* __restrict__ wrow,
                                                      const double* __restrict__ x, const double* __restrict__ Fx,
                                                      const double* __restrict__ zf, const double* __restrict__ yf, int N,
                                                      int D, const int* __restrict__ cell_ptr,
                                                      const double* __restrict__ coef, const double* __restrict__ gval,
                                                      double* __restrict__ p, double* __restrict__ Qp,
                                                      double* __restrict__ Fp, double* __restrict__ part_rz) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double s_rz[NWV];
  const int RSF = pad_col(Rf), RSK = pad_col(K);
  double* Wt = lds;              // [16][RSF]  W', later F p
  double* Gx = Wt + CB * RSF;    // [16][RSK]  gather of eta * g
  double* Xt = Gx + CB * RSK;    // [16][RSK]  x
  double* Rt = Xt + CB * RSK;    // [16][RSK]  r
  double* Pt = Rt + CB * RSK;    // [16][RSK]  p
  double* Qt = Pt + CB * RSK;    // [16][RSK]  S0 p
  const int64_t c0 = (int64_t)blockIdx.x * CB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tK = (K + 15) >> 4, nks = (K + 3) >> 2;
  const double hh = h * h;
  PHASE_MARK(0);
  // ---- prologue: every global load is issued before the first use --------------------------------------------
  constexpr int WU = 4;  // slab rows per thread and pass: 64 WU >= Rf up to K = 64, a second pass beyond
  const int c = threadIdx.x & 15, kg = threadIdx.x >> 4;
  const bool cok = c0 + c < C;
  const int col = (int)(c0 + c), agent = col / D, dd = col - agent * D;
  // Issue order = return order: the incidence-list bounds first (the gather's second hop depends on them), then x and
  // the slab rows, then the H_f^{-1} operands; the dependent coef / gval loads follow while the rest is in flight.
  // (Measured: the prologue takes 4.1 us either way -- two round trips to data another XCD wrote in the last launch.)
  auto gather = [&](int k, double& xv) {  // incidence-list sum of one (time step, column); returns it, loads x
    int g0 = 0, g1 = 0;
    double acc = 0.0;
    xv = 0.0;
    if (cok && k < K) {
      g0 = cell_ptr[cell_of(k, agent, K)];
      g1 = cell_ptr[cell_of(k, agent, K) + 1];
      xv = x[(int64_t)k * C + c0 + c];
    }
    for (int t = g0; t < g1; ++t) acc += coef[(size_t)t * D + dd] * gval[t];
    return acc;
  };
  int g0 = 0, g1 = 0;
  double xv0 = 0.0;
  if (cok && kg < K) {
    g0 = cell_ptr[cell_of(kg, agent, K)];
    g1 = cell_ptr[cell_of(kg, agent, K) + 1];
    xv0 = x[(int64_t)kg * C + c0 + c];
  }
  double wz[WU], wf[WU], wy[WU];
#pragma unroll
  for (int u = 0; u < WU; ++u) {
    const int r = kg + u * (FT / CB);
    wz[u] = wf[u] = wy[u] = 0.0;
    if (cok && r < Rf) {
      const int64_t g = (int64_t)r * C + c0 + c;
      wz[u] = zf[g];
      wf[u] = Fx[g];
      wy[u] = yf[g];
    }
  }
  double aM[CHB];
  tile_prefetch<CHB>(pMinv, nks, wave < tK ? wave : 0, 0, nks, aM);
  {
    double acc = 0.0;
    for (int t = g0; t < g1; ++t) acc += coef[(size_t)t * D + dd] * gval[t];
    if (kg < K) {
      Gx[c * RSK + kg] = acc;
      Xt[c * RSK + kg] = xv0;
    }
  }
#pragma unroll
  for (int u = 0; u < WU; ++u) {
    const int r = kg + u * (FT / CB);
    if (r < Rf) Wt[c * RSF + r] = rho * wrow[r] * (wz[u] - wf[u]) - wy[u];
  }
  for (int k = kg + FT / CB; k < K; k += FT / CB) {  // K > 64
    double xv;
    const double acc = gather(k, xv);
    Gx[c * RSK + k] = acc;
    Xt[c * RSK + k] = xv;
  }
  for (int r = kg + WU * (FT / CB); r < Rf; r += FT / CB) {  // Rf > 256
    const int64_t g = (int64_t)r * C + c0 + c;
    Wt[c * RSF + r] = cok ? rho * wrow[r] * (zf[g] - Fx[g]) - yf[g] : 0.0;
  }
  __syncthreads();
  PHASE_MARK(1);
  // ---- r: one wave per column; index i = lane E + e runs over the time steps in DESCENDING order (k = KM - i), so the
  // reverse cumulative sums of the transposed integrator blocks are ascending scans over the lanes ----------------
  {
    const double* Wc = Wt + wave * RSF;
    const int KM = 64 * E - 1;
    double wj[E], wa[E], u1[E], u2[E], g[E], xk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = KM - (lane * E + e);
      const bool ok = k < K;
      wj[e] = k < K - 1 ? Wc[k] : 0.0;
      wa[e] = ok ? Wc[K - 1 + k] : 0.0;
      const double wv = ok ? Wc[2 * K - 1 + k] : 0.0;
      const double wp = ok ? Wc[3 * K - 1 + k] : 0.0;
      g[e] = ok ? Gx[wave * RSK + k] : 0.0;
      xk[e] = ok ? Xt[wave * RSK + k] : 0.0;
      u1[e] = h * wv + 0.5 * hh * (wp - g[e]);
      u2[e] = wp + g[e];
    }
    double d1[E], d2[E], s1[E], s2[E], wjp[E];
    wave_scan<E>(u1, d1, s1);   // d1 = rsum(u1)
    wave_scan<E>(u2, s1, s2);   // s1 = rsum(u2)
    wave_scan<E>(s1, s2, d2);   // d2 = rsum_excl(rsum(u2))
    wave_next<E>(wj, wjp);      // w_j[k - 1]
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = KM - (lane * E + e);
      const double rk = (((wjp[e] - wj[e]) / h + wa[e]) + (d1[e] + 0.5 * hh * g[e]) + hh * d2[e]) - 2.0 * xk[e];
      if (k < K) Rt[wave * RSK + k] = rk;
    }
  }
  __syncthreads();
  PHASE_MARK(2);
  // ---- p = H_f^{-1} r: one 16-row tile per wave -----------------------------------------------------------------
  for (int t = wave; t < tK; t += NWV) {
    const int li = lane & 15, lk = lane >> 4;
    const double* Ap = pMinv + (size_t)t * nks * 64 + lane;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < nks; kc += CHB) {
      if (kc > 0 || t != wave) {
#pragma unroll
        for (int s = 0; s < CHB; ++s) aM[s] = Ap[(size_t)min(kc + s, nks - 1) * 64];
      }
#pragma unroll
      for (int s = 0; s < CHB; ++s) {
        if (kc + s < nks) {  // wave-uniform
          const int kk = 4 * (kc + s) + lk;
          const double b = kk < K ? Rt[li * RSK + kk] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aM[s], b, acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = t * 16 + lk + 4 * r;
      if (row < K) Pt[li * RSK + row] = acc[r];
    }
  }
  __syncthreads();
  PHASE_MARK(3);
  // ---- S0 p, F p, r.p: one wave per column ------------------------------------------------------------------------
  {
    double* Wc = Wt + wave * RSF;
    double pk[E], c1[E], c2[E], t1[E], t2[E], c1p[E], pn[E];
    double rz = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = lane * E + e;
      pk[e] = k < K ? Pt[wave * RSK + k] : 0.0;
      rz += (k < K ? Rt[wave * RSK + k] : 0.0) * pk[e];
    }
    wave_scan<E>(pk, c1, t1);   // c1 = csum(p)
    wave_scan<E>(c1, t2, c2);   // c2 = csum_excl(csum(p))
    wave_prev<E>(c1, c1p);
    wave_next<E>(pk, pn);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = lane * E + e;
      if (k < K) {
        Qt[wave * RSK + k] = hh * (c2[e] - 0.5 * c1p[e]);
        if (k < K - 1) Wc[k] = (pn[e] - pk[e]) / h;
        Wc[K - 1 + k] = pk[e];
        Wc[2 * K - 1 + k] = h * c1[e];
        Wc[3 * K - 1 + k] = hh * (c2[e] + 0.5 * c1[e]);
      }
    }
    rz = wave_incl_sum(rz);
    if (lane == 63) s_rz[wave] = rz;
  }
  __syncthreads();
  PHASE_MARK(4);
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) t += s_rz[w];
    part_rz[blockIdx.x] = t;
  }
  // ---- coalesced stores ----------------------------------------------------------------------------------------------
  if (cok) {
    for (int k = kg; k < K; k += FT / CB) {
      const int64_t g = (int64_t)k * C + c0 + c;
      p[g] = Pt[c * RSK + k];
      Qp[g] = Qt[c * RSK + k];
    }
    for (int r = kg; r < Rf; r += FT / CB) Fp[(int64_t)r * C + c0 + c] = Wt[c * RSF + r];
  }
  PHASE_MARK(5);
}

// ---- the column kernel for long horizons (K > SCP_FUSED_MAX_K, up to 1024: the reference's demo runs K = 500) ------------
// Same quantities as cg1_col_kernel -- r by reverse cumulative sums, p = H_f^{-1} r, S0 p, F p by forward sums, r.p -- with
// ONE WORKGROUP PER COLUMN and one thread per time step: the sums are block-wide scans (wave scans on DPP + one LDS
// round for the wave totals), and H_f^{-1} (2 MB at K = 500, symmetric: thread k reads column k = row k, coalesced over
// the threads) is streamed from L2 by every column's workgroup instead of living in MFMA operand registers.  No LDS tiles
// of 4K-1 rows x 16 columns, so K is bounded by the thread count only.
__device__ inline double block_scan_incl(double v, bool reverse, double* wtot) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
  const double w = reverse ? wave_incl_rsum(v) : wave_incl_sum(v);
  if (lane == (reverse ? 0 : 63)) wtot[wave] = w;
  __syncthreads();
  double off = 0.0;
  if (reverse) {
    for (int q = nw - 1; q > wave; --q) off += wtot[q];
  } else {
    for (int q = 0; q < wave; ++q) off += wtot[q];
  }
  __syncthreads();
  return w + off;
}
// value of thread k + shift (0 outside [0, K)) through an LDS line
__device__ inline double block_shift(double v, int shift, int K, double* line) {
  const int k = threadIdx.x;
  if (k < K) line[k] = v;
  __syncthreads();
  const int src = k + shift;
  const double out = (k < K && src >= 0 && src < K) ? line[src] : 0.0;
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(1024) void cg1_colK_kernel(int K, int Rf, int64_t C, double rho, double h,
                                                         const double* __restrict__ Minv, const double* __restrict__ wrow,
                                                         const double* __restrict__ x, const double* __restrict__ Fx,
                                                         const double* __restrict__ zf, const double* __restrict__ yf, int N,
                                                         int D, const int* __restrict__ cell_ptr,
                                                         const double* __restrict__ coef, const double* __restrict__ gval,
                                                         double* __restrict__ p, double* __restrict__ Qp,
                                                         double* __restrict__ Fp, double* __restrict__ part_rz) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* rbuf = lds;        // [K] r
  double* line = rbuf + K;   // [K] neighbour shifts
  __shared__ double wtot[16];
  const int col = blockIdx.x, k = threadIdx.x;
  const bool live = k < K;
  const int agent = col / D, dd = col - agent * D;
  const double hh = h * h;
  double wj = 0.0, wa = 0.0, wv = 0.0, wp = 0.0, xk = 0.0, g = 0.0;
  if (live) {
    auto wprime = [&](int row) {
      const int64_t o = (int64_t)row * C + col;
      return rho * wrow[row] * (zf[o] - Fx[o]) - yf[o];
    };
    if (k < K - 1) wj = wprime(k);
    wa = wprime(K - 1 + k);
    wv = wprime(2 * K - 1 + k);
    wp = wprime(3 * K - 1 + k);
    xk = x[(int64_t)k * C + col];
    const int c0 = cell_ptr[cell_of(k, agent, K)], c1 = cell_ptr[cell_of(k, agent, K) + 1];
    for (int t = c0; t < c1; ++t) g += coef[(size_t)t * D + dd] * gval[t];
  }
  const double u1 = h * wv + 0.5 * hh * (wp - g);
  const double u2 = wp + g;
  const double d1 = block_scan_incl(u1, true, wtot);
  const double s1 = block_scan_incl(u2, true, wtot);
  const double d2 = block_shift(block_scan_incl(s1, true, wtot), +1, K, line);  // exclusive suffix sum
  const double wjm = block_shift(wj, -1, K, line);                               // w_j[k - 1]
  const double rk = (((wjm - wj) / h + wa) + (d1 + 0.5 * hh * g) + hh * d2) - 2.0 * xk;
  if (live) rbuf[k] = rk;
  __syncthreads();
  double pk = 0.0;
  if (live) {  // p_k = sum_m Minv[m][k] r_m  (Minv symmetric: column k read as the k-th entries of its rows -> coalesced)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int m = 0;
    for (; m + 4 <= K; m += 4) {
      a0 = fma(Minv[(size_t)m * K + k], rbuf[m], a0);
      a1 = fma(Minv[(size_t)(m + 1) * K + k], rbuf[m + 1], a1);
      a2 = fma(Minv[(size_t)(m + 2) * K + k], rbuf[m + 2], a2);
      a3 = fma(Minv[(size_t)(m + 3) * K + k], rbuf[m + 3], a3);
    }
    for (; m < K; ++m) a0 = fma(Minv[(size_t)m * K + k], rbuf[m], a0);
    pk = (a0 + a1) + (a2 + a3);
  }
  const double c1s = block_scan_incl(pk, false, wtot);                                // csum(p)
  const double c2s = block_shift(block_scan_incl(c1s, false, wtot), -1, K, line);     // csum_excl(csum(p))
  const double c1p = block_shift(c1s, -1, K, line);
  const double pn = block_shift(pk, +1, K, line);
  const double rz = block_scan_incl(live ? rk * pk : 0.0, false, wtot);  // total in the last thread
  if (live) {
    p[(int64_t)k * C + col] = pk;
    Qp[(int64_t)k * C + col] = hh * (c2s - 0.5 * c1p);
    if (k < K - 1) Fp[(int64_t)k * C + col] = (pn - pk) / h;
    Fp[(int64_t)(K - 1 + k) * C + col] = pk;
    Fp[(int64_t)(2 * K - 1 + k) * C + col] = h * c1s;
    Fp[(int64_t)(3 * K - 1 + k) * C + col] = hh * (c2s + 0.5 * c1s);
  }
  if (threadIdx.x == blockDim.x - 1) part_rz[col] = rz;
}

template <int D>
__global__ __launch_bounds__(256) void cg1_rows_sq_kernel(int64_t nW, int64_t C, double rho, const int* __restrict__ wk,
                                                           const int* __restrict__ wi, const int* __restrict__ wj,
                                                           const double* __restrict__ weta,
                                                           const double* __restrict__ Qp, double* __restrict__ part_sq) {
  __shared__ double sw[4];
  double acc = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nW; n += (int64_t)SQ_BLOCKS * 256) {
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
    double ax = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) ax += weta[n * D + d] * (Qp[bi + d] - Qp[bj + d]);
    acc += ax * ax;
  }
  acc = wave_incl_sum(acc);
  if ((threadIdx.x & 63) == 63) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part_sq[blockIdx.x] = rho * ((sw[0] + sw[1]) + (sw[2] + sw[3]));
}

// Fixed rows only (QP#0, or any solve before the first collision row joins): the whole ADMM iteration is column-local,
//   x~ = H_f^{-1} (sigma x + F^T(rho w z - y)),  z~ = F x~,  relaxation, projection, dual update,
// so ONE launch runs `nit` iterations (up to the next termination check) with z, y, l, u of a thread's slab rows in
// registers, x in LDS and the H_f^{-1} operands of a wave's tile resident in registers (K <= 64): four barriers and no
// global memory traffic per iteration, instead of two launches.
template <int E>
__global__ __launch_bounds__(FT) void qp0_col_kernel(int K, int Rf, int64_t C, double rho, double sigma, double alpha,
                                                      double h, int nit, const double* __restrict__ pMinv,
                                                      const double* __restrict__ wrow, const double* __restrict__ lf,
                                                      const double* __restrict__ uf, double* __restrict__ x,
                                                      double* __restrict__ zf, double* __restrict__ yf,
                                                      double* __restrict__ dy_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int RU = 4 * E;  // slab rows per thread: 64 RU >= Rf = 4K - 1 for K <= 64 E
  const int RSF = pad_col(Rf), RSK = pad_col(K);
  double* Wt = lds;              // [16][RSF]  rho w z - y, then F x~
  double* Xt = Wt + CB * RSF;    // [16][RSK]  x
  double* Rt = Xt + CB * RSK;    // [16][RSK]  right-hand side
  double* Pt = Rt + CB * RSK;    // [16][RSK]  x~
  const int64_t c0 = (int64_t)blockIdx.x * CB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = threadIdx.x & 15, kg = threadIdx.x >> 4;
  const bool cok = c0 + c < C;
  const int tK = (K + 15) >> 4, nks = (K + 3) >> 2;
  double aM[CHB];
  tile_prefetch<CHB>(pMinv, nks, wave < tK ? wave : 0, 0, nks, aM);
  double z[RU], y[RU], lo[RU], hi[RU], rw[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = kg + u * (FT / CB);
    z[u] = y[u] = lo[u] = hi[u] = 0.0;
    rw[u] = 1.0;
    if (cok && r < Rf) {
      const int64_t g = (int64_t)r * C + c0 + c;
      z[u] = zf[g]; y[u] = yf[g]; lo[u] = lf[g]; hi[u] = uf[g];
      rw[u] = rho * wrow[r];
    }
  }
  for (int k = kg; k < K; k += FT / CB) Xt[c * RSK + k] = cok ? x[(int64_t)k * C + c0 + c] : 0.0;
  for (int it = 0; it < nit; ++it) {
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int r = kg + u * (FT / CB);
      if (r < Rf) Wt[c * RSF + r] = rw[u] * z[u] - y[u];
    }
    __syncthreads();
    {  // right-hand side sigma x + F^T(rho w z - y)
      double xk[E], atw[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {  // read ahead of the scans: after them the LDS round trip is on the critical path
        const int k = (64 * E - 1) - (lane * E + e);
        xk[e] = k < K ? Xt[wave * RSK + k] : 0.0;
      }
      column_At<E, false>(K, h, Wt + wave * RSF, nullptr, atw);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int k = (64 * E - 1) - (lane * E + e);
        if (k < K) Rt[wave * RSK + k] = atw[e] + sigma * xk[e];
      }
    }
    __syncthreads();
    for (int t = wave; t < tK; t += NWV) {  // x~ = H_f^{-1} rhs
      const int li = lane & 15, lk = lane >> 4;
      const double* Ap = pMinv + (size_t)t * nks * 64 + lane;
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
      for (int kc = 0; kc < nks; kc += CHB) {
        if (nks > CHB || t != wave) {  // operands not resident (K > 64)
#pragma unroll
          for (int s_ = 0; s_ < CHB; ++s_) aM[s_] = Ap[(size_t)min(kc + s_, nks - 1) * 64];
        }
#pragma unroll
        for (int s_ = 0; s_ < CHB; ++s_) {
          if (kc + s_ < nks) {  // wave-uniform
            const int kk = 4 * (kc + s_) + lk;
            const double b = kk < K ? Rt[li * RSK + kk] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aM[s_], b, acc, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = t * 16 + lk + 4 * r;
        if (row < K) Pt[li * RSK + row] = acc[r];
      }
    }
    __syncthreads();
    {  // z~ = F x~, x+ = alpha x~ + (1 - alpha) x
      double pk[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int k = lane * E + e;
        pk[e] = k < K ? Pt[wave * RSK + k] : 0.0;
      }
      column_forward<E, false>(K, h, pk, Wt + wave * RSF, nullptr);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int k = lane * E + e;
        if (k < K) Xt[wave * RSK + k] = alpha * pk[e] + (1.0 - alpha) * Xt[wave * RSK + k];
      }
    }
    __syncthreads();
    const bool emit = dy_out != nullptr && it == nit - 1;  // delta-y of the last iteration (infeasibility certificate)
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int r = kg + u * (FT / CB);
      if (cok && r < Rf) {
        double zn, yn;
        admm_project(alpha * Wt[c * RSF + r] + (1.0 - alpha) * z[u], y[u], rw[u], lo[u], hi[u], zn, yn);
        if (emit) dy_out[(int64_t)r * C + c0 + c] = yn - y[u];
        y[u] = yn;
        z[u] = zn;
      }
    }
  }
  __syncthreads();
  if (cok) {
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int r = kg + u * (FT / CB);
      if (r < Rf) {
        const int64_t g = (int64_t)r * C + c0 + c;
        zf[g] = z[u];
        yf[g] = y[u];
      }
    }
    for (int k = kg; k < K; k += FT / CB) x[(int64_t)k * C + c0 + c] = Xt[c * RSK + k];
  }
}

// step length a = r.p / p.H p  from the per-workgroup partials (p.H_f p = p.r because p = H_f^{-1} r); the same
// instruction sequence in every 256-thread workgroup, so every workgroup holds the same bits
__device__ inline double step_length_256(const double* __restrict__ part_rz, int nblk, const double* __restrict__ part_sq) {
  __shared__ double sw[2][4];
  double v = 0.0, q = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) v += part_rz[b];
  for (int b = threadIdx.x; b < SQ_BLOCKS; b += 256) q += part_sq[b];
  v = wave_incl_sum(v);  // DPP: totals in lane 63 (an LDS-routed __shfl butterfly costs ten times as much)
  q = wave_incl_sum(q);
  if ((threadIdx.x & 63) == 63) {
    sw[0][threadIdx.x >> 6] = v;
    sw[1][threadIdx.x >> 6] = q;
  }
  __syncthreads();
  const double rz = (sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3]);
  const double pHp = rz + ((sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3]));
  return (pHp > 0.0 && rz != 0.0) ? rz / pHp : 0.0;
}

// The same step length with p.Hp's row term summed by the caller itself (every workgroup redundantly, in the same order
// -> the same bits): for small working sets (nW <= SQ_INLINE_MAX) this saves the cg1_rows_sq_kernel launch -- a third
// of an iteration's launches and ~5 us of its latency when a solve is launch bound (N <= ~256).
constexpr int SQ_INLINE_MAX = 2048;
template <int D>
__device__ inline double step_length_inline_256(const double* __restrict__ part_rz, int nblk, int64_t nW, int64_t C, double rho_c,
                                                const int* __restrict__ wk, const int* __restrict__ wi,
                                                const int* __restrict__ wj, const double* __restrict__ weta,
                                                const double* __restrict__ Qp) {
  __shared__ double sw[2][4];
  double v = 0.0, q = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) v += part_rz[b];
  for (int64_t n = threadIdx.x; n < nW; n += 256) {
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
    double ax = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) ax += weta[n * D + d] * (Qp[bi + d] - Qp[bj + d]);
    q += ax * ax;
  }
  v = wave_incl_sum(v);
  q = wave_incl_sum(q);
  if ((threadIdx.x & 63) == 63) {
    sw[0][threadIdx.x >> 6] = v;
    sw[1][threadIdx.x >> 6] = q;
  }
  __syncthreads();
  const double rz = (sw[0][0] + sw[0][1]) + (sw[0][2] + sw[0][3]);
  const double pHp = rz + rho_c * ((sw[1][0] + sw[1][1]) + (sw[1][2] + sw[1][3]));
  return (pHp > 0.0 && rz != 0.0) ? rz / pHp : 0.0;
}

constexpr int UPD_RPT = 2;  // slab rows per thread in the elementwise part of cg1_update_kernel (32 rows per workgroup)

// Launch 3 of 3: everything that follows the step length, elementwise.  Workgroups [0, eblocks): 32 slab
// rows of ONE 16-column block each -- fixed rows: F x~ = F x + a F p, z/y update, F x += alpha a F p; x rows:
// x += alpha a p, S0 x (new buffer) = S0 x + alpha a S0 p.  Workgroup w works on column block w % nblk8 (nblk8 =
// nblk rounded up to a multiple of 8): workgroups go round-robin over the 8 XCDs, so the slabs are rewritten in the L2
// of the XCD whose cg1_col_kernel workgroup reads them next (a row-major split left every read a remote miss: 8 us
// of load latency in the column kernel instead of 2.6).  Workgroups [eblocks, ...): collision rows -- S0 x~ and the
// new S0 x formed on the fly from (S0 x, S0 p) with the same fma, z/y update, then the row values of the NEXT
// right-hand side   g = rho zc - yc - rho eta.d(S0 x)      (A_W^T g is gathered by cg1_col_kernel).
template <int D>
__global__ __launch_bounds__(256) void cg1_update_kernel(int K, int Rf, int64_t C, int nblk, int npart, int eblocks, int nblk8, double rho,
                                                          double rho_c, double alpha, const double* __restrict__ part_rz,
                                                          const double* __restrict__ part_sq,
                                                          const double* __restrict__ wrow, const double* __restrict__ lf,
                                                          const double* __restrict__ uf, double* __restrict__ zf,
                                                          double* __restrict__ yf, double* __restrict__ Fx,
                                                          const double* __restrict__ Fp, double* __restrict__ x,
                                                          const double* __restrict__ pdir,
                                                          const double* __restrict__ Qp, const double* __restrict__ Qx,
                                                          double* __restrict__ Qn, int64_t nW, const int* __restrict__ wk,
                                                          const int* __restrict__ wi, const int* __restrict__ wj,
                                                          const double* __restrict__ weta, const double* __restrict__ wl,
                                                          double* __restrict__ zc, double* __restrict__ yc,
                                                          const int* __restrict__ pos_i, const int* __restrict__ pos_j,
                                                          double* __restrict__ gval, double* __restrict__ dyf,
                                                          double* __restrict__ dyc, int inline_sq) {
  // all operands are loaded BEFORE the step length is reduced (one memory round trip for both)
  if ((int)blockIdx.x < eblocks) {
    const int seg = blockIdx.x / nblk8, blk = blockIdx.x - seg * nblk8;
    const int64_t col = (int64_t)blk * CB + (threadIdx.x & 15);
    const bool live = blk < nblk && col < C;
    const int rows = Rf + K;
    double v0[UPD_RPT], v1[UPD_RPT], v2[UPD_RPT], v3[UPD_RPT], v4[UPD_RPT], v5[UPD_RPT], rr[UPD_RPT];
#pragma unroll
    for (int u = 0; u < UPD_RPT; ++u) {
      const int row = seg * (16 * UPD_RPT) + u * 16 + (threadIdx.x >> 4);
      v0[u] = v1[u] = v2[u] = v3[u] = v4[u] = v5[u] = 0.0;
      rr[u] = 1.0;
      if (live && row < Rf) {
        const int64_t g = (int64_t)row * C + col;
        v0[u] = Fx[g]; v1[u] = Fp[g]; v2[u] = zf[g]; v3[u] = yf[g]; v4[u] = lf[g]; v5[u] = uf[g];
        rr[u] = rho * wrow[row];
      } else if (live && row < rows) {
        const int64_t g = (int64_t)(row - Rf) * C + col;
        v0[u] = x[g]; v1[u] = pdir[g]; v2[u] = Qx[g]; v3[u] = Qp[g];
      }
    }
    const double a = inline_sq ? step_length_inline_256<D>(part_rz, npart, nW, C, rho_c, wk, wi, wj, weta, Qp)
                               : step_length_256(part_rz, npart, part_sq);
    const double aa = alpha * a;
    if (!live) return;
#pragma unroll
    for (int u = 0; u < UPD_RPT; ++u) {
      const int row = seg * (16 * UPD_RPT) + u * 16 + (threadIdx.x >> 4);
      if (row < Rf) {
        const int64_t g = (int64_t)row * C + col;
        const double y = v3[u];
        double zn, yn;
        admm_project(alpha * fma(a, v1[u], v0[u]) + (1.0 - alpha) * v2[u], y, rr[u], v4[u], v5[u], zn, yn);
        yf[g] = yn;
        zf[g] = zn;
        Fx[g] = fma(aa, v1[u], v0[u]);
        if (dyf) dyf[g] = yn - y;  // delta-y of this iteration (primal infeasibility certificate)
      } else if (row < rows) {
        const int64_t g = (int64_t)(row - Rf) * C + col;
        x[g] = fma(aa, v1[u], v0[u]);
        Qn[g] = fma(aa, v3[u], v2[u]);
      }
    }
    return;
  }
  const int64_t n = (int64_t)(blockIdx.x - eblocks) * 256 + threadIdx.x;
  const bool live = n < nW;
  double e[D], qi[D], qj[D], pi[D], pj[D], z = 0.0, y = 0.0, lo = 0.0;
  int posi = 0, posj = 0;
  if (live) {
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      e[d] = weta[n * D + d];
      qi[d] = Qx[bi + d]; qj[d] = Qx[bj + d]; pi[d] = Qp[bi + d]; pj[d] = Qp[bj + d];
    }
    z = zc[n]; y = yc[n]; lo = wl[n];
    posi = pos_i[n]; posj = pos_j[n];
  }
  const double a = inline_sq ? step_length_inline_256<D>(part_rz, npart, nW, C, rho_c, wk, wi, wj, weta, Qp)
                             : step_length_256(part_rz, npart, part_sq);
  const double aa = alpha * a;
  if (!live) return;
  double tc = 0.0, ax = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    tc += e[d] * (fma(a, pi[d], qi[d]) - fma(a, pj[d], qj[d]));
    ax += e[d] * (fma(aa, pi[d], qi[d]) - fma(aa, pj[d], qj[d]));
  }
  double zn, yn;
  admm_project(alpha * tc + (1.0 - alpha) * z, y, rho_c, lo, zn, yn);
  yc[n] = yn;
  zc[n] = zn;
  if (dyc) dyc[n] = fmin(yn - y, 0.0);  // u = +inf: projected onto the polar of the recession cone
  const double g = (rho_c * zn - yn) - rho_c * ax;
  gval[posi] = g;
  gval[posj] = g;
}

}  // namespace

// `nit` ADMM iterations on the fixed rows alone in one launch (qp->nW == 0); dy_out: where to leave delta-y of the last
// iteration for scp_qp_fused_residuals (NULL: not needed)
int scp_qp_qp0_iterations(scp_qp* qp, int nit, double* dy_out) {
  const QpDev& d = qp->d;
  const int K = qp->K, Rf = qp->Rf;
  const int nblk = (int)((qp->C + CB - 1) / CB);
  const size_t lds = (size_t)CB * (pad_col(Rf) + 3 * pad_col(K)) * sizeof(double);
  return qp_launch(qp, K <= 64 ? qp0_col_kernel<1> : qp0_col_kernel<2>, dim3(nblk), dim3(FT), lds, K, Rf, qp->C, qp->rho,
                   qp->st.sigma, qp->st.alpha, qp->h, nit, d.pMinv, d.wrow, d.lf, d.uf, d.x, d.zf, d.yf, dy_out);
}

int scp_qp_cg1_prepare(scp_qp* qp) {
  if (qp->dv.carried)  // (a persistent kernel with its own entry tables left the row values per row)
    return qp->dv.vals_by_row ? scp_qp_rows_values_to_entries(qp) : SCP_OK;
  QP_CHECK(scp_qp_exact_qx(qp, true));
  QP_CHECK(scp_qp_rows_first_values(qp, scp_qp_qx(qp)));
  qp_on_cg1_prepared(qp);
  return SCP_OK;
}

// One ADMM iteration with a single preconditioned CG step from x, in three launches: column blocks (r, then
// [p ; S0 p ; F p]), collision rows (p.H p), elementwise update of every row and column (ping-pong of S0 x).
int scp_qp_cg1_iteration(scp_qp* qp, int* cg_count, bool emit_dy) {
  const QpDev& d = qp->d;
  double* dyf = emit_dy ? d.dyf : nullptr;  // delta-y of this iteration, consumed by scp_qp_fused_residuals(.., 2)
  double* dyc = emit_dy ? d.dyc : nullptr;
  const int K = qp->K, Rf = qp->Rf;
  const int64_t C = qp->C;
  const int nblk = (int)((C + CB - 1) / CB);
  double* Qp = d.s0p;  // S0 p
  double* Fp = d.tf;   // F p
  double* part_rz = d.part;
  double* part_sq = d.part + SCP_PART_CAP / 2;
  const double rho_c = qp->rho * qp->st.rho_col_scale;
  QP_CHECK(scp_qp_cg1_prepare(qp));
  double* Qx = scp_qp_qx(qp);        // S0 x (carried)
  double* Qn = scp_qp_qx(qp, true);  // S0 x of the next iteration
  int npart = nblk;  // partial sums of r.p: one per column block, or one per column (long horizons)
  if (K > SCP_FUSED_MAX_K) {
    npart = (int)C;
    QP_CHECK(qp_launch(qp, cg1_colK_kernel, dim3((unsigned)C), dim3((unsigned)((K + 63) / 64 * 64)), (size_t)2 * K * sizeof(double),
                       K, Rf, C, qp->rho, qp->h, d.Minv, d.wrow, d.x, d.fx, d.zf, d.yf, qp->N, qp->D, d.cell_ptr, d.coef, d.gval,
                       d.p, Qp, Fp, part_rz));
  } else {
    const size_t lds = (size_t)CB * (pad_col(Rf) + 5 * pad_col(K)) * sizeof(double);
    QP_CHECK(qp_launch(qp, K <= 64 ? cg1_col_kernel<1> : cg1_col_kernel<2>, dim3(nblk), dim3(FT), lds, K, Rf, C, qp->rho, qp->h,
                       d.pMinv, d.wrow, d.x, d.fx, d.zf, d.yf, qp->N, qp->D, d.cell_ptr, d.coef, d.gval, d.p, Qp, Fp, part_rz));
  }
  const dim3 rblock(256);
  const int inline_sq = qp->nW <= SQ_INLINE_MAX ? 1 : 0;  // small working set: the update kernel sums p.Hp's row term itself
  if (!inline_sq)
    QP_CHECK(qp_launch(qp, qp->D == 2 ? cg1_rows_sq_kernel<2> : cg1_rows_sq_kernel<3>, dim3(SQ_BLOCKS), rblock, 0, qp->nW, C,
                       rho_c, d.w_k, d.w_i, d.w_j, d.w_eta, Qp, part_sq));
  const int nblk8 = (nblk + 7) & ~7;
  const int eblocks = nblk8 * ((Rf + K + 16 * UPD_RPT - 1) / (16 * UPD_RPT));
  const dim3 ugrid((unsigned)(eblocks + (qp->nW + 255) / 256));
  QP_CHECK(qp_launch(qp, qp->D == 2 ? cg1_update_kernel<2> : cg1_update_kernel<3>, ugrid, rblock, 0, K, Rf, C, nblk, npart,
                     eblocks, nblk8, qp->rho, rho_c, qp->st.alpha, part_rz, part_sq, d.wrow, d.lf, d.uf, d.zf, d.yf, d.fx, Fp,
                     d.x, d.p, Qp, Qx, Qn, qp->nW, d.w_k, d.w_i, d.w_j, d.w_eta, d.w_l, d.zc, d.yc, d.pos_i, d.pos_j, d.gval,
                     dyf, dyc, inline_sq));
  qp_on_cg1_step(qp);
  ++*cg_count;
  return SCP_OK;
}

// =====================================================================================================
// Termination check of the single-step pipeline, fused: one row launch (gval = yc), one column-block launch
// (F x, S0 x, A^T y = F^T y_f + S0^T gather, delta-y of the fixed rows, all their maxima), one row launch
// (collision rows' residuals and delta-y).  14 launches on the generic path.
// =====================================================================================================
namespace {

// per-workgroup partial results of a check: [rp, |Ax|, |z|, rd, |Px|, |A^T y|, |dy|, supp, |A^T dy|] (maxima / a sum),
// reduced on the host -- 7 same-address atomics per workgroup cost more than the rest of the kernel
constexpr int RS_RP = 0, RS_NAX = 1, RS_NZ = 2, RS_RD = 3, RS_NPX = 4, RS_NATY = 5, RS_NDY = 6, RS_SUPP = 7, RS_NATDY = 8;

// Column part of the check, with the integrator blocks as wave scans like cg1_col_kernel (one wave per column):
//   F x, S0 x (stored: the pipeline's carried slabs are refreshed exactly), A^T y = F^T y_f + S0^T G(yc), the maxima of
//   the primal / dual residuals over this block's 16 columns and, with_dy (dyf / gval2 hold delta-y of the last
//   iteration), |dy|, its support value and |A^T dy| of OSQP's primal infeasibility certificate.
template <int E>
__global__ __launch_bounds__(FT) void cg1_resid_col_kernel(int K, int Rf, int64_t C, double h, int N, int D, int with_dy,
                                                            int has_rows, const double* __restrict__ x, const double* __restrict__ zf,
                                                            const double* __restrict__ yf, const double* __restrict__ lf,
                                                            const double* __restrict__ uf, const double* __restrict__ dyf,
                                                            const int* __restrict__ cell_ptr,
                                                            const double* __restrict__ coef,
                                                            const double* __restrict__ gval,
                                                            const double* __restrict__ gval2, double* __restrict__ Qx,
                                                            double* __restrict__ Fx, double* __restrict__ part,
                                                            unsigned* __restrict__ ticket, unsigned long long* flag,
                                                            unsigned long long seq) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int RSF = pad_col(Rf), RSK = pad_col(K);
  double* YF = lds;              // [16][RSF]  y_f, then delta-y_f, then F x (a column is only touched by its own wave)
  double* Gx = YF + CB * RSF;    // [16][RSK]  gather of eta * yc
  double* G2 = Gx + CB * RSK;    // [16][RSK]  gather of eta * delta-yc
  double* Xt = G2 + CB * RSK;    // [16][RSK]  x
  double* Qt = Xt + CB * RSK;    // [16][RSK]  S0 x
  const int64_t c0 = (int64_t)blockIdx.x * CB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = threadIdx.x & 15, kg = threadIdx.x >> 4;
  const bool cok = c0 + c < C;
  const int col = (int)(c0 + c), agent = col / D, dd_ = col - agent * D;
  double ndy = 0.0, supp = 0.0, natdy = 0.0;
  PHASE_MARK(32);
  for (int k = kg; k < K; k += FT / CB) {
    double acc = 0.0, acc2 = 0.0, xv = 0.0;
    if (cok) {
      if (has_rows) {
        const int cell = cell_of(k, agent, K);
        const int t0 = cell_ptr[cell], t1 = cell_ptr[cell + 1];
        for (int t = t0; t < t1; ++t) acc += coef[(size_t)t * D + dd_] * gval[t];
        if (with_dy)
          for (int t = t0; t < t1; ++t) acc2 += coef[(size_t)t * D + dd_] * gval2[t];
      }
      xv = x[(int64_t)k * C + c0 + c];
    }
    Gx[c * RSK + k] = acc;
    G2[c * RSK + k] = acc2;
    Xt[c * RSK + k] = xv;
  }
  for (int r = kg; r < Rf; r += FT / CB) YF[c * RSF + r] = cok ? yf[(int64_t)r * C + c0 + c] : 0.0;
  __syncthreads();
  PHASE_MARK(33);
  double rd = 0.0, npx = 0.0, nat = 0.0;
  {
    double aty[E];
    column_At<E, true>(K, h, YF + wave * RSF, Gx + wave * RSK, aty);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = (64 * E - 1) - (lane * E + e);
      if (k < K) {
        const double px = 2.0 * Xt[wave * RSK + k];
        rd = fmax(rd, fabs(px + aty[e]));
        npx = fmax(npx, fabs(px));
        nat = fmax(nat, fabs(aty[e]));
      }
    }
  }
  PHASE_MARK(34);
  if (with_dy) {  // wave-uniform
    __syncthreads();
    for (int r = kg; r < Rf; r += FT / CB) {
      double dd = 0.0;
      if (cok) {
        const int64_t g = (int64_t)r * C + c0 + c;
        dd = dyf[g];
        ndy = fmax(ndy, fabs(dd));
        supp += uf[g] * fmax(dd, 0.0) + lf[g] * fmin(dd, 0.0);
      }
      YF[c * RSF + r] = dd;
    }
    __syncthreads();
    double atdy[E];
    column_At<E, true>(K, h, YF + wave * RSF, G2 + wave * RSK, atdy);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = (64 * E - 1) - (lane * E + e);
      if (k < K) natdy = fmax(natdy, fabs(atdy[e]));
    }
  }
  PHASE_MARK(35);
  {
    // F x and S0 x (every lane of this wave is done with its column of YF)
    double xk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = lane * E + e;
      xk[e] = k < K ? Xt[wave * RSK + k] : 0.0;
    }
    column_forward<E, true>(K, h, xk, YF + wave * RSF, Qt + wave * RSK);
  }
  __syncthreads();
  PHASE_MARK(36);
  double rp = 0.0, nax = 0.0, nz = 0.0;
  if (cok) {
    for (int r = kg; r < Rf; r += FT / CB) {
      const int64_t g = (int64_t)r * C + c0 + c;
      const double a = YF[c * RSF + r], z = zf[g];
      Fx[g] = a;
      rp = fmax(rp, fabs(a - z));
      nax = fmax(nax, fabs(a));
      nz = fmax(nz, fabs(z));
    }
    for (int k = kg; k < K; k += FT / CB) Qx[(int64_t)k * C + c0 + c] = Qt[c * RSK + k];
  }
  PHASE_MARK(37);
  // nine workgroup reductions with one barrier: DPP inside the waves, lane 63 of every wave to LDS, 9 threads finish
  __shared__ double red[NWV][9];
  {
    const double v[9] = {wave_max_nn(rp),  wave_max_nn(nax), wave_max_nn(nz),     wave_max_nn(rd),   wave_max_nn(npx),
                         wave_max_nn(nat), wave_max_nn(ndy), wave_incl_sum(supp), wave_max_nn(natdy)};
    if (lane == 63) {
#pragma unroll
      for (int j = 0; j < 9; ++j) red[wave][j] = v[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int j = threadIdx.x;
    double t = 0.0;
    for (int w = 0; w < NWV; ++w) t = j == RS_SUPP ? t + red[w][j] : fmax(t, red[w][j]);
    part[(size_t)blockIdx.x * SCP_RESID_STRIDE + j] = t;
  }
  PHASE_MARK(38);
  if (flag) {  // no row kernel follows (QP#0): the LAST workgroup raises the host's completion word itself -- one launch less
    if (threadIdx.x < 9) __threadfence_system();  // (the partials live in mapped host memory)
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
      *ticket = 0u;  // (the next launch on this stream starts after this kernel has ended)
      __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

constexpr int RESID_ROW_BLOCKS = 128;

template <int D>
__global__ __launch_bounds__(256) void cg1_resid_rows_kernel(int64_t nW, int64_t C, int with_dy, const int* __restrict__ wk,
                                                              const int* __restrict__ wi, const int* __restrict__ wj,
                                                              const double* __restrict__ weta,
                                                              const double* __restrict__ wl, const double* __restrict__ Qx,
                                                              const double* __restrict__ zc,
                                                              const double* __restrict__ dyc, double* __restrict__ part) {
  __shared__ double sm[4][5];
  double rp = 0.0, nax = 0.0, nz = 0.0, ndy = 0.0, supp = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nW; n += (int64_t)RESID_ROW_BLOCKS * 256) {
    const int64_t bi = (int64_t)wk[n] * C + (int64_t)wi[n] * D;
    const int64_t bj = (int64_t)wk[n] * C + (int64_t)wj[n] * D;
    double a = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) a += weta[n * D + d] * (Qx[bi + d] - Qx[bj + d]);
    const double z = zc[n];
    rp = fmax(rp, fabs(a - z));
    nax = fmax(nax, fabs(a));
    nz = fmax(nz, fabs(z));
    if (with_dy) {
      const double dd = dyc[n];  // delta-y of the last iteration, already projected (u = +inf)
      ndy = fmax(ndy, fabs(dd));
      supp += wl[n] * dd;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    rp = fmax(rp, __shfl_xor(rp, o)); nax = fmax(nax, __shfl_xor(nax, o)); nz = fmax(nz, __shfl_xor(nz, o));
    ndy = fmax(ndy, __shfl_xor(ndy, o)); supp += __shfl_xor(supp, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[w][0] = rp; sm[w][1] = nax; sm[w][2] = nz; sm[w][3] = ndy; sm[w][4] = supp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (size_t)blockIdx.x * SCP_RESID_STRIDE;
    o[RS_RP] = fmax(fmax(sm[0][0], sm[1][0]), fmax(sm[2][0], sm[3][0]));
    o[RS_NAX] = fmax(fmax(sm[0][1], sm[1][1]), fmax(sm[2][1], sm[3][1]));
    o[RS_NZ] = fmax(fmax(sm[0][2], sm[1][2]), fmax(sm[2][2], sm[3][2]));
    o[RS_RD] = o[RS_NPX] = o[RS_NATY] = o[RS_NATDY] = 0.0;
    o[RS_NDY] = fmax(fmax(sm[0][3], sm[1][3]), fmax(sm[2][3], sm[3][3]));
    o[RS_SUPP] = (sm[0][4] + sm[1][4]) + (sm[2][4] + sm[3][4]);
  }
}

// last launch of a check: everything before it in the stream has completed and, the partials living in host memory,
// is visible to the host; the host spins on this word instead of sleeping in hipStreamSynchronize (25 us per check)
__global__ void check_done_kernel(unsigned long long* flag, unsigned long long seq) {
  __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace

int scp_qp_fused_residuals(scp_qp* qp, bool with_dy) {
  const QpDev& d = qp->d;
  scp_ctx* ctx = qp->ctx;
  const int K = qp->K, Rf = qp->Rf;
  const int64_t C = qp->C;
  const int nblk = (int)((C + CB - 1) / CB);
  double* Qx = scp_qp_qx(qp);
  double* part = qp->h_scal_dev + SL_COUNT;  // [nblk column blocks | RESID_ROW_BLOCKS row blocks][SCP_RESID_STRIDE]
  const int has_rows = qp->nW > 0 ? 1 : 0;
  if (has_rows) QP_CHECK(scp_qp_rows_check_values(qp, with_dy));  // gval2 = yc, gval3 = delta-yc
  const size_t lds = (size_t)CB * (pad_col(Rf) + 4 * pad_col(K)) * sizeof(double);
  const unsigned long long seq = ++qp->check_seq;
  unsigned long long* flag_dev = (unsigned long long*)(qp->h_scal_dev + SL_COUNT + SCP_RESID_CAP);
  unsigned* ticket = ctx->d_ticket + 1;  // ([0]: the small-problem pairwise passes; same stream, never concurrent)
  QP_CHECK(qp_launch(qp, K <= 64 ? cg1_resid_col_kernel<1> : cg1_resid_col_kernel<2>, dim3(nblk), dim3(FT), lds, K, Rf, C, qp->h,
                     qp->N, qp->D, with_dy ? 1 : 0, has_rows, d.x, d.zf, d.yf, d.lf, d.uf, d.dyf, d.cell_ptr, d.coef, d.gval2,
                     d.gval3, Qx, d.fx, part, ticket, has_rows ? nullptr : flag_dev, seq));
  if (has_rows) {  // (QP#0: no row partials, and the column kernel's last workgroup raises the completion word)
    QP_CHECK(qp_launch(qp, qp->D == 2 ? cg1_resid_rows_kernel<2> : cg1_resid_rows_kernel<3>, dim3(RESID_ROW_BLOCKS), dim3(256),
                       0, qp->nW, C, with_dy ? 1 : 0, d.w_k, d.w_i, d.w_j, d.w_eta, d.w_l, Qx, d.zc, d.dyc,
                       part + (size_t)nblk * SCP_RESID_STRIDE));
    QP_CHECK(qp_launch(qp, check_done_kernel, dim3(1), dim3(1), 0, flag_dev, seq));
  }
  const int npart = nblk + (has_rows ? RESID_ROW_BLOCKS : 0);
  volatile unsigned long long* flag = (volatile unsigned long long*)(qp->h_scal + SL_COUNT + SCP_RESID_CAP);
  if (!scp_wait_host_word(flag, seq, 20)) SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // a fault surfaces here
  if (*flag != seq) return scp_fail(ctx, SCP_ERR_HIP, "fused check: completion flag not written");
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  double* hs = qp->h_scal;
  static const int slot[9] = {SL_RP, SL_NAX, SL_NZ, SL_RD, SL_NPX, SL_NATY, SL_NDY, SL_SUPP, SL_NATDY};
  for (int j = 0; j < 9; ++j) hs[slot[j]] = 0.0;
  for (int b = 0; b < npart; ++b) {  // fixed order: deterministic
    const double* o = hs + SL_COUNT + (size_t)b * SCP_RESID_STRIDE;
    for (int j = 0; j < 9; ++j) {
      if (j == RS_SUPP) hs[SL_SUPP] += o[j];
      else hs[slot[j]] = fmax(hs[slot[j]], o[j]);
    }
  }
  qp_on_fused_check(qp);
  return SCP_OK;
}

#ifdef SCP_PHASE_PROFILE
// developer hook of the profiling build only (not declared in include/scp_hip.h)
extern "C" int scp_debug_phase_clocks(unsigned long long* out, int n) {
  if (n > 64) n = 64;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(scp_phase_clk), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
