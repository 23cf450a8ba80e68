// Device body of scp_qp_reset's one-launch form, shared by qp_reset_kernel (scp_qp.hip) and by the kernel that resets a QP
// AND installs its first rows in the same launch (scp_qp_rows.hip).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "scp_pair_device.h"

constexpr int RESET_COLS = 16;
// x0 ([N][K][D] or NULL: zeros) -> time-major x, z_f = F x, the carried F x and S0 x of the single-step pipeline (exact),
// y_f = 0.  16 columns per workgroup (256 columns of a 128-agent problem still make 16 workgroups), the x tile in LDS
// (reset_xs: [K][RESET_COLS] doubles), thread = (column, one sixteenth of the rows); the first 256 threads of the workgroup
// work (`active`), all of them must call (one barrier).  COH: S0 x is written through -- the last workgroup of the same
// kernel reads it.
//
// The reset's own launch at full width (qp_reset_tiled_body below) computes the same dot products, element for element: one
// accumulator per output, k = 0 .. K-1 in order, the expression `acc += row[k] * xv` of this body.
template <bool COH>
__device__ inline void qp_reset_body(int tid, bool active, double* reset_xs, int N, int K, int D, int Rf,
                                     const double* __restrict__ x0, const double* __restrict__ F,
                                     const double* __restrict__ S0, double* __restrict__ x, double* __restrict__ zf,
                                     double* __restrict__ fx, double* __restrict__ Qx, double* __restrict__ yf) {
  constexpr int RG = 256 / RESET_COLS;
  const int64_t C = (int64_t)N * D;
  const int lc = tid & (RESET_COLS - 1), rg = tid / RESET_COLS;
  const int64_t c = (int64_t)blockIdx.x * RESET_COLS + lc;
  const bool live = active && c < C;
  const int64_t agent = live ? c / D : 0;
  const int dim = live ? (int)(c - agent * D) : 0;
  if (active) {
    for (int k = rg; k < K; k += RG) {
      const double v = (live && x0) ? x0[(agent * K + k) * D + dim] : 0.0;
      reset_xs[k * RESET_COLS + lc] = v;
      if (live) x[(int64_t)k * C + c] = v;
    }
  }
  __syncthreads();
  if (!active) return;
  // four rows per thread and pass: one LDS read of x[k] feeds four independent multiply-add chains (one row at a time was
  // a chain of K dependent loads + FMAs per row: 42 us at 1024 agents)
  constexpr int RB = 4;
  for (int r0 = rg * RB; r0 < Rf + K; r0 += RG * RB) {
    const double* __restrict__ row[RB];
    double acc[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const int r = min(r0 + j, Rf + K - 1);
      row[j] = r < Rf ? F + (size_t)r * K : S0 + (size_t)(r - Rf) * K;
      acc[j] = 0.0;
    }
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
      const double xv = reset_xs[k * RESET_COLS + lc];
#pragma unroll
      for (int j = 0; j < RB; ++j) acc[j] += row[j][k] * xv;
    }
    if (!live) continue;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const int r = r0 + j;
      if (r >= Rf + K) break;
      if (r < Rf) {
        zf[(int64_t)r * C + c] = acc[j];
        fx[(int64_t)r * C + c] = acc[j];
        yf[(int64_t)r * C + c] = 0.0;
      } else if (COH) {
        store_coherent(Qx + (int64_t)(r - Rf) * C + c, acc[j]);
      } else {
        Qx[(int64_t)(r - Rf) * C + c] = acc[j];
      }
    }
  }
}

// The same reset spread over the whole chip: a grid of (column tile) x (row slab) workgroups instead of one workgroup per 16
// columns (128 workgroups at 1024 x 2 columns, each thread walking ~800 rows of F | S0 through global loads: 36 us for 11 MB
// of stores).  A workgroup stages RESET_SLAB rows of [F ; S0] (one contiguous piece of each matrix) and the x tile of
// RESET_TILE columns in LDS -- lane = column as in qp_reset_body, the four waves take k mod 4, so the tile's agents are read
// line by line -- then wave w computes rows 4 w .. 4 w + 3 of the slab for its 64 columns: the row value is an LDS
// broadcast, the x value a conflict-free read.  The workgroups of slab 0 also write x (time-major).  Every output is the dot
// product qp_reset_body forms -- same expression, same order of k, same contraction -- so the two forms agree bit for bit
// (tests/test_reset_forms_gpu.py).
constexpr int RESET_TILE = 64;                     // columns per workgroup (one wave across)
constexpr int RESET_RB = 4;                        // rows per wave
constexpr int RESET_SLAB = (256 / 64) * RESET_RB;  // rows of [F ; S0] per workgroup
inline size_t qp_reset_tiled_lds_bytes(int K) { return (size_t)K * (RESET_TILE + RESET_SLAB) * sizeof(double); }

// grid (ceil(C / RESET_TILE), ceil((Rf + K) / RESET_SLAB)), 256 threads, lds: qp_reset_tiled_lds_bytes(K); D is 2 or 3
__device__ inline void qp_reset_tiled_body(double* lds, int N, int K, int D, int Rf, const double* __restrict__ x0,
                                           const double* __restrict__ F, const double* __restrict__ S0,
                                           double* __restrict__ x, double* __restrict__ zf, double* __restrict__ fx,
                                           double* __restrict__ Qx, double* __restrict__ yf) {
  double* xs = lds;                            // [K][RESET_TILE]
  double* fs = lds + (size_t)K * RESET_TILE;   // [RESET_SLAB][K]
  const int tid = threadIdx.x;
  const int lc = tid & (RESET_TILE - 1), w = tid / RESET_TILE;
  const int64_t C = (int64_t)N * D;
  const int64_t c = (int64_t)blockIdx.x * RESET_TILE + lc;
  const bool live = c < C;
  const int R = Rf + K;
  const int r_lo = blockIdx.y * RESET_SLAB;
  {  // the slab: rows r_lo .. of F, continued by S0's (rows past the end: zeros); [row][k] in LDS as in both matrices
    const int f_end = Rf * K, s_end = R * K, e_lo = r_lo * K;
    for (int e = tid; e < RESET_SLAB * K; e += 256) {
      const int g = e_lo + e;
      fs[e] = g < f_end ? F[g] : (g < s_end ? S0[g - f_end] : 0.0);
    }
  }
  {  // the x tile (and, from slab 0, x itself)
    const int64_t agent = D == 2 ? c >> 1 : c / 3;
    const int dim = (int)(c - agent * D);
    const double* __restrict__ src = (live && x0) ? x0 + agent * K * D + dim : nullptr;
    const bool write_x = live && blockIdx.y == 0;
#pragma unroll 4
    for (int k = w; k < K; k += 256 / RESET_TILE) {
      const double v = src ? src[(int64_t)k * D] : 0.0;
      xs[k * RESET_TILE + lc] = v;
      if (write_x) x[(int64_t)k * C + c] = v;
    }
  }
  __syncthreads();
  const int rl0 = w * RESET_RB;
  const double* __restrict__ row = fs + (size_t)rl0 * K;
  double acc[RESET_RB];
#pragma unroll
  for (int j = 0; j < RESET_RB; ++j) acc[j] = 0.0;
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    const double xv = xs[k * RESET_TILE + lc];
#pragma unroll
    for (int j = 0; j < RESET_RB; ++j) acc[j] += row[j * K + k] * xv;
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < RESET_RB; ++j) {
    const int r = r_lo + rl0 + j;
    if (r >= R) break;
    if (r < Rf) {
      zf[(int64_t)r * C + c] = acc[j];
      fx[(int64_t)r * C + c] = acc[j];
      yf[(int64_t)r * C + c] = 0.0;
    } else {
      Qx[(int64_t)(r - Rf) * C + c] = acc[j];
    }
  }
}
