// The near form of the recomputing violations pass (scp_collision_violations_at of a large problem): instead of all
// N (N - 1) / 2 * K rows, only the pairs close enough to be violated are evaluated.
//
//   viol_r = (R - dist_r) - eta_r . (dP_i[k] - dP_j[k]),  |eta_r| = 1   =>   viol_r <= R - dist_r + m_i[k] + m_j[k],  m = |dP|
//
// so a pair with dist >= R + m_i + m_j + tau has viol <= -tau: not violated for any feas_tol >= 0, and not the maximum as
// long as some examined row reaches -tau / 2 (the caller checks that and runs the exhaustive pass otherwise; tau:
// SCP_NEAR_TAU in scp_common.h).  All such pairs of a time step lie within rho_k = R + 2 max_i m_i[k] + tau of each other: a
// uniform grid of cells at least rho_k wide finds them among the 3^D neighbouring cells.  Examined rows go through the
// very functions of the exhaustive pass (scp_pair_device.h): the same bits; marks are bits and the statistic is a maximum,
// so the order in which the cells are walked does not show in the result.
#include "scp_common.h"
#include "scp_compact_device.h"
#include "scp_pair_device.h"
#include "scp_wave_device.h"

#include <algorithm>

constexpr int NEAR_THREADS = CMP_THREADS;  // (block_exclusive_scan is written for this many)
constexpr int NEAR_LANES = 4;              // lanes that share the candidates of one agent
constexpr int NEAR_AGENTS = NEAR_THREADS / NEAR_LANES;  // agents a workgroup examines at a time
constexpr int NEAR_MAX_S = 16;             // workgroups per time step (each bins the whole step: no more than pays)
constexpr int NEAR_MAX_CELLS = 2048;       // bins per time step; fewer and larger cells are always correct
template <int D>
struct NearCap {                           // cells per axis: 45^2, 12^3 <= NEAR_MAX_CELLS
  static constexpr int value = D == 2 ? 45 : 12;
};
// Cells are this factor wider than rho_k: two agents closer than rho_k then differ by less than 1 - 1e-6 in scaled
// coordinates, far more than the rounding of the scaling (1e-16 * cells per axis) -- their cell indices differ by at most 1.
constexpr double NEAR_SIDE_SLACK = 1.0 + 1e-6;
constexpr size_t NEAR_LDS_LIMIT = 160 * 1024 - 1024;  // gfx950: 160 KiB per workgroup, less the static reduction arrays

// LDS tables of one time step: positions, |dP| and ids of the agents sorted by cell, and the cells' ends
static size_t near_lds_bytes(int N, int D) {
  return (size_t)N * D * sizeof(double) + (size_t)N * sizeof(double) + (size_t)N * sizeof(int) + NEAR_MAX_CELLS * sizeof(int);
}
bool scp_near_fits(int N, int D, size_t* lds_bytes) {
  *lds_bytes = near_lds_bytes(N, D);
  return N >= 2 && (D == 2 || D == 3) && *lds_bytes <= NEAR_LDS_LIMIT;
}

template <int D>
struct NearGrid {
  double lo[D], inv[D];
  int n[D];
};
template <int D>
__device__ inline void near_cell(const NearGrid<D>& g, const Pt<D>& p, int (&c)[D]) {
#pragma unroll
  for (int d = 0; d < D; ++d)  // (fmax first: a NaN -- there is none, the staged values are bounded -- would become cell 0)
    c[d] = (int)fmin(fmax((p.v[d] - g.lo[d]) * g.inv[d], 0.0), (double)(g.n[d] - 1));
}
template <int D>
__device__ inline int near_cell_index(const NearGrid<D>& g, const int (&c)[D]) {
  int idx = c[D - 1];
#pragma unroll
  for (int d = D - 2; d >= 0; --d) idx = idx * g.n[d] + c[d];
  return idx;
}
// |dP| rounded up generously (1e-10 relative: nothing next to SCP_NEAR_TAU)
template <int D>
__device__ inline double near_reach(const Pt<D>& dp) {
  double ss = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) ss = fma(dp.v[d], dp.v[d], ss);
  return sqrt(ss) * (1.0 + 1e-10);
}

// Grid (K, S): workgroup (k, s) bins ALL agents of time step k (counting sort in LDS; S copies of that work, each
// N points from L2) and examines the agents in its slice of the sorted order, about [s, s + 1) * ceil(N / S), against the
// agents behind them in the 3^D neighbouring cells, NEAR_LANES lanes per agent.
template <int D>
__global__ __launch_bounds__(NEAR_THREADS) void near_violations_kernel(ScpNearArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double red[NEAR_THREADS / 64][2 * D + 1];
  if (__hip_atomic_load(a.unbounded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.call_no) return;  // (every workgroup)
  const int N = a.N, k = blockIdx.x, tid = threadIdx.x;
  const int64_t nq = a.q_end - a.q_begin;
  const double* P = a.P_tm + (int64_t)k * N * D;
  const double* Q = a.dP_tm + (int64_t)k * N * D;
  double* sP = lds;                                   // [N][D]
  double* sM = lds + (int64_t)N * D;                  // [N]
  int* sId = reinterpret_cast<int*>(sM + N);          // [N]
  int* sEnd = sId + N;                                // [cells]: counts, then starts, then ends of the cells
  const double INF = __longlong_as_double(0x7FF0000000000000LL);

  // ---- the step's bounding box and largest reach -> the grid ----
  double lo[D], hi[D], mmax = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    lo[d] = INF;
    hi[d] = -INF;
  }
  for (int i = tid; i < N; i += NEAR_THREADS) {
    const Pt<D> p = load_pt<D>(P, i);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      lo[d] = fmin(lo[d], p.v[d]);
      hi[d] = fmax(hi[d], p.v[d]);
    }
    mmax = fmax(mmax, near_reach<D>(load_pt<D>(Q, i)));
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    lo[d] = wave_min(lo[d]);
    hi[d] = wave_max(hi[d]);
  }
  mmax = wave_max(mmax);
  if ((tid & 63) == 63) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      red[tid >> 6][d] = lo[d];
      red[tid >> 6][D + d] = hi[d];
    }
    red[tid >> 6][2 * D] = mmax;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < D; ++d) {
    lo[d] = red[0][d];
    hi[d] = red[0][D + d];
  }
  mmax = red[0][2 * D];
#pragma unroll
  for (int w = 1; w < NEAR_THREADS / 64; ++w) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      lo[d] = fmin(lo[d], red[w][d]);
      hi[d] = fmax(hi[d], red[w][D + d]);
    }
    mmax = fmax(mmax, red[w][2 * D]);
  }
  NearGrid<D> g;
  int cells = 1;
  {
    const double side_min = (a.R + 2.0 * mmax + SCP_NEAR_TAU) * NEAR_SIDE_SLACK;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double ext = hi[d] - lo[d];
      g.n[d] = (int)fmin(floor(ext / side_min) + 1.0, (double)NearCap<D>::value);
      const double side = fmax(side_min, ext / (double)g.n[d] * NEAR_SIDE_SLACK);  // (a capped axis: wider cells)
      g.lo[d] = lo[d];
      g.inv[d] = 1.0 / side;
      cells *= g.n[d];
    }
  }

  // ---- counting sort of the agents by cell ----
  for (int c = tid; c < cells; c += NEAR_THREADS) sEnd[c] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += NEAR_THREADS) {
    int c[D];
    near_cell<D>(g, load_pt<D>(P, i), c);
    atomicAdd(sEnd + near_cell_index<D>(g, c), 1);
  }
  __syncthreads();
  {
    const int cpt = (cells + NEAR_THREADS - 1) / NEAR_THREADS;  // consecutive cells per thread (<= 8)
    const int c0 = tid * cpt, c1 = min(c0 + cpt, cells);
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += sEnd[c];
    int total;
    int run = block_exclusive_scan(mine, &total);
    for (int c = c0; c < c1; ++c) {
      const int n = sEnd[c];
      sEnd[c] = run;
      run += n;
    }
  }
  __syncthreads();
  for (int i = tid; i < N; i += NEAR_THREADS) {
    const Pt<D> p = load_pt<D>(P, i);
    int c[D];
    near_cell<D>(g, p, c);
    const int slot = atomicAdd(sEnd + near_cell_index<D>(g, c), 1);  // (the order within a cell is free)
#pragma unroll
    for (int d = 0; d < D; ++d) sP[slot * D + d] = p.v[d];
    sM[slot] = near_reach<D>(load_pt<D>(Q, i));
    sId[slot] = i;
  }
  __syncthreads();  // sEnd[c] is now the END of cell c (= the start of cell c + 1)

  // ---- this workgroup's slice of the agents against the agents behind them in the neighbouring cells ----
  // The order WITHIN a cell differs from workgroup to workgroup (the scatter's atomics), the cells' extents do not: the
  // slices are cut at cell boundaries -- the first cell start at or behind s * ceil(N / S) -- so that every workgroup
  // agrees on who examines an agent, and on which of two agents of different cells comes first.
  auto cell_start_from = [&](int x) -> int {
    if (x <= 0) return 0;
    if (x >= N) return N;
    int lo_c = 0, hi_c = cells - 1;  // the first cell whose end is >= x (sEnd is monotone, sEnd[cells - 1] = N)
    while (lo_c < hi_c) {
      const int mid = (lo_c + hi_c) >> 1;
      if (sEnd[mid] >= x) hi_c = mid;
      else lo_c = mid + 1;
    }
    return sEnd[lo_c];
  };
  const int chunk = (N + (int)gridDim.y - 1) / (int)gridDim.y;
  const int a0 = cell_start_from(min((int)blockIdx.y * chunk, N)), a1 = cell_start_from(min(((int)blockIdx.y + 1) * chunk, N));
  const int sub = tid & (NEAR_LANES - 1);
  double my_max = -INF;
  for (int sa = a0 + tid / NEAR_LANES; sa < a1; sa += NEAR_AGENTS) {
    Pt<D> Pa;
#pragma unroll
    for (int d = 0; d < D; ++d) Pa.v[d] = sP[sa * D + d];
    const double ma = sM[sa];
    const int ia = sId[sa];
    int ca[D];
    near_cell<D>(g, Pa, ca);
    // the cells (ca[0] - 1 .. ca[0] + 1, cy, cz) are consecutive: one range of sorted slots per (cy, cz)
    const int x0 = max(ca[0] - 1, 0), x1 = min(ca[0] + 1, g.n[0] - 1);
    const int z0 = D == 3 ? max(ca[D - 1] - 1, 0) : 0, z1 = D == 3 ? min(ca[D - 1] + 1, g.n[D - 1] - 1) : 0;
    for (int cz = z0; cz <= z1; ++cz) {
      for (int cy = max(ca[1] - 1, 0); cy <= min(ca[1] + 1, g.n[1] - 1); ++cy) {
        const int row = (D == 3 ? cz * g.n[1] + cy : cy) * g.n[0];
        const int b0 = row + x0 > 0 ? sEnd[row + x0 - 1] : 0, b1 = sEnd[row + x1];
        for (int sb = max(b0, sa + 1) + sub; sb < b1; sb += NEAR_LANES) {  // (sb > sa: every pair once)
          Pt<D> Pb;
          double ss = 0.0;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            Pb.v[d] = sP[sb * D + d];
            const double df = Pa.v[d] - Pb.v[d];
            ss = fma(df, df, ss);
          }
          const double reach = a.R + ma + sM[sb] + SCP_NEAR_TAU;
          if (!(ss < reach * reach * (1.0 + 1e-12))) continue;  // cannot be violated, cannot be the maximum
          const int ib = sId[sb];
          const bool fwd = ia < ib;
          const int i = fwd ? ia : ib, j = fwd ? ib : ia;
          const int64_t q = tri_off(i, N) + (j - i - 1);
          if (q < a.q_begin || q >= a.q_end) continue;
          // the row of MODE_VIOL_RECOMPUTE (pair_pass_kernel), operand for operand
          const PairGeom<D> pg = pair_geom<D>(fwd ? Pa : Pb, fwd ? Pb : Pa);
          const Pt<D> Di = load_pt<D>(Q, i), Dj = load_pt<D>(Q, j);  // dP = P_new - P_prev
          const double dist = pg.deg ? 1.0 : pg.raw;
          double qd = 0.0;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const double e_d = pg.deg ? (d == 0 ? 1.0 : 0.0) : pg.diff[d] * pg.inv;
            qd = fma(e_d, Di.v[d] - Dj.v[d], qd);
          }
          const double viol = (a.R - dist) - qd;  // l_r - (A x)_r
          my_max = fmax(my_max, viol);
          if (viol > a.feas_tol) {
            const int64_t lr = (int64_t)k * nq + (q - a.q_begin);
            if (!((a.bitmap[lr >> 5] >> (lr & 31)) & 1u)) atomicOr(a.mark + (lr >> 5), 1u << (lr & 31));
          }
        }
      }
    }
  }

  // one candidate per workgroup, the atomic only when it would improve the result (as the exhaustive pass)
  my_max = wave_max(my_max);
  __syncthreads();  // (red: the grid's reduction has been read)
  if ((tid & 63) == 63) red[tid >> 6][0] = my_max;
  __syncthreads();
  if (tid == 0) {
    double m = red[0][0];
#pragma unroll
    for (int w = 1; w < NEAR_THREADS / 64; ++w) m = fmax(m, red[w][0]);
    const double cur = __hip_atomic_load(&a.stats->max_violation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m > cur) atomic_max_double(&a.stats->max_violation, m);
  }
}

int scp_launch_near_violations(scp_ctx* ctx, const ScpNearArgs& a, size_t lds_bytes) {
  typedef void (*NearKernel)(ScpNearArgs);
  const NearKernel kern = a.D == 2 ? near_violations_kernel<2> : near_violations_kernel<3>;
  if (lds_bytes > 64 * 1024) SCP_HIP_CHECK(ctx, scp_raise_lds_limit(ctx->device, (const void*)kern, lds_bytes));
  const int S = std::min(scp_cdiv(a.N, NEAR_AGENTS), NEAR_MAX_S);
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  hipLaunchKernelGGL(kern, dim3(a.K, S), dim3(NEAR_THREADS), lds_bytes, ctx->stream, a);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev1, ctx->stream));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  return SCP_OK;
}

extern "C" int scp_ctx_set_near_pass(scp_ctx* ctx, int mode) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, mode >= 0 && mode <= 2, "ctx_set_near_pass: mode %d is not 0 (off), 1 (auto) or 2 (force)", mode);
  ctx->near_pass = mode;
  return SCP_OK;
}

extern "C" int scp_ctx_near_pass_counts(scp_ctx* ctx, uint64_t* n_near, uint64_t* n_fell_back) {
  if (!ctx || !n_near || !n_fell_back) return SCP_ERR_INVALID;
  *n_near = ctx->near_ran;
  *n_fell_back = ctx->near_fell_back;
  return SCP_OK;
}

extern "C" int scp_ctx_peek_scratch_map(scp_ctx* ctx, uint32_t* out, int64_t words) {
  if (!ctx || !out || words < 0) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, (size_t)words * sizeof(uint32_t) <= ctx->cmp_map_bytes, "ctx_peek_scratch_map: the map has %lld words",
              (long long)(ctx->cmp_map_bytes / sizeof(uint32_t)));
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (words > 0) SCP_HIP_CHECK(ctx, hipMemcpy(out, ctx->cmp_map, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SCP_OK;
}
