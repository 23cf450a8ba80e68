// What the passes over DELAYED fleets share (gfx950 only): scp_delay_margins (scp_delay.hip) and scp_lag_conflicts
// (scp_stagger.hip).  Both compare a held, flying or parked record of vehicle a with a record of every b, so there is ONE
// definition of the K + 2 staging records per vehicle and of the tile fetch with a record index per side; everything else of
// the tile scaffold is scp_separation_device.h's.  Everything lives in the unnamed namespace, like the kernels that use it.
//
// Records: K + 2 per vehicle, time major -- index 0: held at the start (p[0], 0, 0); 1 .. K: the stored segments; K + 1:
// parked at the goal (pK, 0, 0).  In the global segment g of lag s vehicle a uses record index max(g - s, -1) + 1 and
// every b != a index min(g, K) + 1: two contiguous copies per tile and segment.
#pragma once
#include <algorithm>

#include "scp_separation_device.h"

namespace {

// The staging records.  pK = p[K-1] + (h v[K-1] + (h^2/2) a[K-1]) with every product and every sum rounded on its own, so
// that numpy reproduces its bits.
__global__ __launch_bounds__(256) void dly_prep_kernel(int N, int K, int D, double h, const double* __restrict__ pos,
                                                        const double* __restrict__ vel, const double* __restrict__ acc,
                                                        double* __restrict__ rec, unsigned long long* __restrict__ n_solved) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (record, i)
  if (t == 0) *n_solved = 0ULL;
  if (t >= (int64_t)N * (K + 2)) return;
  const int r = (int)(t / N) - 1, i = (int)(t % N);  // r = -1: held, K: parked
  const int k = r < 0 ? 0 : (r >= K ? K - 1 : r);
  const int64_t src = ((int64_t)i * K + k) * D;
  double* o = rec + t * (3 * D + 1);
  const double hh2 = 0.5 * h * h;
  double vv = 0.0, aa = 0.0;
  for (int d = 0; d < D; ++d) {
    double p = pos[src + d], v = vel[src + d], a = acc[src + d];
    if (r >= K) {
      const double hv = h * v, ha = hh2 * a;
      const double step = hv + ha;
      p = p + step;
    }
    if (r < 0 || r >= K) v = a = 0.0;
    o[d] = p;
    o[D + d] = v;
    o[2 * D + d] = a;
    vv = fma(v, v, vv);
    aa = fma(a, a, aa);
  }
  // sep_prep_kernel's upper bound of h |v| + h^2/2 |a| (exactly 0 for a held or parked record)
  o[3 * D] = (h * sqrt(vv) + hh2 * sqrt(aa)) * (1.0 + 1e-12);
}

// TileStage with a record index per side: the a side (planes [0, 64)) stages record ra, the b side ([64, 128)) record rb
template <int NC>
struct DlyStage : TileStage<NC, NC> {
  using Base = TileStage<NC, NC>;
  __device__ __forceinline__ void fetch2(const double* __restrict__ rec, int ra, int rb, int N, int a0, int b0, int tid) {
#pragma unroll
    for (int e = 0; e < Base::PER_THREAD; ++e) {
      const int x = tid + e * SEP_THREADS;
      if (x < Base::COUNT) {
        const int side = x / (SEP_TILE * NC), y = x % (SEP_TILE * NC);
        const int v = min((side ? b0 : a0) + y / NC, N - 1);
        this->pre[e] = rec[((int64_t)(side ? rb : ra) * N + v) * NC + y % NC];
      }
    }
  }
};

// How a call covers its entries: tiles, lags per workgroup, global segments per workgroup (lag_chunk / time_chunk: the
// call's developer switches, 0: chosen here)
struct DlyPlan {
  int nta, ntb, lc, n_lchunks, gc, n_gchunks;
  int64_t n_tiles;
};

inline DlyPlan dly_plan(const scp_ctx* ctx, int N, int K, int n_a, int S, int lag_chunk, int time_chunk) {
  DlyPlan p{};
  p.nta = scp_cdiv(n_a, SEP_TILE);
  p.ntb = scp_cdiv(N, SEP_TILE);
  p.n_tiles = (int64_t)p.nta * p.ntb;
  // ~8 workgroups per compute unit: first from the lags, then, where tiles x lags are still too few, from the segments (at
  // least four per workgroup: each (lag, chunk) costs a partial per vehicle)
  const int64_t want = 8 * (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
  const int64_t tiles = std::max<int64_t>(p.n_tiles, 1);
  const int64_t lch = std::min<int64_t>(S + 1, std::max<int64_t>(1, (want + tiles - 1) / tiles));
  p.lc = lag_chunk > 0 ? std::min(lag_chunk, S + 1) : scp_cdiv(S + 1, lch);
  p.n_lchunks = scp_cdiv(S + 1, p.lc);
  const int G = K + S;
  const int64_t wgs = tiles * p.n_lchunks;
  const int64_t gch = std::min<int64_t>(G, std::max<int64_t>(1, (want + wgs - 1) / wgs));
  p.gc = time_chunk > 0 ? std::min(time_chunk, G) : std::max(std::min(4, G), scp_cdiv(G, gch));
  p.n_gchunks = scp_cdiv(G, p.gc);
  return p;
}

}  // namespace
