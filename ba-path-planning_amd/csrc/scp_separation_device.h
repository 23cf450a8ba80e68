// Device code shared by the two translation units of the continuous-time separation passes (gfx950 only): the check and the
// conflict list (scp_separation.hip) and the clearance profile (scp_clearance.hip).  The per-segment arithmetic must be the
// same on the same operand bits in all of them -- the profile's minima are compared bit for bit with the check's and the
// list's --, so there is ONE definition of the staging record, the tiling, the quartic and the lexicographic fold.
// Everything lives in the unnamed namespace, like the kernels that use it.
#pragma once
#include "scp_common.h"
#include "scp_pair_device.h"

namespace {

constexpr int SEP_THREADS = 256;
constexpr int SEP_TILE = 64;                               // vehicles per tile side: j = lane, i = wave + 4 s
constexpr int SEP_STEPS = SEP_TILE * SEP_TILE / SEP_THREADS;  // 16 pairs per thread and time step
constexpr double SEP_SKIP_FACTOR = 1.0 + 7e-6;             // on squared distances: (1 + 3e-6)^2 rounded up (derivation: the pass)
constexpr double SEP_INF = __builtin_huge_val();
constexpr unsigned long long SEP_NO_ROW = 0xFFFFFFFFFFFFFFFFULL;

// The staging record: [K][N][3 D + 1] doubles, time major -- pos, vel, acc of (k, vehicle) and its REACH rho.
__global__ __launch_bounds__(256) void sep_prep_kernel(int N, int K, int D, double h, const double* __restrict__ pos,
                                                        const double* __restrict__ vel, const double* __restrict__ acc,
                                                        double* __restrict__ rec) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (k, i): one record
  if (t >= (int64_t)N * K) return;
  const int k = (int)(t / N), i = (int)(t % N);
  const int64_t src = ((int64_t)i * K + k) * D;
  double* o = rec + t * (3 * D + 1);
  double vv = 0.0, aa = 0.0;
  for (int d = 0; d < D; ++d) {
    const double p = pos[src + d], v = vel[src + d], a = acc[src + d];
    o[d] = p;
    o[D + d] = v;
    o[2 * D + d] = a;
    vv = fma(v, v, vv);
    aa = fma(a, a, aa);
  }
  // an upper bound of h |v| + h^2/2 |a| (the roundings of the sums, roots and products stay far below the 3e-6 of the test)
  o[3 * D] = (h * sqrt(vv) + (0.5 * h * h) * sqrt(aa)) * (1.0 + 1e-12);
}

__device__ inline double wave_min_f64(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmin(v, __shfl_xor(v, s, 64));
  return v;
}

// tile index u in the upper triangle (diagonal included) of an nt x nt grid, row major -> (ti, tj), ti <= tj
__device__ inline void decode_tile(int64_t u, int nt, int& ti, int& tj) {
  const double b = 2.0 * nt + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)u)) * 0.5);
  if (r < 0) r = 0;
  if (r > nt - 1) r = nt - 1;
  auto start = [nt](int64_t x) { return x * nt - x * (x - 1) / 2; };
  while (start(r) > u) --r;
  while (r < nt - 1 && start(r + 1) <= u) ++r;
  ti = (int)r;
  tj = (int)(u - start(r) + r);
}

// first tile of tile row r (host and device)
__host__ __device__ inline int64_t tile_start(int64_t r, int64_t nt) { return r * nt - r * (r - 1) / 2; }

struct Quartic {
  double c0, c1, c2, c3, c4;
  __device__ double f(double t) const { return fma(t, fma(t, fma(t, fma(t, c4, c3), c2), c1), c0); }
  __device__ double g(double t) const { return fma(t, fma(t, fma(t, 4.0 * c4, 3.0 * c3), 2.0 * c2), c1); }  // f'
};

// The quartic of the pair (il, jl) of a tile from the staged component planes sm[3 D + 1][128] ([0, 64): the i side,
// [64, 128): the j side): d, w, b and the six dot products in this fma order.  c0 = d.d carries the bits of the sampled pass.
// A macro, not a function: every function form that was tried (array by pointer, by reference, result by value, through a
// reference) made the compiler swap the operands of the one v_add_f64 of c2 in sep_pass_kernel -- the same bits, but the
// instruction stream of the check and the list is pinned (profiles/clearance_device_code_identity.md).  Needs D in scope.
#define SEP_TILE_QUARTIC(q, sm, il, jl)                                                    \
  double dd = 0.0, dw = 0.0, db = 0.0, ww = 0.0, wb = 0.0, bb = 0.0;                       \
  _Pragma("unroll") for (int d = 0; d < D; ++d) {                                          \
    const double dx = sm[d][il] - sm[d][SEP_TILE + jl];                                    \
    const double wx = sm[D + d][il] - sm[D + d][SEP_TILE + jl];                            \
    const double bx = sm[2 * D + d][il] - sm[2 * D + d][SEP_TILE + jl];                    \
    dd = fma(dx, dx, dd);                                                                  \
    dw = fma(dx, wx, dw);                                                                  \
    db = fma(dx, bx, db);                                                                  \
    ww = fma(wx, wx, ww);                                                                  \
    wb = fma(wx, bx, wb);                                                                  \
    bb = fma(bx, bx, bb);                                                                  \
  }                                                                                        \
  const Quartic q{dd, 2.0 * dw, ww + db, wb, 0.25 * bb}

// Minimum of the quartic over [0, h] and where.  Candidates: 0 (f = c0, the sampled value exactly), h, the stationary
// points of f' inside (0, h) -- they split [0, h] into at most three pieces on which f' is monotone --, and in every piece
// over which f' goes from negative to positive the root of f' by bisection (48 halvings: to 4e-15 h; f' = 0 there, so the
// value of f is exact to second order).  No case is special: b = 0 makes f' linear (no split points), b = w = 0 makes f
// constant (no sign change), a double root of f' is a split point and hence a candidate itself.  Strict comparisons: a
// constant f reports t = 0.
__device__ inline void quartic_min(const Quartic& q, double h, double& m_out, double& t_out) {
  double m = q.c0, tm = 0.0;
  auto offer = [&](double t) {
    const double v = q.f(t);
    if (v < m) {
      m = v;
      tm = t;
    }
  };
  offer(h);
  // f''(t) / 2 = c2 + 3 c3 t + 6 c4 t^2
  double s1 = -1.0, s2 = -1.0;  // split points (outside (0, h): none)
  const double qa = 6.0 * q.c4, qb = 3.0 * q.c3, qc = q.c2;
  if (qa != 0.0) {
    const double disc = fma(qb, qb, -4.0 * qa * qc);
    if (disc > 0.0) {
      const double qd = -0.5 * (qb + copysign(sqrt(disc), qb));
      s1 = qd / qa;
      s2 = qc / qd;
    }
  } else if (qb != 0.0) {
    s1 = -qc / qb;
  }
  if (!(s1 > 0.0 && s1 < h)) s1 = -1.0;
  if (!(s2 > 0.0 && s2 < h)) s2 = -1.0;
  if (s1 < 0.0 || (s2 >= 0.0 && s2 < s1)) {
    const double x = s1;
    s1 = s2;
    s2 = x;
  }
  // now: s1 <= s2 where both exist, s1 exists if any does.  Pieces [0, pa], [pa, pb], [pb, h]; an empty one has no sign change
  const double pa = s1 >= 0.0 ? s1 : 0.0, pb = s2 >= 0.0 ? s2 : pa;
  if (s1 >= 0.0) offer(s1);
  if (s2 >= 0.0) offer(s2);
#pragma nounroll
  for (int e = 0; e < 3; ++e) {
    double lo = e == 0 ? 0.0 : (e == 1 ? pa : pb), hi = e == 0 ? pa : (e == 1 ? pb : h);
    if (q.g(lo) < 0.0 && q.g(hi) > 0.0) {
      for (int it = 0; it < 48; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (q.g(mid) < 0.0) lo = mid;
        else hi = mid;
      }
      offer(0.5 * (lo + hi));
    }
  }
  m_out = m;
  t_out = tm;
}

// (m, row) pairs order lexicographically; t rides along
__device__ inline void fold_min(double& m, unsigned long long& row, double& t, double m2, unsigned long long row2, double t2) {
  if (m2 < m || (m2 == m && row2 < row)) {
    m = m2;
    row = row2;
    t = t2;
  }
}

// How a call covers its pair range: the tile rows that hold it and the time steps per workgroup
struct SepPlan {
  int nt, kc, n_chunks;
  int64_t n_tiles, tile0;
  int t_lo, t_hi;  // the tile rows (t_lo > t_hi: none)
};

inline SepPlan sep_plan(const scp_ctx* ctx, int N, int K, int64_t q_begin, int64_t q_end) {
  SepPlan p{};
  p.nt = scp_cdiv(N, SEP_TILE);
  p.t_lo = 1;
  // the tile rows that hold the pair range: vehicle rows i_lo .. i_hi of the triangle
  if (q_end > q_begin) {
    auto row_of = [N](int64_t q) {
      int64_t lo = 0, hi = N - 2;  // largest i with tri_off(i) <= q
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (tri_off(mid, N) <= q) lo = mid;
        else hi = mid - 1;
      }
      return lo;
    };
    const int64_t t_lo = row_of(q_begin) / SEP_TILE, t_hi = row_of(q_end - 1) / SEP_TILE;
    p.t_lo = (int)t_lo;
    p.t_hi = (int)t_hi;
    p.tile0 = tile_start(t_lo, p.nt);
    p.n_tiles = tile_start(t_hi + 1, p.nt) - p.tile0;
  }
  // time steps per workgroup: as many as still leave ~8 workgroups per compute unit (the records of a step are staged once per
  // workgroup and step, so longer chunks only save the per-workgroup reduction)
  p.kc = K;
  if (p.n_tiles > 0) {
    const int64_t want = 8 * (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    const int64_t chunks = std::min<int64_t>(K, std::max<int64_t>(1, (want + p.n_tiles - 1) / p.n_tiles));
    p.kc = scp_cdiv(K, chunks);
  }
  p.n_chunks = scp_cdiv(K, p.kc);
  return p;
}

}  // namespace
