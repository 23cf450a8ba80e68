// What the two translation units of the continuous-time separation passes share (gfx950 only): the check and the conflict
// list (scp_separation.hip) and the clearance profile (scp_clearance.hip).  The per-segment arithmetic must be the same on the
// same operand bits in all of them -- the profile's minima are compared bit for bit with the check's and the list's --, so
// there is ONE definition of every piece of the tile scaffold: the staging record and how a tile's records reach LDS, the
// tiling and its range tests, the sampled d.d, the quartic, the violation test, the row id and the lexicographic fold; and
// ONE host path around the kernels of a call (SepCall: plan, workspace, timing bracket, record staging).
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

// Does the tile with the corner (i0, j0) hold a pair of [q_begin, q_end)?  Rows of the triangle are contiguous in q, so the
// tile's own range decides.
__device__ inline bool tile_live(int i0, int j0, int N, int64_t q_begin, int64_t q_end) {
  const int i_last = min(i0 + SEP_TILE, N - 1) - 1;  // last vehicle that can be an `i` (i < j <= N - 1)
  const int j_lo = max(j0, i0 + 1), j_hi = min(j0 + SEP_TILE, N) - 1;
  bool live = i_last >= i0 && j_hi >= j_lo && j_hi > i0;
  if (live) {
    const int64_t q_min = tri_off(i0, N) + (j_lo - i0 - 1);
    const int64_t q_max = tri_off(i_last, N) + (j_hi - i_last - 1);
    live = q_max >= q_begin && q_min < q_end;
  }
  return live;
}

// A thread's j (fixed: j0 + lane) and its 16 i's (i0 + wave + 4 s): bit s says that the pair exists and lies in the range
__device__ inline unsigned int tile_valid_mask(int i0, int j0, int wave, int lane, int N, int64_t q_begin, int64_t q_end) {
  const int j = j0 + lane;
  unsigned int valid = 0;
  for (int s = 0; s < SEP_STEPS; ++s) {
    const int i = i0 + wave + 4 * s;
    if (i < j && j < N) {
      const int64_t q = tri_off(i, N) + (j - i - 1);
      if (q >= q_begin && q < q_end) valid |= 1u << s;
    }
  }
  return valid;
}

// row id of the segment k of the tile pair (il, jl)
__device__ inline unsigned long long tile_row(int k, int64_t pairs, int N, int i0, int j0, int il, int jl) {
  const int i = i0 + il, j = j0 + jl;
  return (unsigned long long)((int64_t)k * pairs + tri_off(i, N) + (j - i - 1));
}

// Double-buffered staging of a tile's records: the first NF fields of the 2 x 64 records of NC doubles of step k (contiguous
// per side in the time-major array) go to registers (fetch: in flight during the previous step's arithmetic) and from there
// to the component planes sm[field][128] ([0, 64): the i side, [64, 128): the j side; stash).  Vehicles beyond N - 1 repeat
// it: their pairs are not valid.  The kernel owns the loop and the barriers around stash.
template <int NC, int NF>
struct TileStage {
  static constexpr int COUNT = 2 * SEP_TILE * NF, PER_THREAD = (COUNT + SEP_THREADS - 1) / SEP_THREADS;
  double pre[PER_THREAD];
  __device__ __forceinline__ void fetch(const double* __restrict__ rec, int k, int N, int i0, int j0, int tid) {
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
      const int x = tid + e * SEP_THREADS;
      if (x < COUNT) {
        const int side = x / (SEP_TILE * NF), y = x % (SEP_TILE * NF);
        const int v = min((side ? j0 : i0) + y / NF, N - 1);
        pre[e] = rec[((int64_t)k * N + v) * NC + y % NF];
      }
    }
  }
  template <int P>
  __device__ __forceinline__ void stash(double (&sm)[P][2 * SEP_TILE], int tid) const {
    static_assert(P >= NF, "a plane per staged field");
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
      const int x = tid + e * SEP_THREADS;
      if (x < COUNT) {
        const int side = x / (SEP_TILE * NF), y = x % (SEP_TILE * NF);
        sm[y % NF][side * SEP_TILE + y / NF] = pre[e];
      }
    }
  }
};

// sampled d.d of the tile's vehicle il against the position pj: the operands and the order of pair_geom -- the same bits
template <int D, int P>
__device__ __forceinline__ double tile_dd(const double (&sm)[P][2 * SEP_TILE], int il, const double (&pj)[D]) {
  double ss = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double df = sm[d][il] - pj[d];
    ss = fma(df, df, ss);
  }
  return ss;
}

struct Quartic {
  double c0, c1, c2, c3, c4;
  __device__ double f(double t) const { return fma(t, fma(t, fma(t, fma(t, c4, c3), c2), c1), c0); }
  __device__ double g(double t) const { return fma(t, fma(t, fma(t, 4.0 * c4, 3.0 * c3), 2.0 * c2), c1); }  // f'
};

// The quartic of the pair (il, jl) of a tile from the staged component planes sm[3 D + 1][128]: d, w, b and the six dot
// products in this fma order.  c0 = d.d carries the bits of the sampled pass.
template <int D>
__device__ __forceinline__ Quartic tile_quartic(const double (&sm)[3 * D + 1][2 * SEP_TILE], int il, int jl) {
  double dd = 0.0, dw = 0.0, db = 0.0, ww = 0.0, wb = 0.0, bb = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double dx = sm[d][il] - sm[d][SEP_TILE + jl];
    const double wx = sm[D + d][il] - sm[D + d][SEP_TILE + jl];
    const double bx = sm[2 * D + d][il] - sm[2 * D + d][SEP_TILE + jl];
    dd = fma(dx, dx, dd);
    dw = fma(dx, wx, dw);
    db = fma(dx, bx, db);
    ww = fma(wx, wx, ww);
    wb = fma(wx, bx, wb);
    bb = fma(bx, bx, bb);
  }
  return Quartic{dd, 2.0 * dw, ww + db, wb, 0.25 * bb};
}

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

// the same over the 64 lanes of a wave: every lane ends with the wave's smallest (m, row) and its t
__device__ inline void wave_fold_min(double& m, unsigned long long& row, double& t) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double m2 = __shfl_xor(m, s, 64), t2 = __shfl_xor(t, s, 64);
    const unsigned long long r2 = __shfl_xor(row, s, 64);
    fold_min(m, row, t, m2, r2, t2);
  }
}

// Is a segment whose f has the minimum m a violation?  THE test of n_violating, of the list and of the profile's counts
// (crossing vehicles: f a few ulps below 0).
__device__ inline bool sep_violates(double m, double thr) { return sqrt(fmax(m, 0.0)) < thr; }

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

// ---- the host path of a call: what scp_check_separation, scp_list_conflicts and scp_clearance_profile do alike --------------
struct SepCall {
  SepPlan plan;
  double* rec;   // the staged records [K][N][3 D + 1] at the start of the ctx's workspace ...
  char* extra;   // ... and the caller's bytes behind them (64-byte aligned)
};

// The checks common to the three (`who` names the entry point in the messages), the plan, a workspace of the records plus
// extra_bytes(plan) bytes, the start of the timing bracket and the records themselves.  The three calls are stream-ordered
// and each stages its own records, so they share ONE workspace.
template <class ExtraBytes>
int sep_begin(scp_ctx* ctx, const char* who, int N, int K, int D, double h, int64_t q_begin, int64_t q_end, const double* pos,
              const double* vel, const double* acc, ExtraBytes extra_bytes, SepCall* c) {
  int rc = scp_check_pair_range(ctx, N, K, D, q_begin, q_end);
  if (rc) return rc;
  SCP_REQUIRE(ctx, pos && vel && acc, "%s: null pointer", who);
  SCP_REQUIRE(ctx, h > 0.0 && h < SEP_INF, "%s: bad time step h=%g", who, h);
  c->plan = sep_plan(ctx, N, K, q_begin, q_end);
  SCP_REQUIRE(ctx, c->plan.n_tiles < ((int64_t)1 << 31), "%s: %lld tiles exceed grid.x; shard the pair range", who,
              (long long)c->plan.n_tiles);
  const size_t rec_bytes = ((size_t)N * K * (3 * D + 1) * sizeof(double) + 63) & ~(size_t)63;
  rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, rec_bytes + extra_bytes(c->plan));
  if (rc) return rc;
  c->rec = (double*)ctx->sep_ws;
  c->extra = (char*)ctx->sep_ws + rec_bytes;
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  if (c->plan.n_tiles > 0)
    hipLaunchKernelGGL(sep_prep_kernel, dim3(scp_cdiv((int64_t)N * K, 256)), dim3(256), 0, ctx->stream, N, K, D, h, pos, vel,
                       acc, c->rec);
  return SCP_OK;
}

// after the call's last launch: launch errors, the end of the timing bracket
inline int sep_end(scp_ctx* ctx) {
  SCP_HIP_CHECK(ctx, hipGetLastError());
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev1, ctx->stream));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  return SCP_OK;
}

// a tile kernel's D = 2 or D = 3 instantiation over the plan's grid: one workgroup per (tile, chunk of time steps)
template <class Args>
void sep_launch_tiles(scp_ctx* ctx, const SepPlan& p, int D, void (*kernel2)(Args), void (*kernel3)(Args), const Args& a) {
  hipLaunchKernelGGL(D == 2 ? kernel2 : kernel3, dim3((unsigned)p.n_tiles, (unsigned)p.n_chunks), dim3(SEP_THREADS), 0,
                     ctx->stream, a);
}

// One of the ctx's two solved counts (ctx->solved: SEP_SOLVED_CHECK, SEP_SOLVED_PROFILE) to the host; synchronises
enum { SEP_SOLVED_CHECK = 0, SEP_SOLVED_PROFILE = 1 };

inline int sep_read_solved(scp_ctx* ctx, int which, const char* who, uint64_t* n) {
  if (!ctx || !n) return SCP_ERR_INVALID;
  if (!ctx->solved_ran[which]) return scp_fail(ctx, SCP_ERR_STATE, "%s has not run yet", who);
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemcpy(n, ctx->solved + which, sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SCP_OK;
}

}  // namespace
