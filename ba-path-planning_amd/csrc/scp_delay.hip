// Delay margins (scp_delay_margins, include/scp_hip.h): for every vehicle a and every whole number of steps s = 0 .. S the
// clearance of the fleet in which a ALONE starts s steps late -- held at its start for s steps, then flying its stored plan,
// while everybody else flies on schedule and parks at the goal.  A delay of whole steps keeps the segment grids aligned, so
// every comparison is still ONE quartic on [0, h]: the per-segment arithmetic, the staging record, the tile scaffold, the
// violation test and the lexicographic fold are those of the other continuous-time passes (scp_separation_device.h), and entry
// (a, 0) is scp_clearance_profile's per_vehicle[a] bit for bit.
//
// Records and the two-sided tile fetch: scp_delay_device.h (shared with scp_lag_conflicts).
//
// Exclusion: a segment (a, s, b, g) is dropped without its quartic only if its distance provably exceeds
// T = max(R - 0.01, U), U an upper bound of the FINAL minimum of entry (a, s): the smallest minimum the workgroup has computed
// for that entry so far.  The check's margin derivation carries over unchanged (d.d > (T + rho_a + rho_b)^2 SEP_SKIP_FACTOR: the
// computed minimum of f stays above T^2 >= the entry's computed minimum so far), so a dropped segment is neither a violation
// nor the entry's argmin, not even tied: results never depend on what was dropped.  Before the entry has a result U is the
// smallest SAMPLED distance of the workgroup's first segment (the clearance pass's kind of bound: the pair that attains it is
// never dropped, d.d <= U^2 <= T^2, and its computed minimum is <= c0 = d.d), +inf without a pair.
//
// Kernels, all on the ctx stream (launches are the only synchronisation; no workgroup waits for another):
//   dly_prep_kernel    the K + 2 records per vehicle and the solved count to 0;
//   dly_pass_kernel    one workgroup per (64 x 64 tile of ORDERED pairs a != b, chunk of lags, chunk of global segments): per lag
//                      and segment phase A (one reach comparison per pair) and phase B (the queued quartics, dense over the
//                      threads); lane x of wave 0 OWNS the tile's vehicle a0 + x and folds the results that name it --
//                      (f, g, b) lexicographically, an integer count --, so no reduction depends on an order.  One partial per
//                      (segment chunk, b tile, vehicle, lag) goes to global memory;
//   dly_finish_kernel  one thread per entry (a, s): the fold over the segment chunks and the b tiles -> scp_delay_margin.
#include "scp_delay_device.h"

namespace {

// A partial result of one entry (a, s); the finishing kernel folds them in any order
struct DlyEntry {
  double m;                   // smallest segment minimum of f, +inf: none
  unsigned long long key;     // g << 32 | b of that segment; ties: the smallest; SEP_NO_ROW: none
  double t;                   // where in the segment
  unsigned long long n_viol;  // violating (b, g)
};

struct DlyArgs {
  int N, K, D, S;             // S: the largest lag
  int a_begin, a_end;         // the vehicles whose entries the call computes
  int ntb;                    // tiles along b: blockIdx.x = (a tile) * ntb + (b tile)
  int lc, gc;                 // lags (blockIdx.y) and global segments (blockIdx.z) per workgroup
  double h, thr;              // thr = R - 0.01
  const double* rec;          // [K + 2][N][3 D + 1]
  DlyEntry* part;             // [segment chunks][ntb][a_end - a_begin][S + 1]
  unsigned long long* n_solved;  // segments that reached the quartic
};

__device__ inline DlyEntry dly_empty() { return DlyEntry{SEP_INF, SEP_NO_ROW, 0.0, 0ULL}; }

// an upper bound of the distance whose square is m (the rounding of the root stays below the 1e-15)
__device__ inline double dly_bound(double m) { return sqrt(fmax(m, 0.0)) * (1.0 + 1e-15); }

template <int D>
__global__ __launch_bounds__(SEP_THREADS) void dly_pass_kernel(DlyArgs a) {
  constexpr int NC = 3 * D + 1;
  __shared__ double sm[NC][2 * SEP_TILE];            // component planes; [0, 64): the a side, [64, 128): the b side
  __shared__ unsigned short queue[SEP_TILE * SEP_TILE];
  __shared__ unsigned int q_count;
  __shared__ double ub[SEP_TILE];                    // per a of the tile: an upper bound of entry (a, s)'s final distance
  __shared__ double res_m[SEP_THREADS], res_t[SEP_THREADS];  // one round of phase B results ...
  __shared__ unsigned short res_id[SEP_THREADS];             // ... and their pairs (al << 6 | bl)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, K = a.K;
  const int ta = blockIdx.x / a.ntb, tb = blockIdx.x % a.ntb;
  const int a0 = a.a_begin + ta * SEP_TILE, b0 = tb * SEP_TILE;
  const int n_a = a.a_end - a.a_begin;
  const int s_begin = blockIdx.y * a.lc, s_end = min(a.S + 1, s_begin + a.lc);
  const int g_lo = blockIdx.z * a.gc;

  // this thread's b (fixed: b0 + lane) and its 16 a's (a0 + wave + 4 x): bit x says that the ordered pair exists
  unsigned int valid = 0;
  for (int x = 0; x < SEP_STEPS; ++x) {
    const int va = a0 + wave + 4 * x, vb = b0 + lane;
    if (va < a.a_end && vb < N && va != vb) valid |= 1u << x;
  }
  auto rec_a = [&](int g, int s) { return max(g - s, -1) + 1; };
  auto rec_b = [&](int g) { return min(g, K) + 1; };

  unsigned long long n_solved = 0;  // thread 0 only
  DlyStage<NC> stage;
  for (int s = s_begin; s < s_end; ++s) {
    const int g_hi = min(g_lo + a.gc, K + s);
    DlyEntry own = dly_empty();  // wave 0: entry (a0 + lane, s) over this workgroup's b tile and segments
    if (tid < SEP_TILE) ub[tid] = SEP_INF;  // (seeded and read after the first barriers of the loop)
    if (g_lo < g_hi) stage.fetch2(a.rec, rec_a(g_lo, s), rec_b(g_lo), N, a0, b0, tid);
    for (int g = g_lo; g < g_hi; ++g) {
      __syncthreads();  // (the previous segment's phase B has read sm, the queue and the results)
      stage.stash(sm, tid);
      if (tid == 0) q_count = 0;
      __syncthreads();
      if (g + 1 < g_hi) stage.fetch2(a.rec, rec_a(g + 1, s), rec_b(g + 1), N, a0, b0, tid);  // in flight during the arithmetic

      // ---- the first segment seeds U: the smallest sampled d.d of the tile's pairs of a (the bits of their quartics' c0, an
      // upper bound of their computed minima; the pair that attains it passes the test below: d.d <= U^2 <= T^2) --------------
      if (g == g_lo) {  // uniform over the workgroup
#pragma unroll
        for (int x = 0; x < SEP_STEPS; ++x) {
          double pb0[D];
#pragma unroll
          for (int d = 0; d < D; ++d) pb0[d] = sm[d][SEP_TILE + lane];
          const double ss = (valid >> x) & 1u ? tile_dd<D>(sm, wave + 4 * x, pb0) : SEP_INF;
          const double v = wave_min_f64(ss);
          if (lane == 0 && v < SEP_INF) ub[wave + 4 * x] = dly_bound(v);  // (one wave per a: no other writer)
        }
        __syncthreads();
      }

      // ---- phase A: the skip test of the check (its derivation: scp_separation.hip) with T = max(thr, U_(a, s)) ---------
      double pb[D];
#pragma unroll
      for (int d = 0; d < D; ++d) pb[d] = sm[d][SEP_TILE + lane];
      const double rho_b = sm[3 * D][SEP_TILE + lane];
#pragma unroll
      for (int x = 0; x < SEP_STEPS; ++x) {
        const int al = wave + 4 * x;
        const double ss = tile_dd<D>(sm, al, pb);
        if (!((valid >> x) & 1u)) continue;
        const double reach = fmax(a.thr, ub[al]) + (sm[3 * D][al] + rho_b);
        if (!(ss > reach * reach * SEP_SKIP_FACTOR)) {
          const unsigned int slot = atomicAdd(&q_count, 1u);
          queue[slot] = (unsigned short)((al << 6) | lane);
        }
      }
      __syncthreads();

      // ---- phase B: the queued segments, dense over the threads, in rounds of one segment per thread ------------------
      const unsigned int n_q = q_count;
      if (tid == 0) n_solved += n_q;
      for (unsigned int base = 0; base < n_q; base += SEP_THREADS) {
        const unsigned int e = base + tid;
        if (e < n_q) {
          const unsigned int id = queue[e];
          double m, t;
          quartic_min(tile_quartic<D>(sm, (int)(id >> 6), (int)(id & 63)), a.h, m, t);
          res_m[tid] = m;
          res_t[tid] = t;
          res_id[tid] = (unsigned short)id;
        }
        __syncthreads();
        const unsigned int n_r = min((unsigned int)SEP_THREADS, n_q - base);
        if (wave == 0) {  // the owners: every result of the round that names my a
          for (unsigned int r = 0; r < n_r; ++r) {
            const unsigned int id = res_id[r];
            if ((int)(id >> 6) == lane) {
              const double m = res_m[r];
              fold_min(own.m, own.key, own.t, m, ((unsigned long long)g << 32) | (unsigned long long)(b0 + (int)(id & 63)), res_t[r]);
              own.n_viol += sep_violates(m, a.thr) ? 1ULL : 0ULL;
            }
          }
        }
        if (base + SEP_THREADS < n_q) __syncthreads();  // (the next round overwrites the results)
      }
      if (wave == 0 && own.key != SEP_NO_ROW) ub[lane] = dly_bound(own.m);  // (read after the next segment's barriers)
    }
    if (tid < SEP_TILE && a0 + tid < a.a_end)
      a.part[(((int64_t)blockIdx.z * a.ntb + tb) * n_a + (a0 - a.a_begin + tid)) * (a.S + 1) + s] = own;
  }
  if (tid == 0 && n_solved) atomicAdd(a.n_solved, n_solved);
}

// one thread per entry (a, s): fold the partials of all segment chunks and b tiles (any order gives the same result)
__global__ __launch_bounds__(256) void dly_finish_kernel(DlyArgs a, int n_gchunks, scp_delay_margin* __restrict__ out) {
  const int64_t n_ent = (int64_t)(a.a_end - a.a_begin) * (a.S + 1);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ent) return;
  DlyEntry p = dly_empty();
  for (int64_t x = 0; x < (int64_t)n_gchunks * a.ntb; ++x) {
    const DlyEntry o = a.part[x * n_ent + e];
    fold_min(p.m, p.key, p.t, o.m, o.key, o.t);
    p.n_viol += o.n_viol;
  }
  scp_delay_margin r;
  r.min_dist = p.key == SEP_NO_ROW ? SEP_INF : sqrt(fmax(p.m, 0.0));  // crossing vehicles: f a few ulps below 0
  r.t_min = p.t;
  r.partner = (uint32_t)(p.key & 0xFFFFFFFFULL);  // (no pair: both UINT32_MAX)
  r.segment = (uint32_t)(p.key >> 32);
  r.n_violating = p.n_viol;
  out[e] = r;
}

}  // namespace

extern "C" int scp_delay_margins(scp_ctx* ctx, int N, int K, int D, double h, double R, int a_begin, int a_end, int max_lag,
                                 const double* pos, const double* vel, const double* acc, scp_delay_margin* out) {
  const char* who = "scp_delay_margins";
  if (!ctx) return SCP_ERR_INVALID;
  int rc = scp_check_pair_range(ctx, N, K, D, 0, 0);
  if (rc) return rc;
  SCP_REQUIRE(ctx, a_begin >= 0 && a_end >= a_begin && a_end <= N, "%s: bad vehicle range [%d, %d) of %d", who, a_begin, a_end, N);
  SCP_REQUIRE(ctx, max_lag >= 0 && max_lag <= K, "%s: bad lag range: max_lag=%d, K=%d", who, max_lag, K);
  SCP_REQUIRE(ctx, pos && vel && acc && out, "%s: null pointer", who);
  SCP_REQUIRE(ctx, h > 0.0 && h < SEP_INF, "%s: bad time step h=%g", who, h);
  const int n_a = a_end - a_begin;
  const DlyPlan plan = dly_plan(ctx, N, K, n_a, max_lag, ctx->delay_lag_chunk, ctx->delay_time_chunk);
  SCP_REQUIRE(ctx, plan.n_tiles < ((int64_t)1 << 31) && plan.n_lchunks <= 65535 && plan.n_gchunks <= 65535,
              "%s: %lld tiles x %d lag chunks x %d segment chunks exceed the grid; shard the vehicle range", who,
              (long long)plan.n_tiles, plan.n_lchunks, plan.n_gchunks);
  const size_t rec_bytes = ((size_t)N * (K + 2) * (3 * D + 1) * sizeof(double) + 63) & ~(size_t)63;
  const size_t part_bytes = (size_t)plan.n_gchunks * plan.ntb * n_a * (max_lag + 1) * sizeof(DlyEntry);
  rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, rec_bytes + part_bytes);
  if (rc) return rc;

  DlyArgs a{};
  a.N = N; a.K = K; a.D = D; a.S = max_lag;
  a.a_begin = a_begin; a.a_end = a_end;
  a.ntb = plan.ntb; a.lc = plan.lc; a.gc = plan.gc;
  a.h = h; a.thr = R - 0.01;
  a.rec = (const double*)ctx->sep_ws;
  a.part = (DlyEntry*)((char*)ctx->sep_ws + rec_bytes);
  a.n_solved = ctx->delay_solved;

  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  hipLaunchKernelGGL(dly_prep_kernel, dim3(scp_cdiv((int64_t)N * (K + 2), 256)), dim3(256), 0, ctx->stream, N, K, D, h, pos, vel,
                     acc, (double*)ctx->sep_ws, a.n_solved);
  if (n_a > 0) {
    hipLaunchKernelGGL(D == 2 ? dly_pass_kernel<2> : dly_pass_kernel<3>,
                       dim3((unsigned)plan.n_tiles, (unsigned)plan.n_lchunks, (unsigned)plan.n_gchunks), dim3(SEP_THREADS), 0,
                       ctx->stream, a);
    hipLaunchKernelGGL(dly_finish_kernel, dim3(scp_cdiv((int64_t)n_a * (max_lag + 1), 256)), dim3(256), 0, ctx->stream, a,
                       plan.n_gchunks, out);
  }
  rc = sep_end(ctx);
  if (rc) return rc;
  ctx->delay_solved_ran = true;
  return SCP_OK;
}

// segments of the latest scp_delay_margins of this ctx that reached the quartic (developer figure; synchronises)
extern "C" int scp_ctx_last_delay_solved(scp_ctx* ctx, uint64_t* n) {
  if (!ctx || !n) return SCP_ERR_INVALID;
  if (!ctx->delay_solved_ran) return scp_fail(ctx, SCP_ERR_STATE, "scp_delay_margins has not run yet");
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemcpy(n, ctx->delay_solved, sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SCP_OK;
}
