// Staggered starts (scp_lag_conflicts, scp_schedule_starts, scp_schedule_starts_batch; include/scp_hip.h): leave every plan as it is and start some
// vehicles a few steps later.
//
// The MASK pass keeps what scp_delay_margins reduces away: for every ORDERED pair (a, b) and every lag s = 0 .. S, bit s of
// mask[a][b] says whether some global segment g of the fleet in which a starts s steps late violates the threshold against
// b -- record max(g - s, -1) of a against record min(g, K) of b, the segments entry (a, s) of scp_delay_margins counts in
// n_violating, decided on the same bits: the records, the two-sided fetch and the plan are scp_delay_device.h's, the
// per-segment arithmetic, the skip test and the violation test scp_separation_device.h's.
//
// Exclusion: a segment is dropped without its quartic only if its distance provably exceeds T = R - 0.01 (the check's skip
// test; its derivation: scp_separation.hip).  No minimum is wanted, so there is no running bound.  A pair whose bit of the
// lag is already set in this workgroup is not examined again.  Neither shows in the mask: a dropped segment is no violation,
// and a skipped one could only set a bit that is set.
//
// Kernels, all on the ctx stream (launches are the only synchronisation; no workgroup waits for another):
//   dly_prep_kernel   the K + 2 records per vehicle and the solved count to 0 (a memset zeroes the mask before it);
//   lagc_pass_kernel  one workgroup per (64 x 64 tile of ordered pairs a != b, chunk of lags, chunk of global segments): per lag
//                     and segment phase A (one reach comparison per pair) and phase B (the queued quartics, dense over the
//                     threads; a violation sets the pair's bit of an LDS bitmap of the lag).  After a lag every thread moves
//                     the bits of its 16 pairs into bit s of 16 words in registers; at the end the non-zero words are ORed
//                     into the mask -- integer ORs only, so the bytes do not depend on how lags and segments are cut.
//
// The SCHEDULE kernel is one workgroup that runs N dependent steps.  Step t places v = order[t] at the smallest d in [0, S]
// that is not forbidden by a vehicle placed before it.  Instead of reducing over the placed vehicles in every step, the
// workgroup keeps that OR for every vehicle that is still to come: forbid[w], one word in LDS per vehicle, and placing u at
// d_u ORs into every pending w
//     mask[w][u] << d_u                                       the delays d >= d_u of w: bit d - d_u of mask[w][u];
//     (bitrev(mask[u][w]) >> (63 - d_u)) & ((1 << d_u) - 1)   the delays d <  d_u of w: bit d_u - d of mask[u][w].
// The OR is associative and commutative, so forbid[v] at step t is the reduction of the rule, and every thread reads the one
// word forbid[v] and derives d itself: one barrier per step and no reduction tree.  An unplaced vehicle ORs nothing.  All
// shifts go through shl64 / shr64, which shift in two halves: no shift count above 32 occurs.
//
// The order is the only free parameter of that rule.  The BATCH kernel (scp_schedule_starts_batch) runs the same steps for B
// candidate orders at once, one workgroup of 256 or 1024 threads per candidate with its own forbid[] / pending[] in LDS; the
// masks are read only and shared.  Thread 0 of every workgroup packs (n_unplaced, max_delay, total_delay, b) -- or total before
// max -- into one word whose integer order is the key's lexicographic order and takes one atomicMin on a device word; the host
// decodes the best candidate from it.  A second word takes the minimum over the candidates that are no permutation.
#include "scp_assign_device.h"
#include "scp_delay_device.h"

namespace {

struct LagcArgs {
  int N, K, S;                // S: the largest lag
  int a_begin, a_end;         // the vehicles whose rows the call computes
  int ntb;                    // tiles along b: blockIdx.x = (a tile) * ntb + (b tile)
  int lc, gc;                 // lags (blockIdx.y) and global segments (blockIdx.z) per workgroup
  double h, thr;              // thr = R - 0.01
  const double* rec;          // [K + 2][N][3 D + 1]
  unsigned long long* mask;   // [a_end - a_begin][N], zero at the launch
  unsigned long long* n_solved;  // segments that reached the quartic
};

template <int D>
__global__ __launch_bounds__(SEP_THREADS) void lagc_pass_kernel(LagcArgs a) {
  constexpr int NC = 3 * D + 1;
  __shared__ double sm[NC][2 * SEP_TILE];            // component planes; [0, 64): the a side, [64, 128): the b side
  __shared__ unsigned short queue[SEP_TILE * SEP_TILE];
  __shared__ unsigned int q_count;
  __shared__ unsigned long long hit[SEP_TILE];       // per a of the tile: bit bl says that (a, b0 + bl) violates at this lag

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, K = a.K;
  const int ta = blockIdx.x / a.ntb, tb = blockIdx.x % a.ntb;
  const int a0 = a.a_begin + ta * SEP_TILE, b0 = tb * SEP_TILE;
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
  unsigned long long word[SEP_STEPS];  // the mask words of this thread's pairs: the lags of this workgroup
#pragma unroll
  for (int x = 0; x < SEP_STEPS; ++x) word[x] = 0ULL;
  DlyStage<NC> stage;
  for (int s = s_begin; s < s_end; ++s) {
    const int g_hi = min(g_lo + a.gc, K + s);
    if (g_lo >= g_hi) continue;  // (uniform: this lag's fleet ends before the chunk; a later lag's may reach into it)
    if (tid < SEP_TILE) hit[tid] = 0ULL;  // (read after the first barriers of the loop)
    stage.fetch2(a.rec, rec_a(g_lo, s), rec_b(g_lo), N, a0, b0, tid);
    for (int g = g_lo; g < g_hi; ++g) {
      __syncthreads();  // (the previous segment's phase B has read sm and the queue and set its bits)
      stage.stash(sm, tid);
      if (tid == 0) q_count = 0;
      __syncthreads();
      if (g + 1 < g_hi) stage.fetch2(a.rec, rec_a(g + 1, s), rec_b(g + 1), N, a0, b0, tid);  // in flight during the arithmetic

      // ---- phase A: the skip test of the check (its derivation: scp_separation.hip) with T = thr; a pair that already
      // violates at this lag is done ----------------------------------------------------------------------------------------
      double pb[D];
#pragma unroll
      for (int d = 0; d < D; ++d) pb[d] = sm[d][SEP_TILE + lane];
      const double rho_b = sm[3 * D][SEP_TILE + lane];
#pragma unroll
      for (int x = 0; x < SEP_STEPS; ++x) {
        const int al = wave + 4 * x;
        const double ss = tile_dd<D>(sm, al, pb);
        if (!((valid >> x) & 1u)) continue;
        if ((hit[al] >> lane) & 1ULL) continue;
        const double reach = a.thr + (sm[3 * D][al] + rho_b);
        if (!(ss > reach * reach * SEP_SKIP_FACTOR)) {
          const unsigned int slot = atomicAdd(&q_count, 1u);
          queue[slot] = (unsigned short)((al << 6) | lane);
        }
      }
      __syncthreads();

      // ---- phase B: the queued segments, dense over the threads, one segment per thread and round ------------------------
      const unsigned int n_q = q_count;
      if (tid == 0) n_solved += n_q;
      for (unsigned int e = tid; e < n_q; e += SEP_THREADS) {
        const unsigned int id = queue[e];
        double m, t;
        quartic_min(tile_quartic<D>(sm, (int)(id >> 6), (int)(id & 63)), a.h, m, t);
        if (sep_violates(m, a.thr)) atomicOr(&hit[id >> 6], 1ULL << (id & 63));
      }
    }
    __syncthreads();  // (the last segment's bits)
#pragma unroll
    for (int x = 0; x < SEP_STEPS; ++x)
      if ((hit[wave + 4 * x] >> lane) & 1ULL) word[x] |= 1ULL << s;
    __syncthreads();  // (before the next lag clears the bitmap)
  }
#pragma unroll
  for (int x = 0; x < SEP_STEPS; ++x)
    if (((valid >> x) & 1u) && word[x])
      atomicOr(a.mask + ((int64_t)(a0 + wave + 4 * x - a.a_begin) * N + (b0 + lane)), word[x]);
  if (tid == 0 && n_solved) atomicAdd(a.n_solved, n_solved);
}

// ---- the schedule ---------------------------------------------------------------------------------------------------------------
constexpr int STG_MAXN = 16384;
constexpr int STG_MAXB = 65535;  // candidates of one scp_schedule_starts_batch (16 bits of the key)
constexpr int STG_THREADS = 1024;
constexpr unsigned long long STG_ALL = 0xFFFFFFFFFFFFFFFFULL;

// x << n and x >> n for n in [0, 64], in two halves: no shift count above 32
__device__ __host__ inline unsigned long long shl64(unsigned long long x, int n) { return (x << (n >> 1)) << (n - (n >> 1)); }
__device__ __host__ inline unsigned long long shr64(unsigned long long x, int n) { return (x >> (n >> 1)) >> (n - (n >> 1)); }

// what placing u at d_u forbids to w: m_wu = mask[w][u], m_uw = mask[u][w]
__device__ inline unsigned long long stg_forbidden(unsigned long long m_wu, unsigned long long m_uw, int d_u) {
  const unsigned long long later = shl64(m_wu, d_u);  // d >= d_u
  const unsigned long long earlier = shr64(__brevll(m_uw), 63 - d_u) & (shl64(1ULL, d_u) - 1ULL);  // d < d_u (none for d_u = 0)
  return later | earlier;
}

// One workgroup.  LDS: forbid[N] words, then pending[ceil(N / 32)] (bit v: v has not had its step yet).
__global__ __launch_bounds__(STG_THREADS) void stg_schedule_kernel(int N, int S, const unsigned long long* __restrict__ mask,
                                                                   const int32_t* __restrict__ order,
                                                                   int32_t* __restrict__ delay,
                                                                   scp_start_schedule_stats* __restrict__ stats,
                                                                   int* __restrict__ bad_order) {
  extern __shared__ unsigned long long stg_lds[];
  unsigned long long* forbid = stg_lds;
  unsigned int* pending = (unsigned int*)(stg_lds + N);
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int n_words = (N + 31) / 32;
  const unsigned long long beyond = ~(shl64(1ULL, S + 1) - 1ULL);  // the delays above S: never allowed

  // ---- `order` is a permutation: every entry in range, every vehicle named once -----------------------------------------------
  if (tid == 0) bad = 0;
  for (int x = tid; x < n_words; x += STG_THREADS) pending[x] = 0u;
  for (int w = tid; w < N; w += STG_THREADS) forbid[w] = beyond;
  __syncthreads();
  for (int t = tid; t < N; t += STG_THREADS) {
    const int v = order ? order[t] : t;
    if (v < 0 || v >= N) {
      bad = 1;
    } else {
      const unsigned int bit = 1u << (v & 31);
      if (atomicOr(&pending[v >> 5], bit) & bit) bad = 1;
    }
  }
  __syncthreads();
  if (bad) {  // (uniform) nothing is scheduled
    if (tid == 0) *bad_order = 1;
    return;
  }

  int n_delayed = 0, n_unplaced = 0, max_delay = 0, first_unplaced = -1;  // thread 0 only
  long long total = 0;
  for (int t = 0; t < N; ++t) {
    const int v = order ? order[t] : t;
    const unsigned long long f = forbid[v];  // complete: the steps before this one ended with a barrier
    const int d = f == STG_ALL ? -1 : __ffsll((long long)~f) - 1;
    if (tid == 0) {
      delay[v] = d;
      pending[v >> 5] &= ~(1u << (v & 31));  // (read again only after the barrier: this step excludes v itself)
      if (d < 0) {
        ++n_unplaced;
        if (first_unplaced < 0) first_unplaced = v;
      } else {
        n_delayed += d > 0;
        max_delay = max(max_delay, d);
        total += d;
      }
    }
    if (d >= 0) {
      for (int w = tid; w < N; w += STG_THREADS) {
        if (w == v || !((pending[w >> 5] >> (w & 31)) & 1u)) continue;
        const unsigned long long fw = forbid[w];
        if (fw == STG_ALL) continue;  // nothing left to forbid
        forbid[w] = fw | stg_forbidden(mask[(int64_t)w * N + v], mask[(int64_t)v * N + w], d);
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    scp_start_schedule_stats st;
    st.n_delayed = n_delayed;
    st.n_unplaced = n_unplaced;
    st.max_delay = max_delay;
    st.first_unplaced = first_unplaced;
    st.total_delay = total;
    st.reserved[0] = st.reserved[1] = st.reserved[2] = 0;
    *stats = st;
  }
}

// ---- the schedules of many orders ---------------------------------------------------------------------------------------------
// The steps of stg_schedule_kernel for a workgroup of THREADS threads and an order that is given; LDS as there.  (Its own body:
// with the steps in a function of both, stg_schedule_kernel no longer compiled to the instructions it had.)  Returns false
// (uniform) and schedules nothing if `order` is no permutation; otherwise thread 0 holds the stats in `st` at the end.
// mask_t: NULL, or the transposed masks (mask_t[v][w] = mask[w][v]): column v of a step is then read from a row.
template <int THREADS>
__device__ __forceinline__ bool stg_batch_one(int N, int S, const unsigned long long* __restrict__ mask,
                                              const unsigned long long* __restrict__ mask_t,
                                              const int32_t* __restrict__ order, int32_t* __restrict__ delay,
                                              scp_start_schedule_stats& st) {
  extern __shared__ unsigned long long stg_lds[];
  unsigned long long* forbid = stg_lds;
  unsigned int* pending = (unsigned int*)(stg_lds + N);
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int n_words = (N + 31) / 32;
  const unsigned long long beyond = ~(shl64(1ULL, S + 1) - 1ULL);  // the delays above S: never allowed

  // ---- `order` is a permutation: every entry in range, every vehicle named once -----------------------------------------------
  if (tid == 0) bad = 0;
  for (int x = tid; x < n_words; x += THREADS) pending[x] = 0u;
  for (int w = tid; w < N; w += THREADS) forbid[w] = beyond;
  __syncthreads();
  for (int t = tid; t < N; t += THREADS) {
    const int v = order[t];
    if (v < 0 || v >= N) {
      bad = 1;
    } else {
      const unsigned int bit = 1u << (v & 31);
      if (atomicOr(&pending[v >> 5], bit) & bit) bad = 1;
    }
  }
  __syncthreads();
  if (bad) return false;  // (uniform) nothing is scheduled

  int n_delayed = 0, n_unplaced = 0, max_delay = 0, first_unplaced = -1;  // thread 0 only
  long long total = 0;
  for (int t = 0; t < N; ++t) {
    const int v = order[t];
    const unsigned long long f = forbid[v];  // complete: the steps before this one ended with a barrier
    const int d = f == STG_ALL ? -1 : __ffsll((long long)~f) - 1;
    if (tid == 0) {
      delay[v] = d;
      pending[v >> 5] &= ~(1u << (v & 31));  // (read again only after the barrier: this step excludes v itself)
      if (d < 0) {
        ++n_unplaced;
        if (first_unplaced < 0) first_unplaced = v;
      } else {
        n_delayed += d > 0;
        max_delay = max(max_delay, d);
        total += d;
      }
    }
    if (d >= 0) {
      const unsigned long long* column = mask_t ? mask_t + (int64_t)v * N : mask + v;  // mask[w][v] = column[w * stride]
      const int64_t stride = mask_t ? 1 : N;
      for (int w = tid; w < N; w += THREADS) {
        if (w == v || !((pending[w >> 5] >> (w & 31)) & 1u)) continue;
        const unsigned long long fw = forbid[w];
        if (fw == STG_ALL) continue;  // nothing left to forbid
        forbid[w] = fw | stg_forbidden(column[w * stride], mask[(int64_t)v * N + w], d);
      }
    }
    __syncthreads();
  }
  st.n_delayed = n_delayed;
  st.n_unplaced = n_unplaced;
  st.max_delay = max_delay;
  st.first_unplaced = first_unplaced;
  st.total_delay = total;
  st.reserved[0] = st.reserved[1] = st.reserved[2] = 0;
  return true;
}

// The key of a candidate under an objective as ONE word whose integer order is the lexicographic order of the rule:
// n_unplaced <= 2^14 (15 bits), max_delay <= 63 (6 bits), total_delay <= 63 * 16384 < 2^20 (20 bits), b < 2^16.
__device__ __host__ inline unsigned long long stg_key(const scp_start_schedule_stats& st, int objective, unsigned int b) {
  const unsigned long long u = (unsigned long long)st.n_unplaced, m = (unsigned long long)st.max_delay,
                           t = (unsigned long long)st.total_delay;
  return (u << 42) | (objective == 0 ? (m << 36) | (t << 16) : (t << 22) | (m << 16)) | b;
}

// out[c][r] = in[r][c] of N x N words: 64 x 64 tiles through LDS (a column of padding: the reads by column spread over the banks)
__global__ __launch_bounds__(256) void stg_transpose_kernel(int N, const unsigned long long* __restrict__ in,
                                                            unsigned long long* __restrict__ out) {
  __shared__ unsigned long long tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  for (int y = wave; y < 64; y += 4)
    if (r0 + y < N && c0 + lane < N) tile[y][lane] = in[(int64_t)(r0 + y) * N + (c0 + lane)];
  __syncthreads();
  for (int y = wave; y < 64; y += 4)
    if (c0 + y < N && r0 + lane < N) out[(int64_t)(c0 + y) * N + (r0 + lane)] = tile[lane][y];
}

// One workgroup per candidate order; no workgroup waits for another.  words[0]: the smallest key, words[1]: the lowest
// candidate that is no permutation; both all ones at the launch.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void stg_batch_kernel(int N, int S, const unsigned long long* __restrict__ mask,
                                                            const unsigned long long* __restrict__ mask_t,
                                                            const int32_t* __restrict__ orders, int objective,
                                                            int32_t* __restrict__ delay,
                                                            scp_start_schedule_stats* __restrict__ stats,
                                                            unsigned long long* __restrict__ words) {
  const unsigned int b = blockIdx.x;
  scp_start_schedule_stats st;
  if (!stg_batch_one<THREADS>(N, S, mask, mask_t, orders + (int64_t)b * N, delay + (int64_t)b * N, st)) {
    if (threadIdx.x == 0) atomicMin(words + 1, (unsigned long long)b);
    return;
  }
  if (threadIdx.x == 0) {
    stats[b] = st;
    atomicMin(words, stg_key(st, objective, b));
  }
}

}  // namespace

extern "C" int scp_lag_conflicts(scp_ctx* ctx, int N, int K, int D, double h, double R, int a_begin, int a_end, int max_lag,
                                 const double* pos, const double* vel, const double* acc, uint64_t* mask) {
  const char* who = "scp_lag_conflicts";
  if (!ctx) return SCP_ERR_INVALID;
  int rc = scp_check_pair_range(ctx, N, K, D, 0, 0);
  if (rc) return rc;
  SCP_REQUIRE(ctx, a_begin >= 0 && a_end >= a_begin && a_end <= N, "%s: bad vehicle range [%d, %d) of %d", who, a_begin, a_end, N);
  SCP_REQUIRE(ctx, max_lag >= 0 && max_lag <= K && max_lag <= 63, "%s: bad lag range: max_lag=%d, K=%d (at most min(K, 63))", who,
              max_lag, K);
  SCP_REQUIRE(ctx, pos && vel && acc && mask, "%s: null pointer", who);
  SCP_REQUIRE(ctx, h > 0.0 && h < SEP_INF, "%s: bad time step h=%g", who, h);
  const int n_a = a_end - a_begin;
  const DlyPlan plan = dly_plan(ctx, N, K, n_a, max_lag, ctx->lagc_lag_chunk, ctx->lagc_time_chunk);
  SCP_REQUIRE(ctx, plan.n_tiles < ((int64_t)1 << 31) && plan.n_lchunks <= 65535 && plan.n_gchunks <= 65535,
              "%s: %lld tiles x %d lag chunks x %d segment chunks exceed the grid; shard the vehicle range", who,
              (long long)plan.n_tiles, plan.n_lchunks, plan.n_gchunks);
  const size_t rec_bytes = ((size_t)N * (K + 2) * (3 * D + 1) * sizeof(double) + 63) & ~(size_t)63;
  rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, rec_bytes);
  if (rc) return rc;

  LagcArgs a{};
  a.N = N; a.K = K; a.S = max_lag;
  a.a_begin = a_begin; a.a_end = a_end;
  a.ntb = plan.ntb; a.lc = plan.lc; a.gc = plan.gc;
  a.h = h; a.thr = R - 0.01;
  a.rec = (const double*)ctx->sep_ws;
  a.mask = (unsigned long long*)mask;
  a.n_solved = ctx->lag_solved;

  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  hipLaunchKernelGGL(dly_prep_kernel, dim3(scp_cdiv((int64_t)N * (K + 2), 256)), dim3(256), 0, ctx->stream, N, K, D, h, pos, vel,
                     acc, (double*)ctx->sep_ws, a.n_solved);
  if (n_a > 0) {
    SCP_HIP_CHECK(ctx, hipMemsetAsync(mask, 0, (size_t)n_a * N * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(D == 2 ? lagc_pass_kernel<2> : lagc_pass_kernel<3>,
                       dim3((unsigned)plan.n_tiles, (unsigned)plan.n_lchunks, (unsigned)plan.n_gchunks), dim3(SEP_THREADS), 0,
                       ctx->stream, a);
  }
  rc = sep_end(ctx);
  if (rc) return rc;
  ctx->lag_solved_ran = true;
  return SCP_OK;
}

// segments of the latest scp_lag_conflicts of this ctx that reached the quartic (developer figure; synchronises)
extern "C" int scp_ctx_last_lag_solved(scp_ctx* ctx, uint64_t* n) {
  if (!ctx || !n) return SCP_ERR_INVALID;
  if (!ctx->lag_solved_ran) return scp_fail(ctx, SCP_ERR_STATE, "scp_lag_conflicts has not run yet");
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemcpy(n, ctx->lag_solved, sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SCP_OK;
}

extern "C" int scp_schedule_starts(scp_ctx* ctx, int N, int max_lag, const uint64_t* mask, const int32_t* order, int32_t* delay,
                                   scp_start_schedule_stats* stats) {
  const char* who = "scp_schedule_starts";
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, mask && delay && stats, "%s: null pointer", who);
  SCP_REQUIRE(ctx, N >= 1 && N <= STG_MAXN, "%s: N = %d (need 1 <= N <= %d)", who, N, STG_MAXN);
  SCP_REQUIRE(ctx, max_lag >= 0 && max_lag <= 63, "%s: max_lag = %d (need 0 <= max_lag <= 63)", who, max_lag);
  static_assert(sizeof(scp_start_schedule_stats) == 48, "scp_start_schedule_stats is 48 bytes");
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = asg_host_flag(ctx)) return rc;
  const size_t lds = sizeof(unsigned long long) * (size_t)N + sizeof(unsigned int) * (size_t)((N + 31) / 32);
  if (lds > 48 * 1024)
    SCP_HIP_CHECK(ctx, scp_raise_lds_limit(ctx->device, reinterpret_cast<const void*>(stg_schedule_kernel), lds));
  hipStream_t st = ctx->stream;
  volatile int* hflag = ctx->h_gen_flag;
  *hflag = 0;
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, st));
  stg_schedule_kernel<<<1, STG_THREADS, lds, st>>>(N, max_lag, (const unsigned long long*)mask, order, delay, stats,
                                                   ctx->d_gen_flag);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && ctx->timing) e = hipEventRecord(ctx->pair_ev1, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return scp_fail(ctx, SCP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  SCP_REQUIRE(ctx, *hflag == 0, "%s: order is not a permutation of 0 .. N-1", who);
  return SCP_OK;
}

// B candidate orders on the same masks in one launch, one workgroup each, and the candidate with the smallest key.
extern "C" int scp_schedule_starts_batch(scp_ctx* ctx, int N, int max_lag, const uint64_t* mask, int B, const int32_t* orders,
                                         int objective, int32_t* delay, scp_start_schedule_stats* stats, int32_t* best) {
  const char* who = "scp_schedule_starts_batch";
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, mask && orders && delay && stats && best, "%s: null pointer", who);
  SCP_REQUIRE(ctx, N >= 1 && N <= STG_MAXN, "%s: N = %d (need 1 <= N <= %d)", who, N, STG_MAXN);
  SCP_REQUIRE(ctx, max_lag >= 0 && max_lag <= 63, "%s: max_lag = %d (need 0 <= max_lag <= 63)", who, max_lag);
  SCP_REQUIRE(ctx, B >= 1 && B <= STG_MAXB, "%s: B = %d (need 1 <= B <= %d)", who, B, STG_MAXB);
  SCP_REQUIRE(ctx, objective == 0 || objective == 1, "%s: objective = %d (need 0: makespan or 1: total)", who, objective);
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = asg_host_flag(ctx)) return rc;
  // up to 256 vehicles no thread beyond the first 256 would have a vehicle, and a step's barrier spans 4 waves instead of 16
  // (unmeasured); above, the loads of a step are what it waits for and 1024 threads issue them at once (at 1024 and 4096
  // vehicles 256 threads take 1.5 and 1.1 times as long: profiles/stagger_search.txt)
  const int threads = ctx->stg_batch_threads ? ctx->stg_batch_threads : (N <= 256 ? 256 : 1024);
  const void* kernel = threads == 256 ? reinterpret_cast<const void*>(stg_batch_kernel<256>)
                                      : reinterpret_cast<const void*>(stg_batch_kernel<1024>);
  const size_t lds = sizeof(unsigned long long) * (size_t)N + sizeof(unsigned int) * (size_t)((N + 31) / 32);
  if (lds > 48 * 1024) SCP_HIP_CHECK(ctx, scp_raise_lds_limit(ctx->device, kernel, lds));
  // the transposed copy of the masks, in the workspace of the continuous-time passes: with it a step reads two rows instead of a
  // row and a column.  From 16 candidates on the call is faster with it, its launch included (1024 vehicles: 0.87 against
  // 1.19 ms at B = 16, 0.88 against 1.46 ms at B = 256; 4096: 8.8 against 13.8 ms and 9.7 against 38 ms); below 16: unmeasured
  unsigned long long* mask_t = nullptr;
  if (ctx->stg_batch_transposed < 0 ? B >= 16 : ctx->stg_batch_transposed) {
    if (const int rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)N * N * sizeof(unsigned long long)))
      return rc;
    mask_t = (unsigned long long*)ctx->sep_ws;
  }
  hipStream_t st = ctx->stream;
  unsigned long long* words = (unsigned long long*)(ctx->d_ticket + 4);       // [0]: smallest key, [1]: lowest bad candidate
  unsigned long long* hwords = (unsigned long long*)(ctx->h_gen_flag + 4);    // their pinned host copy
  const unsigned long long* mk = (const unsigned long long*)mask;
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, st));
  SCP_HIP_CHECK(ctx, hipMemsetAsync(words, 0xFF, 2 * sizeof(unsigned long long), st));
  if (mask_t) stg_transpose_kernel<<<dim3(scp_cdiv(N, 64), scp_cdiv(N, 64)), 256, 0, st>>>(N, mk, mask_t);
  if (threads == 256)
    stg_batch_kernel<256><<<B, 256, lds, st>>>(N, max_lag, mk, mask_t, orders, objective, delay, stats, words);
  else
    stg_batch_kernel<1024><<<B, 1024, lds, st>>>(N, max_lag, mk, mask_t, orders, objective, delay, stats, words);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && ctx->timing) e = hipEventRecord(ctx->pair_ev1, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hwords, words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return scp_fail(ctx, SCP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  SCP_REQUIRE(ctx, hwords[1] == STG_ALL, "%s: candidate %llu is not a permutation of 0 .. N-1", who, hwords[1]);
  *best = (int32_t)(hwords[0] & 0xFFFFULL);
  return SCP_OK;
}
