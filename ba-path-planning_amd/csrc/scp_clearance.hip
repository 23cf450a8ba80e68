// Clearance profile (scp_clearance_profile, include/scp_hip.h): the K x pairs quartic minimisation of scp_check_separation,
// reduced along the other two axes -- for every VEHICLE the closest approach over all partners and segments, for every time
// STEP the closest approach over all pairs --, plus per entry the sampled minimum and the number of violating segments.
// The per-segment arithmetic is the check's, on the same operand bits, and so are the tile scaffold and the host path around the
// kernels (scp_separation_device.h).
//
// What differs is the exclusion test.  The check drops a segment whose distance provably exceeds ONE bound T = max(R - 0.01,
// an upper bound of the call's minimum); a segment far above the global minimum can still be vehicle i's closest approach, so
// here a segment (i, j, k) is dropped only if it exceeds  T = max(R - 0.01, U_i, U_j, U_k),  each U an upper bound of the FINAL
// minimum of that entry: the smallest sampled distance of the entry's rows.  With that T the check's margin derivation
// carries over unchanged (d.d > (T + rho_i + rho_j)^2 SEP_SKIP_FACTOR: the computed minimum of f stays above T^2), and the row
// that attains an entry's smallest sampled distance is itself never dropped (its d.d <= U^2 <= T^2), so the entry's computed
// minimum is <= U^2 < every dropped segment: a dropped segment is neither a violation nor any entry's argmin, not even tied.
//
// Kernels, all on the ctx stream (launches are the only synchronisation):
//   clr_init_kernel      the bound arrays to +inf, the solved count to 0;
//   sep_prep_kernel      the check's staging records;
//   clr_seed_kernel      pass 1: the tile loop with the sampled distance only; integer atomicMin on the bit pattern of the
//                        non-negative d.d into U2_vehicle[N] and U2_step[K] -- exact and order independent;
//   clr_pass_kernel      pass 2: the check's phases A and B with the per-entry T.  Phase B stays dense over the LDS queue; its
//                        results (f's minimum, t, the pair) go through LDS in rounds of 256 to OWNER threads: lane x of wave 0
//                        owns the tile's i-side vehicle x, lane x of wave 1 its j-side vehicle x, wave 2 the time step.
//                        An owner folds the results that concern its entry into registers -- (f, row) lexicographically,
//                        an integer count -- so no reduction depends on an order.  One partial per (tile, step) and
//                        128 per (tile, chunk of steps) go to global memory.  The sampled minimum, as pair_geom computes
//                        it, is taken only for pairs whose d.d is within 1 + 1e-12 of the largest of their entries' bounds (a
//                        superset of the pairs within 1 + 1e-12 of an entry's smallest d.d): integer atomicMin on the bits
//                        of that non-negative distance;
//   clr_finish_vehicle_kernel / clr_finish_step_kernel   one fold per vehicle over the tiles of its row and column, one per
//                        step over all tiles -> scp_clearance.
#include "scp_separation_device.h"

namespace {

constexpr unsigned long long CLR_INF_BITS = 0x7FF0000000000000ULL;  // +inf: above every bit pattern of a finite d.d >= 0
constexpr int CLR_FINISH_SLICES = 16;                                // waves of the vehicle fold's workgroup

// A partial result of one entry; the finishing kernels fold them in any order
struct ClrEntry {
  double m;                      // smallest segment minimum of f, +inf: none
  unsigned long long row;        // its row id; ties: the smallest
  double t;                      // where in the segment
  unsigned long long n_viol;     // violating segments
};

struct ClrArgs {
  int N, K, D, kc;               // kc: time steps per workgroup
  double h, thr;                 // thr = R - 0.01
  int64_t q_begin, q_end, pairs;
  const double* rec;             // [K][N][3 D + 1]
  int64_t tile0, n_tiles;        // the launch's tiles in the upper triangle of tiles: [tile0, tile0 + n_tiles)
  int nt;                        // tiles per side
  unsigned long long* u2_veh;    // [N] bits of the smallest sampled d.d of the vehicle's rows (pass 1)
  unsigned long long* u2_step;   // [K] the same per step
  unsigned long long* s_veh;     // [N] bits of the smallest sampled distance as pair_geom computes it (pass 2)
  unsigned long long* s_step;    // [K]
  ClrEntry* part_veh;            // [n_chunks][n_tiles][2 * SEP_TILE]: i side, j side
  ClrEntry* part_step;           // [K][n_tiles]
  unsigned long long* n_solved;  // segments that reached the quartic
};

__device__ inline ClrEntry clr_empty() { return ClrEntry{SEP_INF, SEP_NO_ROW, 0.0, 0ULL}; }

__device__ inline void clr_fold(ClrEntry& x, const ClrEntry& o) {
  fold_min(x.m, x.row, x.t, o.m, o.row, o.t);
  x.n_viol += o.n_viol;
}

// one segment's result (f's minimum m at t, its row) into an entry
__device__ inline void clr_offer(ClrEntry& x, double m, unsigned long long row, double t, double thr) {
  fold_min(x.m, x.row, x.t, m, row, t);
  x.n_viol += sep_violates(m, thr) ? 1ULL : 0ULL;  // the test n_violating of the check counts, on the same bits
}

// an upper bound of the distance whose square has these bits (the rounding of the root stays below the 1e-15)
__device__ inline double clr_bound(unsigned long long bits) { return sqrt(__longlong_as_double((long long)bits)) * (1.0 + 1e-15); }

__global__ __launch_bounds__(256) void clr_init_kernel(unsigned long long* __restrict__ bounds, int64_t n,
                                                        unsigned long long* __restrict__ n_solved) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) bounds[e] = CLR_INF_BITS;
  if (e == 0) *n_solved = 0ULL;
}

// ---- pass 1: the smallest sampled d.d per vehicle and per step ------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SEP_THREADS) void clr_seed_kernel(ClrArgs a) {
  constexpr int NC = 3 * D + 1;
  __shared__ double sp[D][2 * SEP_TILE];  // positions only; [0, 64): the i side, [64, 128): the j side

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  int ti, tj;
  decode_tile(a.tile0 + blockIdx.x, a.nt, ti, tj);
  const int i0 = ti * SEP_TILE, j0 = tj * SEP_TILE;
  const int k_begin = blockIdx.y * a.kc, k_end = min(a.K, k_begin + a.kc);
  if (!tile_live(i0, j0, N, a.q_begin, a.q_end)) return;  // uniform over the workgroup
  const unsigned int valid = tile_valid_mask(i0, j0, wave, lane, N, a.q_begin, a.q_end);

  TileStage<NC, D> stage;  // positions only
  double run_i[SEP_STEPS];  // per i of this thread: the smallest d.d over the steps (folded over the lanes at the end)
#pragma unroll
  for (int s = 0; s < SEP_STEPS; ++s) run_i[s] = SEP_INF;
  double run_j = SEP_INF;
  stage.fetch(a.rec, k_begin, N, i0, j0, tid);
  for (int k = k_begin; k < k_end; ++k) {
    __syncthreads();  // (the previous step has read sp)
    stage.stash(sp, tid);
    __syncthreads();
    if (k + 1 < k_end) stage.fetch(a.rec, k + 1, N, i0, j0, tid);
    double pj[D];
#pragma unroll
    for (int d = 0; d < D; ++d) pj[d] = sp[d][SEP_TILE + lane];
    double ss_min = SEP_INF;
#pragma unroll
    for (int s = 0; s < SEP_STEPS; ++s) {
      const double acc_ss = tile_dd<D>(sp, wave + 4 * s, pj);
      const double ss = (valid >> s) & 1u ? acc_ss : SEP_INF;
      run_i[s] = fmin(run_i[s], ss);
      ss_min = fmin(ss_min, ss);
    }
    run_j = fmin(run_j, ss_min);
    const double step_min = wave_min_f64(ss_min);
    if (lane == 0 && step_min < SEP_INF) atomicMin(&a.u2_step[k], (unsigned long long)__double_as_longlong(step_min));
  }
  if (run_j < SEP_INF) atomicMin(&a.u2_veh[j0 + lane], (unsigned long long)__double_as_longlong(run_j));
#pragma unroll
  for (int s = 0; s < SEP_STEPS; ++s) {
    const double v = wave_min_f64(run_i[s]);
    if (lane == s && v < SEP_INF) atomicMin(&a.u2_veh[i0 + wave + 4 * s], (unsigned long long)__double_as_longlong(v));
  }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SEP_THREADS) void clr_pass_kernel(ClrArgs a) {
  constexpr int NC = 3 * D + 1;
  __shared__ double sm[NC][2 * SEP_TILE];            // component planes; [0, 64): the i side, [64, 128): the j side
  __shared__ unsigned short queue[SEP_TILE * SEP_TILE];
  __shared__ unsigned int q_count;
  __shared__ double ub[2 * SEP_TILE];                // per vehicle of the tile: an upper bound of its final minimum distance
  __shared__ double res_m[SEP_THREADS], res_t[SEP_THREADS];  // one round of phase B results ...
  __shared__ unsigned short res_id[SEP_THREADS];             // ... and their pairs (il << 6 | jl)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  int ti, tj;
  decode_tile(a.tile0 + blockIdx.x, a.nt, ti, tj);
  const int i0 = ti * SEP_TILE, j0 = tj * SEP_TILE;
  const int k_begin = blockIdx.y * a.kc, k_end = min(a.K, k_begin + a.kc);

  // waves 0 and 1: this lane's vehicle over the whole chunk; wave 2: the current step (every lane holds it after the shuffles)
  ClrEntry own = clr_empty();
  unsigned long long n_solved = 0;  // thread 0 only

  auto row_of = [&](int k, unsigned int id) { return tile_row(k, a.pairs, N, i0, j0, (int)(id >> 6), (int)(id & 63)); };

  if (tile_live(i0, j0, N, a.q_begin, a.q_end)) {
    const unsigned int valid = tile_valid_mask(i0, j0, wave, lane, N, a.q_begin, a.q_end);
    if (tid < 2 * SEP_TILE) {  // (read after the first barriers of the loop)
      const int v = (tid < SEP_TILE ? i0 : j0) + (tid & 63);
      ub[tid] = v < N ? clr_bound(a.u2_veh[v]) : SEP_INF;  // a vehicle without a row here: +inf, and no valid pair uses it
    }
    TileStage<NC, NC> stage;
    stage.fetch(a.rec, k_begin, N, i0, j0, tid);
    for (int k = k_begin; k < k_end; ++k) {
      __syncthreads();  // (the previous step's phase B has read sm, the queue and the results)
      stage.stash(sm, tid);
      if (tid == 0) q_count = 0;
      __syncthreads();
      if (k + 1 < k_end) stage.fetch(a.rec, k + 1, N, i0, j0, tid);  // in flight during this step's arithmetic

      // ---- phase A ------------------------------------------------------------------------------------------------
      double pj[D];
#pragma unroll
      for (int d = 0; d < D; ++d) pj[d] = sm[d][SEP_TILE + lane];
      const double rho_j = sm[3 * D][SEP_TILE + lane];
      const double u_jk = fmax(ub[SEP_TILE + lane], clr_bound(a.u2_step[k]));
#pragma unroll
      for (int s = 0; s < SEP_STEPS; ++s) {
        const int il = wave + 4 * s;
        const double ss = tile_dd<D>(sm, il, pj);
        if (!((valid >> s) & 1u)) continue;
        const double u = fmax(ub[il], u_jk);  // the largest of the three entries' bounds
        // sampled minimum per entry, as pair_geom computes it (within an ulp of sqrt(ss)): only a pair within 1e-12 of an
        // entry's smallest d.d can carry that entry's smallest distance; u * u >= the largest of the three smallest d.d
        if (ss <= u * u * (1.0 + 1e-12)) {
          Pt<D> Pi, Pj;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            Pi.v[d] = sm[d][il];
            Pj.v[d] = pj[d];
          }
          const unsigned long long raw = (unsigned long long)__double_as_longlong(pair_geom<D>(Pi, Pj).raw);
          atomicMin(&a.s_veh[i0 + il], raw);
          atomicMin(&a.s_veh[j0 + lane], raw);
          atomicMin(&a.s_step[k], raw);
        }
        // The skip test of the check (its derivation: scp_separation.hip) with T = max(thr, U_i, U_j, U_k)
        const double reach = fmax(a.thr, u) + (sm[3 * D][il] + rho_j);
        if (!(ss > reach * reach * SEP_SKIP_FACTOR)) {
          const unsigned int slot = atomicAdd(&q_count, 1u);
          queue[slot] = (unsigned short)((il << 6) | lane);
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
          const int il = id >> 6, jl = id & 63;
          double m, t;
          quartic_min(tile_quartic<D>(sm, il, jl), a.h, m, t);
          res_m[tid] = m;
          res_t[tid] = t;
          res_id[tid] = (unsigned short)id;
        }
        __syncthreads();
        const unsigned int n_r = min((unsigned int)SEP_THREADS, n_q - base);
        if (wave < 2) {  // the owners of the vehicles: every result of the round that names mine
          for (unsigned int r = 0; r < n_r; ++r) {
            const unsigned int id = res_id[r];
            if ((int)(wave == 0 ? id >> 6 : id & 63) == lane) clr_offer(own, res_m[r], row_of(k, id), res_t[r], a.thr);
          }
        } else if (wave == 2) {  // the owner of the step: all results, strided over the lanes, then folded over the wave
          ClrEntry p = clr_empty();
          for (unsigned int r = lane; r < n_r; r += 64) clr_offer(p, res_m[r], row_of(k, res_id[r]), res_t[r], a.thr);
          wave_fold_min(p.m, p.row, p.t);
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) p.n_viol += __shfl_xor(p.n_viol, s, 64);
          clr_fold(own, p);
        }
        if (base + SEP_THREADS < n_q) __syncthreads();  // (the next round overwrites the results)
      }
      if (wave == 2) {
        if (lane == 0) a.part_step[(int64_t)k * a.n_tiles + blockIdx.x] = own;
        own = clr_empty();
      }
    }
  } else {
    for (int k = k_begin + tid; k < k_end; k += SEP_THREADS) a.part_step[(int64_t)k * a.n_tiles + blockIdx.x] = clr_empty();
  }
  if (tid < 2 * SEP_TILE) a.part_veh[((int64_t)blockIdx.y * a.n_tiles + blockIdx.x) * (2 * SEP_TILE) + tid] = own;
  if (tid == 0 && n_solved) atomicAdd(a.n_solved, n_solved);
}

__device__ inline scp_clearance clr_result(const ClrEntry& r, unsigned long long sample_bits) {
  scp_clearance c;
  c.min_dist = r.row == SEP_NO_ROW ? SEP_INF : sqrt(fmax(r.m, 0.0));  // crossing vehicles: f a few ulps below 0
  c.t_min = r.t;
  c.row = r.row;
  c.sample_min_dist = __longlong_as_double((long long)sample_bits);
  c.n_violating = r.n_viol;
  c.reserved = 0;
  return c;
}

// One workgroup per tile index tv (vehicles 64 tv .. 64 tv + 63): lane = vehicle, 16 waves share the partials of the tiles of
// its row (tv, tj >= tv: the i side) and of its column (ti <= tv, tv: the j side) that the launch covered (tile rows t_lo ..
// t_hi), over all chunks; then the waves' results through LDS.  Any order gives the same result.
__global__ __launch_bounds__(CLR_FINISH_SLICES * 64) void clr_finish_vehicle_kernel(ClrArgs a, int n_chunks, int t_lo, int t_hi,
                                                                                     scp_clearance* __restrict__ out) {
  __shared__ ClrEntry red[CLR_FINISH_SLICES][64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int tv = blockIdx.x;
  const int cnt_i = tv >= t_lo && tv <= t_hi ? a.nt - tv : 0;
  const int j_last = min(tv, t_hi);
  const int cnt_j = j_last >= t_lo ? j_last - t_lo + 1 : 0;
  const int cnt = cnt_i + cnt_j;
  ClrEntry p = clr_empty();
  for (int64_t idx = slice; idx < (int64_t)cnt * n_chunks; idx += CLR_FINISH_SLICES) {
    const int c = (int)(idx / cnt), x = (int)(idx % cnt);
    int64_t u;
    int side;
    if (x < cnt_i) {
      u = tile_start(tv, a.nt) + x;
      side = 0;
    } else {
      const int ti = t_lo + (x - cnt_i);
      u = tile_start(ti, a.nt) + (tv - ti);
      side = 1;
    }
    clr_fold(p, a.part_veh[((int64_t)c * a.n_tiles + (u - a.tile0)) * (2 * SEP_TILE) + side * SEP_TILE + lane]);
  }
  red[slice][lane] = p;
  __syncthreads();
  if (slice == 0) {
    for (int s = 1; s < CLR_FINISH_SLICES; ++s) clr_fold(p, red[s][lane]);
    const int v = tv * SEP_TILE + lane;
    if (v < a.N) out[v] = clr_result(p, a.s_veh[v]);
  }
}

// one workgroup per step: fold the partials of all tiles
__global__ __launch_bounds__(SEP_THREADS) void clr_finish_step_kernel(ClrArgs a, scp_clearance* __restrict__ out) {
  __shared__ ClrEntry red[SEP_THREADS];
  const int k = blockIdx.x;
  ClrEntry p = clr_empty();
  for (int64_t e = threadIdx.x; e < a.n_tiles; e += SEP_THREADS) clr_fold(p, a.part_step[(int64_t)k * a.n_tiles + e]);
  red[threadIdx.x] = p;
  __syncthreads();
  for (int s = SEP_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) clr_fold(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[k] = clr_result(red[0], a.s_step[k]);
}

}  // namespace

extern "C" int scp_clearance_profile(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                                     const double* pos, const double* vel, const double* acc, scp_clearance* per_vehicle,
                                     scp_clearance* per_step) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, per_vehicle || per_step, "clearance_profile: both outputs are null");
  const int64_t n_bounds = 2 * ((int64_t)N + K);  // U2_vehicle, U2_step, sample_vehicle, sample_step
  const size_t bound_bytes = ((size_t)n_bounds * sizeof(unsigned long long) + 63) & ~(size_t)63;
  auto veh_bytes = [](const SepPlan& p) { return (size_t)p.n_chunks * (size_t)p.n_tiles * 2 * SEP_TILE * sizeof(ClrEntry); };
  SepCall c;
  int rc = sep_begin(ctx, "clearance_profile", N, K, D, h, q_begin, q_end, pos, vel, acc, [&](const SepPlan& p) {
    return bound_bytes + veh_bytes(p) + (size_t)K * (size_t)p.n_tiles * sizeof(ClrEntry);
  }, &c);
  if (rc) return rc;
  const SepPlan& plan = c.plan;

  ClrArgs a{};
  a.N = N; a.K = K; a.D = D; a.kc = plan.kc;
  a.h = h; a.thr = R - 0.01;
  a.q_begin = q_begin; a.q_end = q_end; a.pairs = scp_pairs(N);
  a.rec = c.rec;
  a.tile0 = plan.tile0; a.n_tiles = plan.n_tiles; a.nt = plan.nt;
  unsigned long long* bounds = (unsigned long long*)c.extra;
  a.u2_veh = bounds;
  a.u2_step = bounds + N;
  a.s_veh = bounds + N + K;
  a.s_step = bounds + 2 * (int64_t)N + K;
  a.n_solved = ctx->solved + SEP_SOLVED_PROFILE;
  a.part_veh = (ClrEntry*)(c.extra + bound_bytes);
  a.part_step = (ClrEntry*)((char*)a.part_veh + veh_bytes(plan));

  hipLaunchKernelGGL(clr_init_kernel, dim3(scp_cdiv(n_bounds, 256)), dim3(256), 0, ctx->stream, bounds, n_bounds, a.n_solved);
  if (plan.n_tiles > 0) {
    sep_launch_tiles(ctx, plan, D, clr_seed_kernel<2>, clr_seed_kernel<3>, a);
    sep_launch_tiles(ctx, plan, D, clr_pass_kernel<2>, clr_pass_kernel<3>, a);
  }
  if (per_vehicle)
    hipLaunchKernelGGL(clr_finish_vehicle_kernel, dim3(plan.nt), dim3(CLR_FINISH_SLICES * 64), 0, ctx->stream, a, plan.n_chunks,
                       plan.t_lo, plan.t_hi, per_vehicle);
  if (per_step) hipLaunchKernelGGL(clr_finish_step_kernel, dim3(K), dim3(SEP_THREADS), 0, ctx->stream, a, per_step);
  rc = sep_end(ctx);
  if (rc) return rc;
  ctx->solved_ran[SEP_SOLVED_PROFILE] = true;
  return SCP_OK;
}

// segments of the latest scp_clearance_profile of this ctx that reached the quartic (developer figure; synchronises)
extern "C" int scp_ctx_last_clearance_solved(scp_ctx* ctx, uint64_t* n) {
  return sep_read_solved(ctx, SEP_SOLVED_PROFILE, "clearance_profile", n);
}
