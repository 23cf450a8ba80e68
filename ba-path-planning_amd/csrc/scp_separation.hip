// Continuous-time separation check (scp_check_separation, include/scp_hip.h): the minimum over every SEGMENT of a
// trajectory -- not only over its K samples -- of the distance of every pair of vehicles.  Over segment k vehicle i flies
//   p_i[k] + t v_i[k] + t^2/2 a_i[k],  t in [0, h]   (the kinematics of scp_kinematics, constant acceleration per step),
// so with d = p_i - p_j, w = v_i - v_j, b = a_i - a_j at sample k the squared distance of a pair is the quartic
//   f(t) = |d + t w + t^2/2 b|^2 = c0 + c1 t + c2 t^2 + c3 t^3 + c4 t^4,
//   c0 = d.d, c1 = 2 d.w, c2 = w.w + d.b, c3 = w.b, c4 = b.b / 4.
//
// Three kernels, all on the ctx stream:
//   sep_prep_kernel    [N][K][D] pos / vel / acc -> one time-major record per (k, vehicle): pos, vel, acc and the vehicle's
//                      REACH rho = h |v| + h^2/2 |a| (how far it can be from its sample within the segment);
//   sep_pass_kernel    one workgroup = one 64 x 64 tile of the (i, j) triangle over a chunk of time steps.  Tiles, not the
//                      N-wide k-slices of the sampled passes: the LDS footprint (128 records) does not depend on N.
//                      Phase A (every segment, ~10 fp64 operations): sampled distance, and ONE conservative comparison
//                      |d| > (T + rho_i + rho_j)(1 + 3e-6): such a segment stays above T = max(R - 0.01, an upper bound of the
//                      minimum that is already known), so it is neither a violation nor the argmin and is dropped.  The
//                      others are queued in LDS.  Phase B (the queue, dense over the threads -- no wave runs the solve for
//                      one near lane and 63 idle ones): the quartic's minimum over [0, h];
//   sep_finish_kernel  the per-workgroup partials -> scp_separation_stats.
// Every reduction is a minimum of (value, row id) pairs or an integer sum: exact and commutative, so the result depends
// neither on scheduling nor on how the pair range was cut.
//
// The conflict list (scp_list_conflicts) is the same pass instantiated with LIST = true: phase B keeps, for every violating
// segment, one scp_conflict record (appended through a device counter), and sep_sort_* / sep_gather_kernel put the records
// into ascending row order -- the keys are unique, so the sorted list depends neither on scheduling nor on the cut.
//
// The tile scaffold (staging, range tests, sampled d.d, quartic, violation test, row id, lexicographic fold) and the host path
// around the kernels (SepCall) are scp_separation_device.h's: the clearance profile (scp_clearance.hip) runs the same
// arithmetic on the same bits.
#include "scp_separation_device.h"

namespace {

// Per-workgroup partial result; the finishing kernel folds them in any order.
struct SepPartial {
  double m;                      // smallest segment minimum of f (may be slightly negative where vehicles cross), +inf: none
  unsigned long long row;        // its row id; ties: the smallest
  double t;                      // where in the segment
  unsigned long long first;      // smallest violating row id
  unsigned long long n_viol;     // violating segments
  double sample;                 // smallest sampled distance, as pair_geom computes it (= scp_check_avoidance's)
  unsigned long long n_solved;   // segments that reached the quartic (reported by tools/separation_times.py)
  unsigned long long pad;
};

__device__ inline SepPartial sep_empty() { return SepPartial{SEP_INF, SEP_NO_ROW, 0.0, SEP_NO_ROW, 0, SEP_INF, 0, 0}; }

__device__ inline void sep_fold(SepPartial& x, const SepPartial& o) {
  fold_min(x.m, x.row, x.t, o.m, o.row, o.t);
  x.first = o.first < x.first ? o.first : x.first;
  x.n_viol += o.n_viol;
  x.n_solved += o.n_solved;
  x.sample = fmin(x.sample, o.sample);
}

// Where the LIST instantiation of the pass keeps its records
struct SepList {
  scp_conflict* raw;             // records in the order of arrival, `capacity` of them
  unsigned long long* n_found;   // the caller's counter: counts every violating segment, stored or not
  int64_t capacity;
};

struct SepArgs {
  int N, K, D, kc;               // kc: time steps per workgroup
  double h, thr;                 // thr = R - 0.01 (scp.py:610)
  int64_t q_begin, q_end, pairs;
  const double* rec;             // [K][N][3 D + 1]
  SepPartial* part;              // [gridDim.y][gridDim.x]
  int64_t tile0;                 // index of the first tile of this launch in the upper triangle (diagonal included) of tiles
  int nt;                        // tiles per side
  SepList list;                  // LIST only (last: the offsets of the fields above are those of the check)
};

// Where a violating segment is below the threshold: g = f - thr2 over [0, h].  The scheme of quartic_min, with BOTH sign
// changes of f', yields every stationary point of f in (0, h) (f' is monotone on each of the three pieces, so a piece holds
// at most one).  Between consecutive breakpoints {0, stationary points, h} f is monotone, so g has at most one root there:
// g is evaluated at the five breakpoint slots (a piece without a stationary point repeats the breakpoint before it, which
// changes nothing) and the two outermost sub-intervals over which it changes sign are bisected (48 halvings).
//   t_in   0 if the segment starts below the threshold, else the end of the first bisection that lies below it;
//   t_out  h if it ends below, else the same from the right;
//   pieces maximal runs of breakpoints below the threshold (f has at most one interior maximum: 1 or 2).
// The caller's test is sqrt(max(min f, 0)) < thr, which can differ from min f < thr2 in the last bit, and quartic_min may
// report a split point: if no breakpoint is below thr2 the window is the single point t_min.
__device__ inline void quartic_window(const Quartic& q, double h, double thr2, double t_min, double& t_in, double& t_out,
                                      unsigned int& pieces) {
  double s1 = -1.0, s2 = -1.0;  // the split points, as in quartic_min
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
  const double pa = s1 >= 0.0 ? s1 : 0.0, pb = s2 >= 0.0 ? s2 : pa;
  // breakpoints b0 <= b1 <= b2 <= b3 <= b4 (named, not an array: nothing here is indexed at run time)
  auto stationary = [&](double lo, double hi, double prev) {
    const double gl = q.g(lo), gh = q.g(hi);
    if (!((gl < 0.0 && gh > 0.0) || (gl > 0.0 && gh < 0.0))) return prev;
    const bool rising = gl < 0.0;
    for (int it = 0; it < 48; ++it) {
      const double mid = 0.5 * (lo + hi);
      if ((q.g(mid) < 0.0) == rising) lo = mid;
      else hi = mid;
    }
    return 0.5 * (lo + hi);
  };
  const double b0 = 0.0;
  const double b1 = stationary(0.0, pa, b0);
  const double b2 = stationary(pa, pb, b1);
  const double b3 = stationary(pb, h, b2);
  const double b4 = h;
  const bool u0 = q.f(b0) < thr2, u1 = q.f(b1) < thr2, u2 = q.f(b2) < thr2, u3 = q.f(b3) < thr2, u4 = q.f(b4) < thr2;
  if (!(u0 || u1 || u2 || u3 || u4)) {
    t_in = t_out = t_min;
    pieces = 1;
    return;
  }
  pieces = (unsigned int)u0 + (unsigned int)(u1 && !u0) + (unsigned int)(u2 && !u1) + (unsigned int)(u3 && !u2) +
           (unsigned int)(u4 && !u3);
  // lo: at or above the threshold, hi: below it (either may be the larger time); returns the end that is below
  auto crossing = [&](double above, double below) {
    for (int it = 0; it < 48; ++it) {
      const double mid = 0.5 * (above + below);
      if (q.f(mid) < thr2) below = mid;
      else above = mid;
    }
    return below;
  };
  // the first breakpoint below the threshold and the one before it; the last one and the one after it
  const double in_b = u0 ? b0 : u1 ? b1 : u2 ? b2 : u3 ? b3 : b4, in_a = u1 ? b0 : u2 ? b1 : u3 ? b2 : b3;
  const double out_b = u4 ? b4 : u3 ? b3 : u2 ? b2 : u1 ? b1 : b0, out_a = u3 ? b4 : u2 ? b3 : u1 ? b2 : b1;
  t_in = u0 ? 0.0 : crossing(in_a, in_b);
  t_out = u4 ? h : crossing(out_a, out_b);
}

// The pass.  LIST = false: the reductions of scp_check_separation (a.list unused).  LIST = true: the records of
// scp_list_conflicts and nothing else -- no partials, no sampled minimum, and the skip test with T = thr alone (the known
// upper bound of the minimum only serves the argmin): a skipped segment stays above thr, so it is not a violation.
template <int D, bool LIST = false>
__global__ __launch_bounds__(SEP_THREADS) void sep_pass_kernel(SepArgs a) {
  constexpr int NC = 3 * D + 1;
  __shared__ double sm[NC][2 * SEP_TILE];            // component planes; [0, 64): the i side, [64, 128): the j side
  __shared__ unsigned short queue[SEP_TILE * SEP_TILE];
  __shared__ unsigned int q_count;
  __shared__ SepPartial red[SEP_THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  int ti, tj;
  decode_tile(a.tile0 + blockIdx.x, a.nt, ti, tj);
  const int i0 = ti * SEP_TILE, j0 = tj * SEP_TILE;
  const int k_begin = blockIdx.y * a.kc, k_end = min(a.K, k_begin + a.kc);

  double best_m = SEP_INF, best_t = 0.0, min_ss = SEP_INF, min_raw = SEP_INF;
  unsigned long long best_row = SEP_NO_ROW, first = SEP_NO_ROW, n_viol = 0, n_solved = 0;

  if (tile_live(i0, j0, N, a.q_begin, a.q_end)) {
    const unsigned int valid = tile_valid_mask(i0, j0, wave, lane, N, a.q_begin, a.q_end);
    TileStage<NC, NC> stage;
    double ub = SEP_INF;  // an upper bound of this call's minimum distance: the smallest sampled distance this wave has seen
    stage.fetch(a.rec, k_begin, N, i0, j0, tid);
    for (int k = k_begin; k < k_end; ++k) {
      __syncthreads();  // (the previous step's phase B has read sm and the queue)
      stage.stash(sm, tid);
      if (tid == 0) q_count = 0;
      __syncthreads();
      if (k + 1 < k_end) stage.fetch(a.rec, k + 1, N, i0, j0, tid);  // in flight during this step's arithmetic

      // ---- phase A ------------------------------------------------------------------------------------------------
      double pj[D];
#pragma unroll
      for (int d = 0; d < D; ++d) pj[d] = sm[d][SEP_TILE + lane];
      const double rho_j = sm[3 * D][SEP_TILE + lane];
      double ss[SEP_STEPS];
      double ss_min = SEP_INF;
#pragma unroll
      for (int s = 0; s < SEP_STEPS; ++s) {
        const double acc_ss = tile_dd<D>(sm, wave + 4 * s, pj);
        ss[s] = (valid >> s) & 1u ? acc_ss : SEP_INF;
        ss_min = fmin(ss_min, ss[s]);
      }
      // sampled minimum, bit for bit scp_check_avoidance's: pair_geom's distance is within an ulp of sqrt(ss), so only a
      // pair whose ss is within 1e-12 of the smallest one seen can carry a smaller distance -- it alone pays for pair_geom
      if (!LIST && ss_min <= min_ss * (1.0 + 1e-12)) {
#pragma unroll
        for (int s = 0; s < SEP_STEPS; ++s)
          if (((valid >> s) & 1u) && ss[s] <= min_ss * (1.0 + 1e-12)) {
            Pt<D> Pi, Pj;
#pragma unroll
            for (int d = 0; d < D; ++d) {
              Pi.v[d] = sm[d][wave + 4 * s];
              Pj.v[d] = pj[d];
            }
            min_raw = fmin(min_raw, pair_geom<D>(Pi, Pj).raw);
          }
        min_ss = fmin(min_ss, ss_min);
      }
      // The skip test.  L = |d| - rho_i - rho_j bounds the segment's distance from below, S = |d| + rho_i + rho_j bounds
      // every term of f.  Skipping needs the COMPUTED minimum of f above T^2, and the evaluation of f errs by a few eps S^2:
      // L >= T (1 + 1e-6) + 1e-6 S gives L^2 >= T^2 + 1e-12 S^2, four orders above that error.  Rearranged:
      // |d| >= (T + rho) (1 + 1e-6) / (1 - 1e-6); tested as d.d > (T + rho)^2 (1 + 7e-6).  T >= this wave's smallest sampled
      // distance >= the call's minimum, so a skipped segment is strictly above the minimum: never the argmin, not even tied.
      if constexpr (!LIST) ub = fmin(ub, sqrt(wave_min_f64(ss_min)) * (1.0 + 1e-15));
      const double T = LIST ? a.thr : fmax(a.thr, ub);
#pragma unroll
      for (int s = 0; s < SEP_STEPS; ++s) {
        const double reach = T + (sm[3 * D][wave + 4 * s] + rho_j);
        if (((valid >> s) & 1u) && !(ss[s] > reach * reach * SEP_SKIP_FACTOR)) {
          const unsigned int slot = atomicAdd(&q_count, 1u);
          queue[slot] = (unsigned short)(((wave + 4 * s) << 6) | lane);
        }
      }
      __syncthreads();

      // ---- phase B: the queued segments, dense over the threads (the queue's order does not matter: exact reductions) ----
      const unsigned int n_q = q_count;
      for (unsigned int e = tid; e < n_q; e += SEP_THREADS) {
        const int il = queue[e] >> 6, jl = queue[e] & 63;
        const Quartic q = tile_quartic<D>(sm, il, jl);
        double m, t;
        quartic_min(q, a.h, m, t);
        const unsigned long long row = tile_row(k, a.pairs, N, i0, j0, il, jl);
        if constexpr (LIST) {
          if (sep_violates(m, a.thr)) {  // the test n_violating counts, on the same bits
            double t_in, t_out;
            unsigned int pieces;
            quartic_window(q, a.h, a.thr * a.thr, t, t_in, t_out, pieces);
            const unsigned long long slot = atomicAdd(a.list.n_found, 1ULL);
            if (slot < (unsigned long long)a.list.capacity) a.list.raw[slot] = scp_conflict{row, sqrt(fmax(m, 0.0)), t, t_in, t_out, pieces, 0u};
          }
        } else {
          fold_min(best_m, best_row, best_t, m, row, t);
          if (sep_violates(m, a.thr)) {
            ++n_viol;
            first = row < first ? row : first;
          }
          ++n_solved;
        }
      }
    }
  }

  if constexpr (LIST) return;
  // ---- workgroup reduction: wave shuffles, then the four wave results through LDS ---------------------------------------
  wave_fold_min(best_m, best_row, best_t);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long f2 = __shfl_xor(first, s, 64);
    first = f2 < first ? f2 : first;
    n_viol += __shfl_xor(n_viol, s, 64);
    n_solved += __shfl_xor(n_solved, s, 64);
    min_raw = fmin(min_raw, __shfl_xor(min_raw, s, 64));
  }
  if (lane == 0) red[wave] = SepPartial{best_m, best_row, best_t, first, n_viol, min_raw, n_solved, 0};
  __syncthreads();
  if (tid == 0) {
    SepPartial p = red[0];
    for (int w = 1; w < SEP_THREADS / 64; ++w) sep_fold(p, red[w]);
    a.part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
  }
}

// one workgroup: fold the partials (any order gives the same result) and write the stats
__global__ __launch_bounds__(SEP_THREADS) void sep_finish_kernel(const SepPartial* __restrict__ part, int64_t n,
                                                                 scp_separation_stats* __restrict__ stats,
                                                                 unsigned long long* __restrict__ n_solved_out) {
  __shared__ SepPartial red[SEP_THREADS];
  SepPartial p = sep_empty();
  for (int64_t e = threadIdx.x; e < n; e += SEP_THREADS) {
    const SepPartial o = part[e];
    sep_fold(p, o);
  }
  red[threadIdx.x] = p;
  __syncthreads();
  for (int s = SEP_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sep_fold(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const SepPartial& r = red[0];
    // an empty pair range: the values scp_check_avoidance leaves (min_dist = +inf, no violation)
    stats->min_dist = r.row == SEP_NO_ROW ? SEP_INF : sqrt(fmax(r.m, 0.0));  // crossing vehicles: f a few ulps below 0
    stats->sample_min_dist = r.sample;
    stats->argmin_t = r.t;
    stats->argmin_row = r.row;
    stats->first_violation = r.first;
    stats->n_violating = r.n_viol;
    *n_solved_out = r.n_solved;
  }
}

// ---- the conflict list's order: a bitonic sort of (row, arrival index) pairs, then one gather of the records ---------------
// The length n is known on the device only, so the host sizes every launch for the capacity and each kernel leaves early
// where n (rounded up to a power of two, at least one chunk) does not reach it.  Slots beyond n carry the key SEP_NO_ROW and
// sort to the end.  An overflowed list (n > capacity) counts as empty: nothing in `out` is defined then.
constexpr int SORT_CHUNK = 1024;  // pairs one workgroup sorts in LDS (12 KiB): short lists need this one launch

__device__ inline unsigned long long list_len(const unsigned long long* n_found, int64_t capacity) {
  const unsigned long long n = *n_found;
  return n > (unsigned long long)capacity ? 0ULL : n;
}

__device__ inline unsigned long long sort_span(unsigned long long n) {  // the power of two the network runs over
  unsigned long long p = SORT_CHUNK;
  while (p < n) p <<= 1;
  return p;
}

// comparator c of the step with distance j: elements i < partner = i + j
__device__ inline unsigned long long comparator_low(unsigned long long c, unsigned long long j) {
  return ((c & ~(j - 1)) << 1) | (c & (j - 1));
}

// One chunk per workgroup, in LDS.  init: keys from the records, then every stage k = 2 .. SORT_CHUNK of the network;
// otherwise the steps j = SORT_CHUNK / 2 .. 1 of stage k (the ones that stay inside a chunk).
__global__ __launch_bounds__(SEP_THREADS) void sep_sort_local_kernel(const scp_conflict* __restrict__ raw,
                                                                     const unsigned long long* __restrict__ n_found,
                                                                     int64_t capacity, unsigned long long* __restrict__ keys,
                                                                     unsigned int* __restrict__ idx, unsigned long long k_stage,
                                                                     int init) {
  __shared__ unsigned long long sk[SORT_CHUNK];
  __shared__ unsigned int si[SORT_CHUNK];
  const unsigned long long n = list_len(n_found, capacity), span = sort_span(n);
  const unsigned long long base = (unsigned long long)blockIdx.x * SORT_CHUNK;
  if (base >= span || (!init && k_stage > span)) return;  // uniform over the workgroup
  for (int e = threadIdx.x; e < SORT_CHUNK; e += SEP_THREADS) {
    const unsigned long long g = base + e;
    sk[e] = init ? (g < n ? raw[g].row : SEP_NO_ROW) : keys[g];
    si[e] = init ? (unsigned int)g : idx[g];
  }
  __syncthreads();
  auto steps = [&](unsigned long long k, int j_first) {
    for (int j = j_first; j >= 1; j >>= 1) {
      for (int c = threadIdx.x; c < SORT_CHUNK / 2; c += SEP_THREADS) {
        const int i = (int)comparator_low(c, j), o = i + j;
        const bool up = ((base + i) & k) == 0;
        const unsigned long long a = sk[i], b = sk[o];
        if ((a > b) == up) {
          sk[i] = b;
          sk[o] = a;
          const unsigned int x = si[i];
          si[i] = si[o];
          si[o] = x;
        }
      }
      __syncthreads();
    }
  };
  if (init) {
    for (int k = 2; k <= SORT_CHUNK; k <<= 1) steps(k, k >> 1);
  } else {
    steps(k_stage, SORT_CHUNK / 2);
  }
  for (int e = threadIdx.x; e < SORT_CHUNK; e += SEP_THREADS) {
    keys[base + e] = sk[e];
    idx[base + e] = si[e];
  }
}

// one step (stage k, distance j >= SORT_CHUNK) over global memory
__global__ __launch_bounds__(SEP_THREADS) void sep_sort_global_kernel(const unsigned long long* __restrict__ n_found,
                                                                      int64_t capacity, unsigned long long* __restrict__ keys,
                                                                      unsigned int* __restrict__ idx, unsigned long long k,
                                                                      unsigned long long j) {
  const unsigned long long span = sort_span(list_len(n_found, capacity));
  const unsigned long long c = (unsigned long long)blockIdx.x * SEP_THREADS + threadIdx.x;
  if (k > span || c >= span / 2) return;
  const unsigned long long i = comparator_low(c, j), o = i + j;
  const bool up = (i & k) == 0;
  const unsigned long long a = keys[i], b = keys[o];
  if ((a > b) == up) {
    keys[i] = b;
    keys[o] = a;
    const unsigned int x = idx[i];
    idx[i] = idx[o];
    idx[o] = x;
  }
}

__global__ __launch_bounds__(SEP_THREADS) void sep_gather_kernel(const scp_conflict* __restrict__ raw,
                                                                 const unsigned long long* __restrict__ n_found,
                                                                 int64_t capacity, const unsigned int* __restrict__ idx,
                                                                 scp_conflict* __restrict__ out) {
  const unsigned long long n = list_len(n_found, capacity);
  const unsigned long long e = (unsigned long long)blockIdx.x * SEP_THREADS + threadIdx.x;
  if (e < n) out[e] = raw[idx[e]];
}

SepArgs sep_args(int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end, const SepCall& c, SepPartial* part) {
  SepArgs a{};
  a.N = N; a.K = K; a.D = D; a.kc = c.plan.kc;
  a.h = h; a.thr = R - 0.01;
  a.q_begin = q_begin; a.q_end = q_end; a.pairs = scp_pairs(N);
  a.rec = c.rec; a.part = part; a.tile0 = c.plan.tile0; a.nt = c.plan.nt;
  return a;
}

template <bool LIST>
void sep_launch_pass(scp_ctx* ctx, const SepCall& c, const SepArgs& a) {
  sep_launch_tiles(ctx, c.plan, a.D, sep_pass_kernel<2, LIST>, sep_pass_kernel<3, LIST>, a);
}

}  // namespace

extern "C" int scp_check_separation(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                                    const double* pos, const double* vel, const double* acc, scp_separation_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, stats, "check_separation: null pointer");
  SepCall c;
  auto n_part = [](const SepPlan& p) { return p.n_tiles * p.n_chunks; };
  int rc = sep_begin(ctx, "check_separation", N, K, D, h, q_begin, q_end, pos, vel, acc,
                     [&](const SepPlan& p) { return (size_t)std::max<int64_t>(n_part(p), 1) * sizeof(SepPartial); }, &c);
  if (rc) return rc;
  SepPartial* part = (SepPartial*)c.extra;
  if (c.plan.n_tiles > 0) sep_launch_pass<false>(ctx, c, sep_args(N, K, D, h, R, q_begin, q_end, c, part));
  hipLaunchKernelGGL(sep_finish_kernel, dim3(1), dim3(SEP_THREADS), 0, ctx->stream, part, n_part(c.plan), stats,
                     ctx->solved + SEP_SOLVED_CHECK);
  rc = sep_end(ctx);
  if (rc) return rc;
  ctx->solved_ran[SEP_SOLVED_CHECK] = true;
  return SCP_OK;
}

// segments of the latest scp_check_separation of this ctx that reached the quartic (developer figure; synchronises)
extern "C" int scp_ctx_last_separation_solved(scp_ctx* ctx, uint64_t* n) {
  return sep_read_solved(ctx, SEP_SOLVED_CHECK, "check_separation", n);
}

// The violating segments of the pair range, one record each, in ascending row order (include/scp_hip.h)
extern "C" int scp_list_conflicts(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                                  const double* pos, const double* vel, const double* acc, scp_conflict* out, int64_t capacity,
                                  uint64_t* n_found) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, n_found, "list_conflicts: null pointer");
  SCP_REQUIRE(ctx, capacity >= 0 && capacity <= ((int64_t)1 << 30), "list_conflicts: bad capacity %lld", (long long)capacity);
  SCP_REQUIRE(ctx, out || capacity == 0, "list_conflicts: null list of capacity %lld", (long long)capacity);
  int64_t span = SORT_CHUNK;  // sort_span(capacity)
  while (span < capacity) span <<= 1;
  const size_t raw_bytes = ((size_t)capacity * sizeof(scp_conflict) + 63) & ~(size_t)63;
  SepCall c;
  int rc = sep_begin(ctx, "list_conflicts", N, K, D, h, q_begin, q_end, pos, vel, acc, [&](const SepPlan&) {
    return raw_bytes + (size_t)span * (sizeof(unsigned long long) + sizeof(unsigned int));
  }, &c);
  if (rc) return rc;
  scp_conflict* raw = (scp_conflict*)c.extra;
  unsigned long long* keys = (unsigned long long*)(c.extra + raw_bytes);
  unsigned int* idx = (unsigned int*)(keys + span);
  unsigned long long* count = (unsigned long long*)n_found;

  SCP_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(unsigned long long), ctx->stream));
  if (c.plan.n_tiles > 0) {
    SepArgs a = sep_args(N, K, D, h, R, q_begin, q_end, c, nullptr);
    a.list = SepList{raw, count, capacity};
    sep_launch_pass<true>(ctx, c, a);
    if (capacity > 0) {
      const dim3 chunks((unsigned)(span / SORT_CHUNK)), halves((unsigned)scp_cdiv(span / 2, SEP_THREADS));
      hipLaunchKernelGGL(sep_sort_local_kernel, chunks, dim3(SEP_THREADS), 0, ctx->stream, raw, count, capacity, keys, idx,
                         0ULL, 1);
      for (int64_t k = 2 * SORT_CHUNK; k <= span; k <<= 1) {
        for (int64_t j = k >> 1; j >= SORT_CHUNK; j >>= 1)
          hipLaunchKernelGGL(sep_sort_global_kernel, halves, dim3(SEP_THREADS), 0, ctx->stream, count, capacity, keys, idx,
                             (unsigned long long)k, (unsigned long long)j);
        hipLaunchKernelGGL(sep_sort_local_kernel, chunks, dim3(SEP_THREADS), 0, ctx->stream, raw, count, capacity, keys, idx,
                           (unsigned long long)k, 0);
      }
      hipLaunchKernelGGL(sep_gather_kernel, dim3((unsigned)scp_cdiv(capacity, SEP_THREADS)), dim3(SEP_THREADS), 0, ctx->stream,
                         raw, count, capacity, idx, out);
    }
  }
  return sep_end(ctx);
}
