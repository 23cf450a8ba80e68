// Goal assignment for interchangeable vehicles and the straight-line check (include/scp_hip.h states both rules; the numpy
// restatement the tests compare against bit for bit is tests/assignment_ref.py).
//
//   asg_auction_kernel  (a template on where c_ij comes from: the coordinates -- scp_assign_goals -- or a matrix in global
//                       memory -- scp_assign_costs; everything below is the one copy both run)
//                       ONE workgroup per scenario, the whole epsilon-scaled Jacobi auction in one launch.  In LDS: the prices,
//                       every person's pending bid, per goal its owner and the lowest-index bidder of the round's highest bid,
//                       per person its goal (>= 0), -1 (unassigned) or -2 - j1 (a bid for j1 is pending).  A round is
//                         A  one wave per unassigned person (persons dealt round-robin to the waves), lanes striding over the
//                            goals: costs recomputed from the points (read through the caches) or read from the person's
//                            row of the matrix (consecutive words), best / second best by shuffles
//                         B  the goal's price := max(price, bids) by 64-bit LDS atomicMax -- every bid exceeds the old price
//                         C  among the bidders whose bid IS the new price the lowest index, by LDS atomicMin
//                         D  that bidder takes the goal, its previous owner and the losers are unassigned again
//                       with a workgroup barrier between the steps: which thread gets where first never shows in the result.
//   line_pair_kernel    tiled pair pass (one workgroup per scenario and tile pair, the generator's tiling): per workgroup the
//                       smallest (d^2, i, j) and the two counts, written as one partial
//   line_finish_kernel  one wave per scenario folds its partials in the same order relation
// No workgroup waits for another one; every loop is bounded by a count (rounds by the guard, phases by the halving of eps).
#include "scp_common.h"
#include "scp_assign_device.h"
#include "scp_line_device.h"

#include <climits>
#include <cmath>

namespace {

constexpr int ASG_MAXN = 4096;
constexpr int LINE_TILE = 256;

// Where c_ij comes from.  A source is made from the kernel's arguments for scenario b (the pointers themselves stay
// __restrict__ parameters of the kernel), hands a bidding wave what it needs of person i (row) and states c_ij from that (at)
// or from the indices alone (pair).
struct AsgFromPoints {  // scp_assign_goals: asg_cost of the coordinates, recomputed wherever it is needed
  static constexpr bool kMatrix = false;
  const double* start;
  const double* goal;
  int D, sh;
  struct Row {
    double a[3];
  };
  __device__ AsgFromPoints(int b, int N, int D_, const double* s, const double* g, const int32_t*)
      : start(s + (int64_t)b * N * D_), goal(g + (int64_t)b * N * D_), D(D_), sh(0) {}
  __device__ Row row(int i, int) const {
    const double* p = start + (int64_t)i * D;  // (constant indices: the row stays in registers)
    return Row{{p[0], p[1], D == 3 ? p[2] : 0.0}};
  }
  __device__ long long at(const Row& r, int j) const { return asg_cost(r.a, goal + (int64_t)j * D, D, sh); }
  __device__ long long pair(int i, int j, int) const { return asg_cost(start + (int64_t)i * D, goal + (int64_t)j * D, D, sh); }
};

struct AsgFromMatrix {  // scp_assign_costs: row i of the scenario's matrix, the lanes of a wave on consecutive words
  static constexpr bool kMatrix = true;
  const int32_t* cost;
  struct Row {
    const int32_t* c;
  };
  __device__ AsgFromMatrix(int b, int N, int, const double*, const double*, const int32_t* c) : cost(c + (int64_t)b * N * N) {}
  __device__ Row row(int i, int N) const { return Row{cost + (int64_t)i * N}; }
  __device__ long long at(const Row& r, int j) const { return r.c[j]; }
  __device__ long long pair(int i, int j, int N) const { return cost[(int64_t)i * N + j]; }
};

template <class Src>
__global__ __launch_bounds__(1024) void asg_auction_kernel(int N, int D, const double* __restrict__ start,
                                                           const double* __restrict__ goal, const int32_t* __restrict__ cost,
                                                           int32_t* __restrict__ goal_of,
                                                           long long* __restrict__ prices, long long max_rounds,
                                                           scp_assign_stats* __restrict__ stats, int* bad_flag) {
#pragma clang fp contract(off)
  extern __shared__ long long s_dyn[];
  long long* s_price = s_dyn;            // [N]
  long long* s_mybid = s_dyn + N;        // [N] the pending bid of person i
  int* s_bidder = (int*)(s_dyn + 2 * N); // [N] per goal: lowest person whose bid is the round's highest
  int* s_owner = s_bidder + N;           // [N] per goal: its person or -1
  int* s_gof = s_owner + N;              // [N] per person: goal, -1 unassigned, -2 - j1 bid pending
  __shared__ double s_lo[3][16], s_hi[3][16];
  __shared__ long long s_red[2][16];
  __shared__ int s_bad[16];
  __shared__ int s_unassigned, s_shift, s_isbad;
  __shared__ long long s_eps0;

  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  const int b = blockIdx.x;
  Src src(b, N, D, start, goal, cost);

  if constexpr (Src::kMatrix) {
    // ---- the largest entry of the scenario's matrix; a negative one is unusable ----
    long long top = 0;
    int bad = 0;
    for (int64_t k = tid; k < (int64_t)N * N; k += nthr) {
      const long long c = src.cost[k];
      bad |= c < 0;
      top = c > top ? c : top;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const long long o = __shfl_xor(top, off, 64);
      top = o > top ? o : top;
      bad |= __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
      s_red[0][wave] = top;
      s_bad[wave] = bad;
    }
    __syncthreads();
    if (tid == 0) {
      int anybad = 0;
      for (int w = 0; w < nwave; ++w) {
        anybad |= s_bad[w];
        top = s_red[0][w] > top ? s_red[0][w] : top;
      }
      const long long e0 = ((long long)(N + 1) * top) / 2;
      s_shift = 0;
      s_eps0 = e0 > 1 ? e0 : 1;
      s_isbad = anybad;
    }
    __syncthreads();  // (s_red is next written after the auction's barriers)
  } else {
    // ---- quantisation: the box of all 2N points ----
    const double* sb = src.start;
    const double* gb = src.goal;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int k = tid; k < 2 * N; k += nthr) {
      const double* p = k < N ? sb + (int64_t)k * D : gb + (int64_t)(k - N) * D;
      for (int d = 0; d < D; ++d) {
        const double v = p[d];
        if (!(fabs(v) <= 1.7976931348623157e308)) bad = 1;  // NaN or infinite
        lo[d] = fmin(lo[d], v);
        hi[d] = fmax(hi[d], v);
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      for (int d = 0; d < 3; ++d) {
        lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, 64));
        hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, 64));
      }
      bad |= __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
      for (int d = 0; d < 3; ++d) {
        s_lo[d][wave] = lo[d];
        s_hi[d][wave] = hi[d];
      }
      s_bad[wave] = bad;
    }
    __syncthreads();
    if (tid == 0) {
      double Bd = 0.0;
      int anybad = 0;
      for (int w = 0; w < nwave; ++w) anybad |= s_bad[w];
      for (int d = 0; d < D; ++d) {
        double l = s_lo[d][0], h = s_hi[d][0];
        for (int w = 1; w < nwave; ++w) {
          l = fmin(l, s_lo[d][w]);
          h = fmax(h, s_hi[d][w]);
        }
        const double span = h - l;
        Bd = d == 0 ? span * span : Bd + span * span;
      }
      if (!(Bd <= 1.7976931348623157e308)) anybad = 1;  // the range overflows
      int sh = 0;
      long long top = 0;
      if (!anybad && Bd > 0.0) {
        int e;
        (void)frexp(Bd, &e);
        sh = 31 - e;
        top = (long long)ldexp(Bd, sh);
      }
      const long long e0 = ((long long)(N + 1) * top) / 2;
      s_shift = sh;
      s_eps0 = e0 > 1 ? e0 : 1;
      s_isbad = anybad;
    }
    __syncthreads();
  }
  const int sh = s_shift;
  if constexpr (!Src::kMatrix) src.sh = sh;
  if (s_isbad) {  // (workgroup-uniform) the host turns the flag into SCP_ERR_INVALID
    for (int i = tid; i < N; i += nthr) {
      goal_of[(int64_t)b * N + i] = i;
      if (prices) prices[(int64_t)b * N + i] = 0;
    }
    if (tid == 0) {
      scp_assign_stats st;
      st.cost_q = st.cost_q_identity = 0;
      st.quantum = 0.0;
      st.rounds = st.bids = 0;
      st.phases = 0;
      st.status = 2;
      stats[b] = st;
      *bad_flag = 1;
    }
    return;
  }

  for (int i = tid; i < N; i += nthr) {
    s_price[i] = 0;
    s_gof[i] = i;  // (N = 1: the identity; every phase starts from -1)
  }
  const long long np1 = (long long)N + 1;
  long long eps = s_eps0, rounds = 0, bids = 0;
  int phases = 0, status = 0;
  if (N >= 2) {
    for (;;) {  // phases: eps falls by 4 until it is 1
      for (int i = tid; i < N; i += nthr) {
        s_owner[i] = -1;
        s_gof[i] = -1;
      }
      if (tid == 0) s_unassigned = N;
      __syncthreads();
      ++phases;
      long long r = 0;
      for (;;) {  // rounds (everything tested here is workgroup-uniform)
        const int un = s_unassigned;
        if (un == 0) break;
        if (r == max_rounds) {
          status = 1;
          break;
        }
        ++r;
        bids += un;
        // A: the bids.  Person base + l * nwave + wave belongs to this wave (a partition of the persons).
        for (int base = 0; base < N; base += 64 * nwave) {
          const int mine = base + lane * nwave + wave;
          unsigned long long m = __ballot(mine < N && s_gof[mine] == -1);
          while (m) {
            const int pi = base + (__ffsll((long long)m) - 1) * nwave + wave;
            m &= m - 1;
            const typename Src::Row mine_row = src.row(pi, N);
            long long v1 = LLONG_MIN, v2 = LLONG_MIN;
            int j1 = INT_MAX;
            for (int j = lane; j < N; j += 64) {
              const long long v = -np1 * src.at(mine_row, j) - s_price[j];
              if (v > v1) {
                v2 = v1;
                v1 = v;
                j1 = j;
              } else if (v > v2) {
                v2 = v;
              }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
              const long long ov1 = __shfl_xor(v1, off, 64), ov2 = __shfl_xor(v2, off, 64);
              const int oj1 = __shfl_xor(j1, off, 64);
              if (ov1 > v1 || (ov1 == v1 && oj1 < j1)) {
                v2 = v1 > ov2 ? v1 : ov2;
                v1 = ov1;
                j1 = oj1;
              } else {
                v2 = v2 > ov1 ? v2 : ov1;
              }
            }
            if (lane == 0) {  // (N >= 2: j1 < N and v2 is a value)
              s_mybid[pi] = s_price[j1] + (v1 - v2) + eps;
              s_gof[pi] = -2 - j1;
            }
          }
        }
        __syncthreads();
        // B: highest bid per goal (a bid exceeds the price it was computed from by at least eps)
        for (int i = tid; i < N; i += nthr) {
          const int g = s_gof[i];
          if (g <= -2) {
            s_bidder[-2 - g] = INT_MAX;  // (every writer stores the same value)
            atomicMax((unsigned long long*)&s_price[-2 - g], (unsigned long long)s_mybid[i]);  // (prices and bids are positive)
          }
        }
        __syncthreads();
        // C: lowest person among those who bid it
        for (int i = tid; i < N; i += nthr) {
          const int g = s_gof[i];
          if (g <= -2 && s_price[-2 - g] == s_mybid[i]) atomicMin(&s_bidder[-2 - g], i);
        }
        __syncthreads();
        // D: hand over.  One winner per goal; only it touches the goal's owner and the previous owner's entry.
        for (int i = tid; i < N; i += nthr) {
          const int g = s_gof[i];
          if (g <= -2) {
            const int j = -2 - g;
            if (s_bidder[j] == i) {
              const int prev = s_owner[j];
              if (prev >= 0)
                s_gof[prev] = -1;
              else
                atomicSub(&s_unassigned, 1);
              s_owner[j] = i;
              s_gof[i] = j;
            } else {
              s_gof[i] = -1;
            }
          }
        }
        __syncthreads();
      }
      rounds += r;
      if (status != 0 || eps == 1) break;
      eps = eps / 4 > 1 ? eps / 4 : 1;
      __syncthreads();  // (s_unassigned was read above; the next phase rewrites it)
    }
  }
  __syncthreads();

  // ---- results ----
  long long cq = 0, ci = 0;
  for (int i = tid; i < N; i += nthr) {
    const int g = status == 0 ? s_gof[i] : i;
    goal_of[(int64_t)b * N + i] = g;
    if (prices) prices[(int64_t)b * N + i] = s_price[i];
    const long long cii = src.pair(i, i, N);
    ci += cii;
    cq += g == i ? cii : src.pair(i, g, N);
  }
  cq = asg_wave_sum(cq);
  ci = asg_wave_sum(ci);
  if (lane == 0) {
    s_red[0][wave] = cq;
    s_red[1][wave] = ci;
  }
  __syncthreads();
  if (tid == 0) {
    scp_assign_stats st;
    st.cost_q = st.cost_q_identity = 0;
    for (int w = 0; w < nwave; ++w) {
      st.cost_q += s_red[0][w];
      st.cost_q_identity += s_red[1][w];
    }
    st.quantum = Src::kMatrix ? 1.0 : ldexp(1.0, -sh);
    st.rounds = rounds;
    st.bids = bids;
    st.phases = phases;
    st.status = status;
    stats[b] = st;
  }
}

// ---- straight-line check ----------------------------------------------------------------------------------------------------
struct LinePartial {
  unsigned long long bits;  // min d^2 (non-negative double: the bits order like the values); +inf: no pair
  unsigned long long pair;  // i << 32 | j of the smallest (d^2, i, j)
  unsigned long long close, opposed;
};

__device__ inline bool line_less(unsigned long long ba, unsigned long long pa, unsigned long long bb, unsigned long long pb) {
  return ba < bb || (ba == bb && pa < pb);
}

// One workgroup per (scenario, tile pair ti <= tj): thread i of tile ti against the agents of tile tj staged in LDS.
__global__ __launch_bounds__(LINE_TILE) void line_pair_kernel(int N, int D, int ntiles, int ntri, double thr,
                                                              const double* __restrict__ start, const double* __restrict__ goal,
                                                              const int32_t* __restrict__ goal_of,
                                                              LinePartial* __restrict__ part, int* bad_flag) {
#pragma clang fp contract(off)
  __shared__ double s_a[3][LINE_TILE], s_g[3][LINE_TILE];
  __shared__ LinePartial s_part[LINE_TILE / 64];

  const int b = blockIdx.x / ntri;
  int rem = blockIdx.x - b * ntri, ti = 0;
  while (rem >= ntiles - ti) {  // upper-triangle index -> (ti, tj)
    rem -= ntiles - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const int tid = threadIdx.x;
  const double* ib = start + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  const int32_t* gof = goal_of ? goal_of + (int64_t)b * N : nullptr;
  auto goal_index = [&](int i) {
    int p = gof ? gof[i] : i;
    if ((unsigned)p >= (unsigned)N) {  // not an index: flagged for the host, read nothing out of bounds
      *bad_flag = 1;
      p = i;
    }
    return p;
  };
  {
    const int j = tj * LINE_TILE + tid;
    if (j < N) {
      const int pj = goal_index(j);
      for (int d = 0; d < D; ++d) {
        s_a[d][tid] = ib[(int64_t)j * D + d];
        s_g[d][tid] = gb[(int64_t)pj * D + d];
      }
    }
  }
  __syncthreads();
  const int i = ti * LINE_TILE + tid;
  double dmin = INFINITY;
  int jmin = 0;
  unsigned long long close = 0, opposed = 0;
  if (i < N) {
    const int pi = goal_index(i);
    const double ax = ib[(int64_t)i * D], ay = ib[(int64_t)i * D + 1];
    const double gx = gb[(int64_t)pi * D], gy = gb[(int64_t)pi * D + 1];
    const double az = D == 3 ? ib[(int64_t)i * D + 2] : 0.0, gz = D == 3 ? gb[(int64_t)pi * D + 2] : 0.0;
    const int jend = min(LINE_TILE, N - tj * LINE_TILE);
    for (int jj = (ti == tj ? tid + 1 : 0); jj < jend; ++jj) {
      const double r0x = ax - s_a[0][jj], r0y = ay - s_a[1][jj], dgx = gx - s_g[0][jj], dgy = gy - s_g[1][jj];
      double d2, dot = r0x * dgx + r0y * dgy;
      if (D == 3) {
        const double r0z = az - s_a[2][jj], dgz = gz - s_g[2][jj];
        d2 = gen_d2_3(r0x, r0y, r0z, dgx, dgy, dgz);
        dot = dot + r0z * dgz;
      } else {
        d2 = gen_d2(r0x, r0y, dgx, dgy);
      }
      if (d2 < dmin) {  // (j ascending: the lowest j of equal minima stays)
        dmin = d2;
        jmin = tj * LINE_TILE + jj;
      }
      if (d2 < thr) ++close;
      if (dot < 0.0) ++opposed;
    }
  }
  unsigned long long mb = (unsigned long long)__double_as_longlong(dmin);
  unsigned long long mp = ((unsigned long long)(unsigned)i << 32) | (unsigned)jmin;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long ob = __shfl_xor(mb, off, 64), op = __shfl_xor(mp, off, 64);
    if (line_less(ob, op, mb, mp)) {
      mb = ob;
      mp = op;
    }
    close += __shfl_xor(close, off, 64);
    opposed += __shfl_xor(opposed, off, 64);
  }
  if ((tid & 63) == 0) s_part[tid >> 6] = LinePartial{mb, mp, close, opposed};
  __syncthreads();
  if (tid == 0) {
    LinePartial p = s_part[0];
    for (int w = 1; w < LINE_TILE / 64; ++w) {
      if (line_less(s_part[w].bits, s_part[w].pair, p.bits, p.pair)) {
        p.bits = s_part[w].bits;
        p.pair = s_part[w].pair;
      }
      p.close += s_part[w].close;
      p.opposed += s_part[w].opposed;
    }
    part[blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(64) void line_finish_kernel(int ntri, const LinePartial* __restrict__ part,
                                                         scp_line_stats* __restrict__ stats) {
  const int b = blockIdx.x, lane = threadIdx.x;
  unsigned long long mb = 0x7FF0000000000000ull, mp = ~0ull, close = 0, opposed = 0;
  for (int t = lane; t < ntri; t += 64) {
    const LinePartial p = part[(int64_t)b * ntri + t];
    if (line_less(p.bits, p.pair, mb, mp)) {
      mb = p.bits;
      mp = p.pair;
    }
    close += p.close;
    opposed += p.opposed;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long ob = __shfl_xor(mb, off, 64), op = __shfl_xor(mp, off, 64);
    if (line_less(ob, op, mb, mp)) {
      mb = ob;
      mp = op;
    }
    close += __shfl_xor(close, off, 64);
    opposed += __shfl_xor(opposed, off, 64);
  }
  if (lane == 0) {
    scp_line_stats st;
    const bool none = mb == 0x7FF0000000000000ull;  // N = 1 (a d^2 is never +inf for finite points)
    st.min_approach = sqrt(__longlong_as_double((long long)mb));
    st.arg_i = none ? -1 : (int32_t)(mp >> 32);
    st.arg_j = none ? -1 : (int32_t)(mp & 0xFFFFFFFFull);
    st.n_close = (int64_t)close;
    st.n_opposed = (int64_t)opposed;
    stats[b] = st;
  }
}

}  // namespace

// the launch behind both calls: one workgroup per scenario, the raised word of the mapped host flag -> SCP_ERR_INVALID
template <class Src>
static int asg_run(scp_ctx* ctx, const char* who, const char* unusable, bool timed, int B, int N, int D, const double* start,
                   const double* goal, const int32_t* cost, int32_t* goal_of, int64_t* prices, int64_t max_rounds_per_phase,
                   scp_assign_stats* stats) {
  static_assert(sizeof(scp_assign_stats) == 48, "scp_assign_stats is 48 bytes");
  const long long guard = max_rounds_per_phase > 0 ? (long long)max_rounds_per_phase : 256ll * N + 4096;
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = asg_host_flag(ctx)) return rc;
  const size_t lds = (size_t)N * (2 * sizeof(long long) + 3 * sizeof(int));  // 28 N bytes: 112 KiB at N = 4096
  if (lds > 48 * 1024)
    SCP_HIP_CHECK(ctx, scp_raise_lds_limit(ctx->device, reinterpret_cast<const void*>(asg_auction_kernel<Src>), lds));
  // small scenarios: four waves, so that several workgroups share a compute unit; large ones: sixteen
  const int threads = N <= 512 ? 256 : 1024;
  hipStream_t st = ctx->stream;
  volatile int* hflag = ctx->h_gen_flag;
  *hflag = 0;
  if (timed && ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, st));
  asg_auction_kernel<Src><<<B, threads, lds, st>>>(N, D, start, goal, cost, goal_of, (long long*)prices, guard, stats,
                                                   ctx->d_gen_flag);
  hipError_t e = hipGetLastError();
  if (timed && e == hipSuccess) {
    if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev1, st));
    ctx->pair_timed = ctx->timing != 0;
    ctx->pair_ran = true;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return scp_fail(ctx, SCP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  SCP_REQUIRE(ctx, *hflag == 0, "%s: %s", who, unusable);
  return SCP_OK;
}

extern "C" int scp_assign_goals(scp_ctx* ctx, int B, int N, int D, const double* start, const double* goal, int32_t* goal_of,
                                int64_t* prices, int64_t max_rounds_per_phase, scp_assign_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, start && goal && goal_of && stats, "assign_goals: NULL argument");
  SCP_REQUIRE(ctx, B >= 1, "assign_goals: B = %d (need B >= 1)", B);
  SCP_REQUIRE(ctx, N >= 1 && N <= ASG_MAXN, "assign_goals: N = %d (need 1 <= N <= %d)", N, ASG_MAXN);
  SCP_REQUIRE(ctx, D == 2 || D == 3, "assign_goals: D = %d (need 2 or 3)", D);
  return asg_run<AsgFromPoints>(ctx, "assign_goals", "a coordinate is not finite, or the range of the points overflows", false, B,
                                N, D, start, goal, nullptr, goal_of, prices, max_rounds_per_phase, stats);
}

extern "C" int scp_assign_costs(scp_ctx* ctx, int B, int N, const int32_t* cost, int32_t* goal_of, int64_t* prices,
                                int64_t max_rounds_per_phase, scp_assign_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, cost && goal_of && stats, "assign_costs: NULL argument");
  SCP_REQUIRE(ctx, B >= 1, "assign_costs: B = %d (need B >= 1)", B);
  SCP_REQUIRE(ctx, N >= 1 && N <= ASG_MAXN, "assign_costs: N = %d (need 1 <= N <= %d)", N, ASG_MAXN);
  return asg_run<AsgFromMatrix>(ctx, "assign_costs", "a cost is negative", true, B, N, 0, nullptr, nullptr, cost, goal_of, prices,
                                max_rounds_per_phase, stats);
}

extern "C" int scp_straight_line_check(scp_ctx* ctx, int B, int N, int D, const double* start, const double* goal,
                                       const int32_t* goal_of, double min_sep, scp_line_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, start && goal && stats, "straight_line_check: NULL argument");
  SCP_REQUIRE(ctx, B >= 1, "straight_line_check: B = %d (need B >= 1)", B);
  SCP_REQUIRE(ctx, N >= 1 && N <= 65536, "straight_line_check: N = %d (need 1 <= N <= 65536)", N);
  SCP_REQUIRE(ctx, D == 2 || D == 3, "straight_line_check: D = %d (need 2 or 3)", D);
  SCP_REQUIRE(ctx, std::isfinite(min_sep) && min_sep >= 0.0, "straight_line_check: min_sep must be finite and >= 0");
  static_assert(sizeof(scp_line_stats) == 32 && sizeof(LinePartial) == 32, "32-byte records");
  const int ntiles = (N + LINE_TILE - 1) / LINE_TILE, ntri = ntiles * (ntiles + 1) / 2;
  SCP_REQUIRE(ctx, (int64_t)B * ntri * LINE_TILE < INT32_MAX,
              "straight_line_check: B = %d scenarios of %d agents exceed one call's grid; split the batch", B, N);
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = asg_host_flag(ctx)) return rc;
  if (const int rc = scp_ctx_ensure_bytes(ctx, &ctx->asg_ws, &ctx->asg_ws_bytes, sizeof(LinePartial) * (size_t)B * ntri))
    return rc;
  LinePartial* part = (LinePartial*)ctx->asg_ws;
  hipStream_t st = ctx->stream;
  volatile int* hflag = ctx->h_gen_flag;
  *hflag = 0;
  line_pair_kernel<<<B * ntri, LINE_TILE, 0, st>>>(N, D, ntiles, ntri, min_sep * min_sep, start, goal, goal_of, part,
                                                   ctx->d_gen_flag);
  line_finish_kernel<<<B, 64, 0, st>>>(ntri, part, stats);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return scp_fail(ctx, SCP_ERR_HIP, "straight_line_check: %s", hipGetErrorString(e));
  SCP_REQUIRE(ctx, *hflag == 0, "straight_line_check: goal_of holds an entry outside [0, N)");
  return SCP_OK;
}
