// Goal assignment of scenarios too large for one workgroup's LDS, and of single scenarios that want the whole chip
// (scp_assign_goals_wide; include/scp_hip.h states the rule, scp_assign.hip is the one-workgroup form, and both agree with
// tests/assignment_ref.py bit for bit).  The auction's state lives in global memory, in a workspace the ctx owns: per
// scenario the prices, per goal the round's highest bid and the key of its lowest bidder, per goal its owner, per person its
// goal (>= 0), -1 (unassigned) or -2 - j1 (a bid for j1 is pending) and its pending bid, two lists of bidders (this round's
// and the next one's), and a control block.
//
//   asgw_init_kernel      resets the arrays and the control blocks
//   asgw_box_kernel       the box of the 2N points: per workgroup min / max, folded by integer atomics on order-preserving keys
//   asgw_control_kernel   ONE workgroup per scenario, the only kernel that advances a scenario's control block.  It derives the
//                         quantisation from the box, starts and ends phases, applies the guard and counts the rounds; a round
//                         with fewer bidders than the threshold it runs itself (a NARROW round: steps A, C, D below over the
//                         bidder list, the goals of a bidder split among the waves that would otherwise idle), round after
//                         round; at a round with more it sets `wide` and returns
//   asgw_bid_kernel       A of a WIDE round: one wave per ASGW_PB bidders, lanes striding over the goals; the bid is folded
//                         into the goal's highest bid by a 64-bit atomicMax (B of scp_assign.hip; the prices are not touched,
//                         every bidder of the round reads the old ones)
//   asgw_claim_kernel     C: a bidder whose bid IS the goal's highest puts its key into the goal by atomicMin
//   asgw_handover_kernel  D: the bidder whose key stands takes the goal and sets its price, the previous owner and the losers
//                         go onto the next round's list
//   asgw_result_kernel, asgw_stats_kernel   goal_of, prices, the two cost sums (integer atomicAdd) and the stats
//
// A bidder's key is (KEY_TOP - round number) << 17 | person: the keys of a later round are smaller than anything an earlier
// one left behind, so the per-goal words are never reset.  Only integer max / min / add fold values that several workgroups
// produce, so the outcome does not depend on which gets where first.  The bidder lists ARE in arrival order -- nothing depends
// on their order: a round's result is a function of the SET of bidders.
//
// The host enqueues init, box, control and then batches of (bid, claim, handover, control); every kernel reads the control
// block first and returns at once where it has nothing to do (scenario done, no wide round pending).  After each batch the
// host waits for the stream and reads one mapped word that the control kernel of the last scenario to finish has set.
// No workgroup waits for another one; every device loop is bounded by a count (rounds by the guard, phases by the halving of
// eps), the host loop by phases x (guard + 1) steps.
#include "scp_common.h"
#include "scp_assign_device.h"

#include <climits>
#include <cmath>

namespace {

constexpr int ASGW_MAXN = 65536;
constexpr int ASGW_PB = 4;              // bidders per wave and sweep of the goals in a wide round (each goal is loaded once for all)
constexpr int ASGW_LDS_MAXN = 16384;    // narrow runs keep the prices in LDS up to here (8 N bytes = 128 KiB of 160)
constexpr int ASGW_TILE = 256;          // threads of every kernel but the control kernel
constexpr unsigned long long ASGW_KEY_TOP = (1ull << 46) - 1;  // (rounds of one call: below 2^46; persons: below 2^17)

struct alignas(64) AsgwCtl {
  unsigned long long lo[3], hi[3];  // the box, as order-preserving keys (asgw_enc)
  long long eps, r, rounds, bids;   // the phase's eps, rounds of the phase so far, totals
  long long round_no;               // rounds of the call so far (the bidders' keys)
  unsigned long long cq, ci;        // the two cost sums
  int shift, phases, status;
  int done, started, bad;
  int wide;                         // the round that was counted last runs as bid / claim / handover launches
  int cur, nbid, next;              // the list the bidders are in, their number; entries of the other list (a wide round's output)
};

struct AsgwView {
  long long* price;            // [N] per goal
  unsigned long long* hb;      // [N] per goal: the highest bid of the round in progress, 0 between rounds
  long long* mybid;            // [N] per person
  unsigned long long* bidder;  // [N] per goal: the smallest key among the bidders of the highest bid
  int* owner;                  // [N] per goal: its person or -1
  int* gof;                    // [N] per person
  int* lists;                  // [2][N]
  int N;
  __device__ int* list(int k) const { return lists + (k ? N : 0); }
};
constexpr size_t ASGW_BYTES_PER_ENTRY = 4 * 8 + 4 * 4;  // 48 N bytes per scenario
constexpr size_t ASGW_HEADER = 64;                      // word 0: scenarios done

__host__ __device__ inline AsgwCtl* asgw_ctl(void* ws) { return (AsgwCtl*)((char*)ws + ASGW_HEADER); }

__device__ inline AsgwView asgw_view(void* ws, int B, int b, int N) {
  char* p = (char*)ws + ASGW_HEADER + sizeof(AsgwCtl) * (size_t)B + ASGW_BYTES_PER_ENTRY * (size_t)N * b;
  AsgwView v;
  v.price = (long long*)p;
  v.hb = (unsigned long long*)(p + 8 * (size_t)N);
  v.mybid = (long long*)(p + 16 * (size_t)N);
  v.bidder = (unsigned long long*)(p + 24 * (size_t)N);
  v.owner = (int*)(p + 32 * (size_t)N);
  v.gof = v.owner + N;
  v.lists = v.gof + N;
  v.N = N;
  return v;
}

// doubles (no NaN) -> unsigned integers in the same order, and back
__device__ inline unsigned long long asgw_enc(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double asgw_dec(unsigned long long e) {
  return __longlong_as_double((long long)((e >> 63) ? (e ^ 0x8000000000000000ull) : ~e));
}

// words that atomics of other threads change are read and reset past the L1
__device__ inline unsigned long long asgw_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void asgw_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(ASGW_TILE) void asgw_init_kernel(int B, int N, int G, void* ws) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const AsgwView v = asgw_view(ws, B, b, N);
  for (int i = g * ASGW_TILE + threadIdx.x; i < N; i += G * ASGW_TILE) {
    v.price[i] = 0;
    v.hb[i] = 0;
    v.bidder[i] = ~0ull;
    v.gof[i] = i;  // (N = 1: the identity; every phase starts from -1)
  }
  if (g == 0 && threadIdx.x == 0) {
    AsgwCtl c;
    memset(&c, 0, sizeof(c));
    for (int d = 0; d < 3; ++d) c.lo[d] = ~0ull;
    asgw_ctl(ws)[b] = c;
    if (b == 0) *(unsigned*)ws = 0;
  }
}

__global__ __launch_bounds__(ASGW_TILE) void asgw_box_kernel(int B, int N, int D, int G, const double* __restrict__ start,
                                                             const double* __restrict__ goal, void* ws) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const double* sb = start + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int k = g * ASGW_TILE + threadIdx.x; k < 2 * N; k += G * ASGW_TILE) {
    const double* p = k < N ? sb + (int64_t)k * D : gb + (int64_t)(k - N) * D;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < D) {
        const double v = p[d];
        if (!(fabs(v) <= 1.7976931348623157e308)) bad = 1;  // NaN or infinite
        lo[d] = fmin(lo[d], v);
        hi[d] = fmax(hi[d], v);
      }
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    for (int d = 0; d < 3; ++d) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, 64));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, 64));
    }
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    AsgwCtl* c = asgw_ctl(ws) + b;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < D) {
        atomicMin(&c->lo[d], asgw_enc(lo[d]));
        atomicMax(&c->hi[d], asgw_enc(hi[d]));
      }
    }
    if (bad) atomicOr(&c->bad, 1);
  }
}

// (v1, j1, v2) := the best value with the lowest index and the best of all the others, of the union of two such triples
__device__ inline void asgw_merge(long long& v1, long long& v2, int& j1, long long ov1, long long ov2, int oj1) {
  if (ov1 > v1 || (ov1 == v1 && oj1 < j1)) {
    v2 = v1 > ov2 ? v1 : ov2;
    v1 = ov1;
    j1 = oj1;
  } else {
    v2 = v2 > ov1 ? v2 : ov1;
  }
}

// One wave, PB persons, the goals [jbeg, jend): per person the best value v_ij = a_ij - p_j (lowest j on ties), the second
// best and the argmax, in every lane.  Each goal and its price are loaded once for the PB persons.
template <int PB>
__device__ __forceinline__ void asgw_scan(const double* __restrict__ sb, const double* __restrict__ gb, const long long* price,
                                          int D, int sh, long long np1, const int (&pi)[PB], int jbeg, int jend, int lane,
                                          long long (&v1)[PB], long long (&v2)[PB], int (&j1)[PB]) {
#pragma clang fp contract(off)
  double a[PB][3];
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    a[q][0] = sb[(int64_t)pi[q] * D];
    a[q][1] = sb[(int64_t)pi[q] * D + 1];
    a[q][2] = D == 3 ? sb[(int64_t)pi[q] * D + 2] : 0.0;
    v1[q] = v2[q] = LLONG_MIN;
    j1[q] = INT_MAX;
  }
  for (int j = jbeg + lane; j < jend; j += 64) {
    double g[3];
    g[0] = gb[(int64_t)j * D];
    g[1] = gb[(int64_t)j * D + 1];
    g[2] = D == 3 ? gb[(int64_t)j * D + 2] : 0.0;
    const long long p = price[j];
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      const long long v = -np1 * asg_cost(a[q], g, D, sh) - p;
      if (v > v1[q]) {
        v2[q] = v1[q];
        v1[q] = v;
        j1[q] = j;
      } else if (v > v2[q]) {
        v2[q] = v;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < PB; ++q) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const long long ov1 = __shfl_xor(v1[q], off, 64), ov2 = __shfl_xor(v2[q], off, 64);
      const int oj1 = __shfl_xor(j1[q], off, 64);
      asgw_merge(v1[q], v2[q], j1[q], ov1, ov2, oj1);
    }
  }
}

// the end of step A for one person (N >= 2: j1 < N and v2 is a value): its bid, folded into the goal's highest (positive: a
// bid exceeds the price it was computed from by at least eps >= 1)
__device__ inline void asgw_place_bid(const AsgwView& v, const long long* price, int person, long long v1, long long v2, int j1,
                                      long long eps) {
  const long long bid = price[j1] + (v1 - v2) + eps;
  v.mybid[person] = bid;
  v.gof[person] = -2 - j1;
  atomicMax(&v.hb[j1], (unsigned long long)bid);
}

// step C for one bidder
__device__ inline void asgw_claim(const AsgwView& v, int i, unsigned long long key_base) {
  const int j = -2 - v.gof[i];
  if (asgw_load(&v.hb[j]) == (unsigned long long)v.mybid[i]) atomicMin(&v.bidder[j], key_base | (unsigned)i);
}

// step D for one bidder: returns the person that is unassigned afterwards (the loser itself, the previous owner of the goal
// it won) or -1.  One winner per goal; only it touches the goal's words and the previous owner's entry.
__device__ inline int asgw_handover(const AsgwView& v, long long* price, int i, unsigned long long key_base) {
  const int j = -2 - v.gof[i];
  if (asgw_load(&v.bidder[j]) != (key_base | (unsigned)i)) {
    v.gof[i] = -1;
    return i;
  }
  const int prev = v.owner[j];
  price[j] = (long long)asgw_load(&v.hb[j]);
  asgw_store(&v.hb[j], 0);
  v.owner[j] = i;
  v.gof[i] = j;
  if (prev >= 0) v.gof[prev] = -1;
  return prev;
}

__device__ inline unsigned long long asgw_key_base(long long round_no) {
  return (ASGW_KEY_TOP - (unsigned long long)round_no) << 17;
}

// ---- a wide round: three launches ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASGW_TILE) void asgw_bid_kernel(int B, int N, int D, int G, const double* __restrict__ start,
                                                             const double* __restrict__ goal, void* ws) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const AsgwCtl* c = asgw_ctl(ws) + b;
  if (c->done || !c->wide) return;
  const int nbid = c->nbid, sh = c->shift;
  const long long eps = c->eps, np1 = (long long)N + 1;
  const AsgwView v = asgw_view(ws, B, b, N);
  const int* list = v.list(c->cur);
  const double* sb = start + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WAVES = ASGW_TILE / 64;
  for (int first = (g * WAVES + wave) * ASGW_PB; first < nbid; first += G * WAVES * ASGW_PB) {
    int pi[ASGW_PB], j1[ASGW_PB];
    long long v1[ASGW_PB], v2[ASGW_PB];
#pragma unroll
    for (int q = 0; q < ASGW_PB; ++q) pi[q] = list[first + q < nbid ? first + q : first];
    asgw_scan<ASGW_PB>(sb, gb, v.price, D, sh, np1, pi, 0, N, lane, v1, v2, j1);
#pragma unroll
    for (int q = 0; q < ASGW_PB; ++q)
      if (lane == q && first + q < nbid) asgw_place_bid(v, v.price, pi[q], v1[q], v2[q], j1[q], eps);
  }
}

__global__ __launch_bounds__(ASGW_TILE) void asgw_claim_kernel(int B, int N, int G, void* ws) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const AsgwCtl* c = asgw_ctl(ws) + b;
  if (c->done || !c->wide) return;
  const int nbid = c->nbid;
  const AsgwView v = asgw_view(ws, B, b, N);
  const int* list = v.list(c->cur);
  const unsigned long long key_base = asgw_key_base(c->round_no);
  for (int k = g * ASGW_TILE + threadIdx.x; k < nbid; k += G * ASGW_TILE) asgw_claim(v, list[k], key_base);
}

__global__ __launch_bounds__(ASGW_TILE) void asgw_handover_kernel(int B, int N, int G, void* ws) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  AsgwCtl* c = asgw_ctl(ws) + b;
  if (c->done || !c->wide) return;
  const int nbid = c->nbid, cur = c->cur;
  const AsgwView v = asgw_view(ws, B, b, N);
  const int* list = v.list(cur);
  int* out = v.list(cur ^ 1);
  const unsigned long long key_base = asgw_key_base(c->round_no);
  const int lane = threadIdx.x & 63;
  for (int k0 = g * ASGW_TILE; k0 < nbid; k0 += G * ASGW_TILE) {  // (uniform per wave: the ballots below)
    const int k = k0 + threadIdx.x;
    const int left = k < nbid ? asgw_handover(v, v.price, list[k], key_base) : -1;
    // one atomicAdd per wave reserves the places of its entries of the next list
    const unsigned long long m = __ballot(left >= 0);
    int at = 0;
    if (lane == 0 && m) at = atomicAdd(&c->next, __popcll(m));
    at = __shfl(at, 0, 64);
    if (left >= 0) out[at + __popcll(m & ((1ull << lane) - 1))] = left;
  }
}

// ---- the control kernel, with the narrow rounds -----------------------------------------------------------------------------
struct AsgwPart {
  long long v1, v2;
  int j1, pad;
};

template <bool LDS>
__global__ __launch_bounds__(1024) void asgw_control_kernel(int B, int N, int D, const double* __restrict__ start,
                                                            const double* __restrict__ goal, void* ws, long long guard,
                                                            int min_bidders, int* bad_flag, int* done_flag) {
#pragma clang fp contract(off)
  extern __shared__ long long s_price[];  // [N] (LDS form only)
  __shared__ AsgwPart s_part[16];
  __shared__ int s_cnt[2];

  const int b = blockIdx.x;
  AsgwCtl* c = asgw_ctl(ws) + b;
  if (c->done) return;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  const AsgwView v = asgw_view(ws, B, b, N);
  const double* sb = start + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  const long long np1 = (long long)N + 1;

  // the scenario's state: every thread carries the same copy, thread 0 writes it back
  long long eps = c->eps, r = c->r, rounds = c->rounds, bids = c->bids, round_no = c->round_no;
  int sh = c->shift, phases = c->phases, status = c->status, cur = c->cur, nbid = c->nbid;
  const int started = c->started, was_wide = c->wide, next = c->next;

  bool done = false, wide = false;
  if (!started) {  // the quantisation, from the box
    int anybad = c->bad;
    double Bd = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < D) {
        const double span = asgw_dec(c->hi[d]) - asgw_dec(c->lo[d]);
        Bd = d == 0 ? span * span : Bd + span * span;
      }
    }
    if (!(Bd <= 1.7976931348623157e308)) anybad = 1;  // the range overflows
    long long top = 0;
    sh = 0;
    if (!anybad && Bd > 0.0) {
      int e;
      (void)frexp(Bd, &e);
      sh = 31 - e;
      top = (long long)ldexp(Bd, sh);
    }
    const long long e0 = (np1 * top) / 2;
    eps = e0 > 1 ? e0 : 1;
    nbid = 0;
    if (anybad) {  // the host turns the flag into SCP_ERR_INVALID
      status = 2;
      sh = 0;
      done = true;
      if (tid == 0) *bad_flag = 1;
    } else if (N < 2) {
      done = true;
    }
  } else if (was_wide) {  // the launches before this one ran the round that was counted last
    cur ^= 1;
    nbid = next;
  }
  __syncthreads();  // (thread 0 rewrites the block at the end; everybody has read it)

  bool loaded = false;  // (LDS form) the prices are in LDS and go back at the end
  long long* price = LDS ? s_price : v.price;
  while (!done) {  // (everything tested here is workgroup-uniform)
    if (nbid == 0) {  // the phase is over, or none has begun
      if (phases > 0) {
        rounds += r;
        if (eps == 1) {
          done = true;
          break;
        }
        eps = eps / 4 > 1 ? eps / 4 : 1;
      }
      ++phases;
      r = 0;
      nbid = N;
      for (int i = tid; i < N; i += nthr) {
        v.owner[i] = -1;
        v.gof[i] = -1;
        v.list(cur)[i] = i;
      }
      __syncthreads();
      continue;
    }
    if (r == guard) {
      status = 1;
      rounds += r;
      done = true;
      break;
    }
    ++r;
    bids += nbid;
    ++round_no;
    if (nbid >= min_bidders) {
      wide = true;
      break;
    }

    // ---- a narrow round ----
    if (LDS && !loaded) {
      for (int i = tid; i < N; i += nthr) s_price[i] = v.price[i];
      loaded = true;
      __syncthreads();
    }
    if (tid == 0) s_cnt[cur ^ 1] = 0;  // (read last before the barriers of the previous round; D adds to it after two more)
    const int* list = v.list(cur);
    const unsigned long long key_base = asgw_key_base(round_no);
    // A: S waves per bidder, each over a stretch of the goals; then one thread per bidder folds the S partial results
    int S = nbid >= nwave ? 1 : nwave / nbid;
    if (S > (N + 63) / 64) S = (N + 63) / 64;
    const int per = nwave / S, seg = (((N + S - 1) / S) + 63) & ~63;
    for (int base = 0; base < nbid; base += per) {
      const int slot = wave / S, s = wave - slot * S;
      if (slot < per && base + slot < nbid) {
        const int pi[1] = {list[base + slot]};
        long long v1[1], v2[1];
        int j1[1];
        const int jbeg = s * seg < N ? s * seg : N, jend = jbeg + seg < N ? jbeg + seg : N;
        asgw_scan<1>(sb, gb, price, D, sh, np1, pi, jbeg, jend, lane, v1, v2, j1);
        if (lane == 0) s_part[wave] = AsgwPart{v1[0], v2[0], j1[0], 0};
      }
      __syncthreads();
      if (tid < per && base + tid < nbid) {
        AsgwPart p = s_part[tid * S];
        for (int t = 1; t < S; ++t) {
          const AsgwPart o = s_part[tid * S + t];
          asgw_merge(p.v1, p.v2, p.j1, o.v1, o.v2, o.j1);
        }
        asgw_place_bid(v, price, list[base + tid], p.v1, p.v2, p.j1, eps);
      }
      __syncthreads();
    }
    // C
    for (int k = tid; k < nbid; k += nthr) asgw_claim(v, list[k], key_base);
    __syncthreads();
    // D
    for (int k = tid; k < nbid; k += nthr) {
      const int left = asgw_handover(v, price, list[k], key_base);
      if (left >= 0) v.list(cur ^ 1)[atomicAdd(&s_cnt[cur ^ 1], 1)] = left;
    }
    __syncthreads();
    cur ^= 1;
    nbid = s_cnt[cur];
  }
  if (LDS && loaded)
    for (int i = tid; i < N; i += nthr) v.price[i] = s_price[i];

  if (tid == 0) {
    c->eps = eps;
    c->r = r;
    c->rounds = rounds;
    c->bids = bids;
    c->round_no = round_no;
    c->shift = sh;
    c->phases = phases;
    c->status = status;
    c->started = 1;
    c->wide = wide ? 1 : 0;
    c->cur = cur;
    c->nbid = nbid;
    c->next = 0;
    if (done) {
      c->done = 1;
      if (atomicAdd((unsigned*)ws, 1u) + 1u == (unsigned)B) {  // the last scenario of the call
        *done_flag = 1;
        __threadfence_system();
      }
    }
  }
}

// ---- results ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASGW_TILE) void asgw_result_kernel(int B, int N, int D, int G, const double* __restrict__ start,
                                                                const double* __restrict__ goal, void* ws,
                                                                int32_t* __restrict__ goal_of, long long* __restrict__ prices) {
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  AsgwCtl* c = asgw_ctl(ws) + b;
  const int status = c->done ? c->status : 1, sh = c->shift;  // (a scenario that is not done: the host reports the call failed)
  const AsgwView v = asgw_view(ws, B, b, N);
  const double* sb = start + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  long long cq = 0, ci = 0;
  for (int i = g * ASGW_TILE + threadIdx.x; i < N; i += G * ASGW_TILE) {
    int gi = status == 0 ? v.gof[i] : i;
    if ((unsigned)gi >= (unsigned)N) gi = i;  // (cannot happen for status 0; nothing is read out of bounds)
    goal_of[(int64_t)b * N + i] = gi;
    if (prices) prices[(int64_t)b * N + i] = status == 2 ? 0 : v.price[i];
    if (status != 2) {
      const long long cii = asg_cost(sb + (int64_t)i * D, gb + (int64_t)i * D, D, sh);
      ci += cii;
      cq += gi == i ? cii : asg_cost(sb + (int64_t)i * D, gb + (int64_t)gi * D, D, sh);
    }
  }
  cq = asg_wave_sum(cq);
  ci = asg_wave_sum(ci);
  if ((threadIdx.x & 63) == 0 && status != 2) {
    atomicAdd(&c->cq, (unsigned long long)cq);
    atomicAdd(&c->ci, (unsigned long long)ci);
  }
}

__global__ __launch_bounds__(ASGW_TILE) void asgw_stats_kernel(int B, void* ws, scp_assign_stats* __restrict__ stats) {
  const int b = blockIdx.x * ASGW_TILE + threadIdx.x;
  if (b >= B) return;
  const AsgwCtl* c = asgw_ctl(ws) + b;
  scp_assign_stats st;
  st.cost_q = (int64_t)c->cq;
  st.cost_q_identity = (int64_t)c->ci;
  st.quantum = c->status == 2 ? 0.0 : ldexp(1.0, -c->shift);
  st.rounds = c->rounds;
  st.bids = c->bids;
  st.phases = c->phases;
  st.status = c->status;
  stats[b] = st;
}

// workgroups per scenario of a kernel with `per_wg` items per workgroup and `items` items, within `budget` workgroups a call
int asgw_groups(int64_t items, int per_wg, int B, int budget) {
  int64_t g = (items + per_wg - 1) / per_wg;
  const int64_t most = budget / B > 1 ? budget / B : 1;
  if (g > most) g = most;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

extern "C" int scp_assign_goals_wide(scp_ctx* ctx, int B, int N, int D, const double* start, const double* goal,
                                     int32_t* goal_of, int64_t* prices, int64_t max_rounds_per_phase, scp_assign_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, start && goal && goal_of && stats, "assign_goals_wide: NULL argument");
  SCP_REQUIRE(ctx, B >= 1, "assign_goals_wide: B = %d (need B >= 1)", B);
  SCP_REQUIRE(ctx, N >= 1 && N <= ASGW_MAXN, "assign_goals_wide: N = %d (need 1 <= N <= %d)", N, ASGW_MAXN);
  SCP_REQUIRE(ctx, D == 2 || D == 3, "assign_goals_wide: D = %d (need 2 or 3)", D);
  static_assert(sizeof(scp_assign_stats) == 48, "scp_assign_stats is 48 bytes");
  const long long guard = max_rounds_per_phase > 0 ? (long long)max_rounds_per_phase : 256ll * N + 4096;
  // The forks.  A narrow round costs one workgroup about ceil(bidders / 16) sweeps of N / 64 steps, a wide one three launches
  // and the control kernel's: the call's own threshold keeps the narrow round below ~128 such steps.
  int min_bidders = ctx->asgw_min_bidders;
  if (min_bidders == 0) {
    min_bidders = 131072 / N;
    min_bidders = min_bidders < 8 ? 8 : (min_bidders > 1024 ? 1024 : min_bidders);
  }
  const bool never_wide = min_bidders >= N;  // (a phase's first round has N bidders: ">= N" means "no round")
  if (never_wide) min_bidders = INT_MAX;
  const bool lds = ctx->asgw_prices_in_lds != 0 && N <= ASGW_LDS_MAXN;
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = asg_host_flag(ctx)) return rc;
  const size_t need = ASGW_HEADER + sizeof(AsgwCtl) * (size_t)B + ASGW_BYTES_PER_ENTRY * (size_t)N * (size_t)B;
  if (const int rc = scp_ctx_ensure_bytes(ctx, &ctx->asgw_ws, &ctx->asgw_ws_bytes, need)) return rc;
  void* ws = ctx->asgw_ws;
  const size_t lds_bytes = lds ? sizeof(long long) * (size_t)N : 0;
  if (lds_bytes > 48 * 1024)
    SCP_HIP_CHECK(ctx, scp_raise_lds_limit(ctx->device, reinterpret_cast<const void*>(asgw_control_kernel<true>), lds_bytes));
  // small scenarios: four waves, so that several control workgroups share a compute unit; large ones: sixteen
  const int ctl_threads = ctx->asgw_control_threads ? ctx->asgw_control_threads : (N <= 512 ? 256 : 1024);
  const int g_sweep = asgw_groups(2 * (int64_t)N, 4 * ASGW_TILE, B, 1 << 20);       // init, box, results
  const int g_bid = asgw_groups(N, (ASGW_TILE / 64) * ASGW_PB, B, 1 << 20);       // one wave per ASGW_PB bidders
  const int g_list = asgw_groups(N, ASGW_TILE, B, 1 << 20);                       // claim, handover
  hipStream_t st = ctx->stream;
  volatile int* hflag = ctx->h_gen_flag;
  hflag[0] = 0;
  hflag[1] = 0;
  int* d_bad = ctx->d_gen_flag;
  int* d_done = ctx->d_gen_flag + 1;
  auto control = [&]() {
    if (lds)
      asgw_control_kernel<true><<<B, ctl_threads, lds_bytes, st>>>(B, N, D, start, goal, ws, guard, min_bidders, d_bad, d_done);
    else
      asgw_control_kernel<false><<<B, ctl_threads, 0, st>>>(B, N, D, start, goal, ws, guard, min_bidders, d_bad, d_done);
  };
  asgw_init_kernel<<<B * g_sweep, ASGW_TILE, 0, st>>>(B, N, g_sweep, ws);
  asgw_box_kernel<<<B * g_sweep, ASGW_TILE, 0, st>>>(B, N, D, g_sweep, start, goal, ws);
  control();
  hipError_t e = hipGetLastError();
  bool finished = never_wide;  // (one control launch then runs every round)
  // a step runs at least one round of every unfinished scenario, or ends one of its phases (at most 25: eps_0 < 2^47)
  const long long max_steps = guard > (LLONG_MAX >> 6) ? LLONG_MAX : 32 * (guard + 2);
  long long steps = 0;
  for (int batch = 4; e == hipSuccess && !finished && steps < max_steps; batch = batch < 64 ? batch * 4 : 64) {
    for (int s = 0; s < batch; ++s) {
      asgw_bid_kernel<<<B * g_bid, ASGW_TILE, 0, st>>>(B, N, D, g_bid, start, goal, ws);
      asgw_claim_kernel<<<B * g_list, ASGW_TILE, 0, st>>>(B, N, g_list, ws);
      asgw_handover_kernel<<<B * g_list, ASGW_TILE, 0, st>>>(B, N, g_list, ws);
      control();
    }
    steps += batch;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    finished = hflag[1] != 0;
  }
  if (e == hipSuccess) {
    asgw_result_kernel<<<B * g_sweep, ASGW_TILE, 0, st>>>(B, N, D, g_sweep, start, goal, ws, goal_of, (long long*)prices);
    asgw_stats_kernel<<<scp_cdiv(B, ASGW_TILE), ASGW_TILE, 0, st>>>(B, ws, stats);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return scp_fail(ctx, SCP_ERR_HIP, "assign_goals_wide: %s", hipGetErrorString(e));
  SCP_REQUIRE(ctx, hflag[0] == 0, "assign_goals_wide: a coordinate is not finite, or the range of the points overflows");
  if (hflag[1] == 0) return scp_fail(ctx, SCP_ERR_HIP, "assign_goals_wide: the auction did not finish within its step bound");
  return SCP_OK;
}
