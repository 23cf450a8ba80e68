// Scenario family "grid-swap-device": B grid-swap scenarios per call (include/scp_hip.h states the algorithm; the numpy
// restatement the tests compare against bit for bit is tests/scenario_device_ref.py).
//
//   gen_starts_kernel   one thread per (scenario, agent): jittered grid starts, z of the layer, per-scenario scratch reset
//   gen_draw_kernel     one 256-thread workgroup per (scenario, block) due in this sweep, one candidate permutation per
//                       thread; the block's starts and cells in LDS, the pick by wave64 shuffles then LDS (index-ordered)
//   gen_pair_kernel     tiled pair pass per scenario: CONFLICT flags blocks (plain int stores, every writer stores 1),
//                       FINAL keeps min d^2 (64-bit integer atomicMin on the bit pattern of a non-negative double) and the
//                       count of cross-block conflicts left
//   gen_finish_kernel   one workgroup per scenario: space box and scp_gen_stats
// No floating-point atomics; no grid-wide barrier (the host loop syncs once per sweep on a mapped 4-byte word).
#include "scp_common.h"
#include "scp_line_device.h"

#include <cmath>
#include <vector>

namespace {

constexpr int GEN_T = 256;      // candidates per round = threads per draw workgroup
constexpr int GEN_MAXM = 64;    // agents per block (block <= 8)
constexpr int GEN_TILE = 256;   // agents per tile of the pair pass
constexpr uint64_t TAG_START = 1, TAG_PERM = 2, TAG_GOAL = 3;

__host__ __device__ inline uint64_t gen_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// h of the key (tag, layer, block, sweep, round, cand) before its lane: gen_mix(prefix ^ lane) is the number
__device__ inline uint64_t gen_prefix(uint64_t seed, uint64_t tag, uint64_t layer, uint64_t block, uint64_t sweep,
                                      uint64_t round, uint64_t cand) {
  uint64_t h = gen_mix(seed);
  h = gen_mix(h ^ tag);
  h = gen_mix(h ^ layer);
  h = gen_mix(h ^ block);
  h = gen_mix(h ^ sweep);
  h = gen_mix(h ^ round);
  return gen_mix(h ^ cand);
}

__device__ inline double gen_coord(int cell, double pitch, double jitter, uint64_t h) {
#pragma clang fp contract(off)  // every product rounded before it is added, as numpy does
  const double u = (double)(h >> 11) * 0x1.0p-53;
  const double j = (2.0 * u - 1.0) * jitter;
  return (double)cell * pitch + j;
}

// pick order of two candidates: acceptable (d2 >= thr) before not; among acceptable the lower index; otherwise the larger
// d2, then the lower index
__device__ inline bool gen_better(double da, int ta, double db, int tb, double thr) {
  const bool oa = da >= thr, ob = db >= thr;
  if (oa != ob) return oa;
  if (oa) return ta < tb;
  if (da != db) return da > db;
  return ta < tb;
}

struct GenShape {
  int N, D, per, side, nblk;
  double pitch, jitter, layer_gap, thr;  // thr = min_sep^2
};

__global__ __launch_bounds__(256) void gen_starts_kernel(GenShape g, int B, const uint64_t* __restrict__ seeds,
                                                         double* __restrict__ init, double* __restrict__ goal,
                                                         unsigned long long* __restrict__ minbits,
                                                         unsigned long long* __restrict__ conflicts, int* __restrict__ swept) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * g.N) return;
  const int b = (int)(t / g.N), k = (int)(t - (int64_t)b * g.N);
  const int L = k / g.per, c = k - L * g.per;
  const uint64_t pre = gen_prefix(seeds[b], TAG_START, (uint64_t)L, 0, 0, 0, 0);
  double* a = init + t * g.D;
  a[0] = gen_coord(c / g.side, g.pitch, g.jitter, gen_mix(pre ^ (uint64_t)(2 * c)));
  a[1] = gen_coord(c % g.side, g.pitch, g.jitter, gen_mix(pre ^ (uint64_t)(2 * c + 1)));
  if (g.D == 3) {
    const double z = (double)L * g.layer_gap;
    a[2] = z;
    goal[t * g.D + 2] = z;
  }
  if (k == 0) {
    minbits[b] = 0x7FF0000000000000ull;  // +inf
    conflicts[b] = 0;
    swept[b] = 0;
  }
}

// blk: [nblk][4] = first member (into `members`), m, layer, owner id in the layer
__global__ __launch_bounds__(GEN_T) void gen_draw_kernel(GenShape g, int sweep, int rounds, const uint64_t* __restrict__ seeds,
                                                         const int* __restrict__ blk, const int* __restrict__ members,
                                                         const double* __restrict__ init, double* __restrict__ goal,
                                                         int* __restrict__ flags, int* __restrict__ unmet) {
#pragma clang fp contract(off)
  __shared__ uint8_t s_perm[GEN_MAXM * GEN_T];  // [slot][candidate]: consecutive candidates in consecutive bytes
  __shared__ double s_ax[GEN_MAXM], s_ay[GEN_MAXM];
  __shared__ int s_cx[GEN_MAXM], s_cy[GEN_MAXM], s_agent[GEN_MAXM];
  __shared__ uint8_t s_best[GEN_MAXM];
  __shared__ double s_wd[GEN_T / 64];
  __shared__ int s_wt[GEN_T / 64];
  __shared__ double s_pick_d;
  __shared__ int s_pick_t;

  const int b = blockIdx.x / g.nblk, o_g = blockIdx.x - b * g.nblk;
  const int fi = b * g.nblk + o_g;
  if (sweep > 0 && flags[fi] == 0) return;  // (workgroup-uniform)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first = blk[4 * o_g], m = blk[4 * o_g + 1], L = blk[4 * o_g + 2], own = blk[4 * o_g + 3];
  const uint64_t seed = seeds[b];
  if (tid < m) {
    const int k = members[first + tid];
    const int c = k - L * g.per;
    s_agent[tid] = k;
    s_cx[tid] = c / g.side;
    s_cy[tid] = c % g.side;
    const double* a = init + ((int64_t)b * g.N + k) * g.D;
    s_ax[tid] = a[0];
    s_ay[tid] = a[1];
  }
  __syncthreads();

  double best_d = -1.0;
  int best_r = 0, best_t = 0;
  for (int r = 0; r < rounds; ++r) {
    // Fisher-Yates of this thread's candidate, in its LDS column
    const uint64_t pp = gen_prefix(seed, TAG_PERM, (uint64_t)L, (uint64_t)own, (uint64_t)sweep, (uint64_t)r, (uint64_t)tid);
    const uint64_t pg = gen_prefix(seed, TAG_GOAL, (uint64_t)L, (uint64_t)own, (uint64_t)sweep, (uint64_t)r, (uint64_t)tid);
    for (int i = 0; i < m; ++i) s_perm[i * GEN_T + tid] = (uint8_t)i;
    for (int i = m - 1; i >= 1; --i) {
      const uint64_t h = gen_mix(pp ^ (uint64_t)i);
      const int j = (int)(((h >> 32) * (uint64_t)(i + 1)) >> 32);
      const uint8_t vi = s_perm[i * GEN_T + tid], vj = s_perm[j * GEN_T + tid];
      s_perm[i * GEN_T + tid] = vj;
      s_perm[j * GEN_T + tid] = vi;
    }
    // score: smallest d^2 over the block's pairs (goals recomputed from the permutation and the hash, nothing stored)
    double d2min = INFINITY;
    for (int i = 0; i + 1 < m; ++i) {
      const int pi = s_perm[i * GEN_T + tid];
      const double gix = gen_coord(s_cx[pi], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * i)));
      const double giy = gen_coord(s_cy[pi], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * i + 1)));
      const double aix = s_ax[i], aiy = s_ay[i];
      for (int j = i + 1; j < m; ++j) {
        const int pj = s_perm[j * GEN_T + tid];
        const double gjx = gen_coord(s_cx[pj], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * j)));
        const double gjy = gen_coord(s_cy[pj], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * j + 1)));
        const double d2 = gen_d2(aix - s_ax[j], aiy - s_ay[j], gix - gjx, giy - gjy);
        d2min = d2 < d2min ? d2 : d2min;
      }
    }
    // the round's pick: wave64 butterfly (every lane ends with the wave's pick), then the four waves through LDS
    double pd = d2min;
    int pt = tid;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(pd, off, 64);
      const int ot = __shfl_xor(pt, off, 64);
      if (gen_better(od, ot, pd, pt, g.thr)) {
        pd = od;
        pt = ot;
      }
    }
    if (lane == 0) {
      s_wd[wave] = pd;
      s_wt[wave] = pt;
    }
    __syncthreads();
    if (tid == 0) {
      double bd = s_wd[0];
      int bt = s_wt[0];
      for (int w = 1; w < GEN_T / 64; ++w)
        if (gen_better(s_wd[w], s_wt[w], bd, bt, g.thr)) {
          bd = s_wd[w];
          bt = s_wt[w];
        }
      s_pick_d = bd;
      s_pick_t = bt;
    }
    __syncthreads();
    const double rd = s_pick_d;
    const int rt = s_pick_t;
    if (rd > best_d) {  // (the same in every thread)
      best_d = rd;
      best_r = r;
      best_t = rt;
    }
    if (rd >= g.thr) break;
    __syncthreads();  // s_perm and the pick are rewritten by the next round
  }

  // the kept candidate's permutation, recomputed once
  if (tid == 0) {
    const uint64_t pp = gen_prefix(seed, TAG_PERM, (uint64_t)L, (uint64_t)own, (uint64_t)sweep, (uint64_t)best_r,
                                   (uint64_t)best_t);
    for (int i = 0; i < m; ++i) s_best[i] = (uint8_t)i;
    for (int i = m - 1; i >= 1; --i) {
      const uint64_t h = gen_mix(pp ^ (uint64_t)i);
      const int j = (int)(((h >> 32) * (uint64_t)(i + 1)) >> 32);
      const uint8_t v = s_best[i];
      s_best[i] = s_best[j];
      s_best[j] = v;
    }
    unmet[fi] = best_d >= g.thr ? 0 : 1;
    if (sweep > 0) flags[fi] = 0;
  }
  __syncthreads();
  if (tid < m) {
    const uint64_t pg = gen_prefix(seed, TAG_GOAL, (uint64_t)L, (uint64_t)own, (uint64_t)sweep, (uint64_t)best_r,
                                   (uint64_t)best_t);
    const int p = s_best[tid];
    double* q = goal + ((int64_t)b * g.N + s_agent[tid]) * g.D;
    q[0] = gen_coord(s_cx[p], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * tid)));
    q[1] = gen_coord(s_cy[p], g.pitch, g.jitter, gen_mix(pg ^ (uint64_t)(2 * tid + 1)));
  }
}

// One workgroup per (scenario, tile pair ti <= tj): thread i of tile ti against the 256 agents of tile tj staged in LDS.
// owner: global block id of every agent (blocks of one layer are consecutive, in owner order, so the larger global id of two
// agents of one layer is the larger owner id).  Layer of agent k = k / per.
template <bool FINAL>
__global__ __launch_bounds__(GEN_TILE) void gen_pair_kernel(GenShape g, int ntiles, int ntri, int sweep,
                                                            const double* __restrict__ init, const double* __restrict__ goal,
                                                            const int* __restrict__ owner, int* __restrict__ flags,
                                                            int* __restrict__ swept, int* host_flag,
                                                            unsigned long long* __restrict__ minbits,
                                                            unsigned long long* __restrict__ conflicts) {
#pragma clang fp contract(off)
  __shared__ double s_a[3][GEN_TILE], s_g[3][GEN_TILE];
  __shared__ int s_own[GEN_TILE];
  __shared__ unsigned long long s_min[GEN_TILE / 64], s_cnt[GEN_TILE / 64];
  __shared__ int s_any;

  const int b = blockIdx.x / ntri;
  int rem = blockIdx.x - b * ntri, ti = 0;
  while (rem >= ntiles - ti) {  // upper-triangle index -> (ti, tj)
    rem -= ntiles - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const int tid = threadIdx.x;
  const int D = g.D, N = g.N;
  const double* ib = init + (int64_t)b * N * D;
  const double* gb = goal + (int64_t)b * N * D;
  {
    const int j = tj * GEN_TILE + tid;
    if (j < N) {
      for (int d = 0; d < D; ++d) {
        s_a[d][tid] = ib[(int64_t)j * D + d];
        s_g[d][tid] = gb[(int64_t)j * D + d];
      }
      s_own[tid] = owner[j];
    }
    if (tid == 0) s_any = 0;
  }
  __syncthreads();
  const int i = ti * GEN_TILE + tid;
  double dmin = INFINITY;
  unsigned long long cnt = 0;
  bool flagged = false;
  if (i < N) {
    const double ax = ib[(int64_t)i * D], ay = ib[(int64_t)i * D + 1];
    const double gx = gb[(int64_t)i * D], gy = gb[(int64_t)i * D + 1];
    const double az = D == 3 ? ib[(int64_t)i * D + 2] : 0.0, gz = D == 3 ? gb[(int64_t)i * D + 2] : 0.0;
    const int oi = owner[i], li = i / g.per;
    const int jend = min(GEN_TILE, N - tj * GEN_TILE);
    for (int jj = (ti == tj ? tid + 1 : 0); jj < jend; ++jj) {
      const int j = tj * GEN_TILE + jj;
      const bool cross = (j / g.per == li) && s_own[jj] != oi;
      if (FINAL) {
        double d2;
        if (D == 3)
          d2 = gen_d2_3(ax - s_a[0][jj], ay - s_a[1][jj], az - s_a[2][jj], gx - s_g[0][jj], gy - s_g[1][jj],
                        gz - s_g[2][jj]);
        else
          d2 = gen_d2(ax - s_a[0][jj], ay - s_a[1][jj], gx - s_g[0][jj], gy - s_g[1][jj]);
        dmin = d2 < dmin ? d2 : dmin;
        if (cross && d2 < g.thr) ++cnt;
      } else if (cross) {
        const double d2 = gen_d2(ax - s_a[0][jj], ay - s_a[1][jj], gx - s_g[0][jj], gy - s_g[1][jj]);
        if (d2 < g.thr) {
          flags[b * g.nblk + max(oi, s_own[jj])] = 1;
          flagged = true;
        }
      }
    }
  }
  if (!FINAL) {
    if (flagged) s_any = 1;
    __syncthreads();
    if (tid == 0 && s_any) {
      swept[b] = sweep;
      *host_flag = 1;
    }
    return;
  }
  unsigned long long mb = (unsigned long long)__double_as_longlong(dmin);  // non-negative: the bits order like the values
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long om = __shfl_xor(mb, off, 64);
    mb = om < mb ? om : mb;
    cnt += __shfl_xor(cnt, off, 64);
  }
  if ((tid & 63) == 0) {
    s_min[tid >> 6] = mb;
    s_cnt[tid >> 6] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = s_min[0], c = s_cnt[0];
    for (int w = 1; w < GEN_TILE / 64; ++w) {
      m = s_min[w] < m ? s_min[w] : m;
      c += s_cnt[w];
    }
    atomicMin(&minbits[b], m);
    if (c) atomicAdd(&conflicts[b], c);
  }
}

__global__ __launch_bounds__(256) void gen_finish_kernel(GenShape g, double min_sep, const double* __restrict__ init,
                                                         const double* __restrict__ goal, const int* __restrict__ unmet,
                                                         const int* __restrict__ swept,
                                                         const unsigned long long* __restrict__ minbits,
                                                         const unsigned long long* __restrict__ conflicts,
                                                         double* __restrict__ space, scp_gen_stats* __restrict__ stats) {
  __shared__ double s_lo[3][4], s_hi[3][4];
  __shared__ int s_un[4];
  const int b = blockIdx.x, tid = threadIdx.x, D = g.D;
  const double* ib = init + (int64_t)b * g.N * D;
  const double* gb = goal + (int64_t)b * g.N * D;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = tid; k < g.N; k += 256)
    for (int d = 0; d < D; ++d) {
      const double a = ib[(int64_t)k * D + d], q = gb[(int64_t)k * D + d];
      lo[d] = fmin(lo[d], fmin(a, q));
      hi[d] = fmax(hi[d], fmax(a, q));
    }
  int un = 0;
  for (int o = tid; o < g.nblk; o += 256) un += unmet[b * g.nblk + o];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int d = 0; d < 3; ++d) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, 64));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, 64));
    }
    un += __shfl_xor(un, off, 64);
  }
  if ((tid & 63) == 0) {
    for (int d = 0; d < 3; ++d) {
      s_lo[d][tid >> 6] = lo[d];
      s_hi[d][tid >> 6] = hi[d];
    }
    s_un[tid >> 6] = un;
  }
  __syncthreads();
  if (tid == 0) {
    for (int d = 0; d < D; ++d) {
      double l = s_lo[d][0], h = s_hi[d][0];
      for (int w = 1; w < 4; ++w) {
        l = fmin(l, s_lo[d][w]);
        h = fmax(h, s_hi[d][w]);
      }
      space[(int64_t)b * 2 * D + d] = l - 2.0;
      space[(int64_t)b * 2 * D + D + d] = h + 2.0;
    }
    scp_gen_stats st;
    st.sweeps = swept[b];
    st.unmet_blocks = s_un[0] + s_un[1] + s_un[2] + s_un[3];
    st.conflicts = (int64_t)conflicts[b];
    st.min_approach = sqrt(__longlong_as_double((long long)minbits[b]));
    st.ok = st.min_approach >= min_sep ? 1 : 0;
    st.reserved = 0;
    stats[b] = st;
  }
}

size_t gen_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" void scp_gen_default_params(scp_gen_params* p) {
  if (!p) return;
  p->pitch = 2.0;
  p->jitter = 0.2;
  p->layer_gap = 2.0;
  p->min_sep = 0.3;
  p->block = 4;
  p->max_tries = 8192;
  p->sweeps = 20;
  p->reserved = 0;
}

extern "C" int scp_generate_grid_swap(scp_ctx* ctx, int B, int N, int D, const uint64_t* seeds, const scp_gen_params* p,
                                      double* init, double* goal, double* space, scp_gen_stats* stats) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, p && seeds && init && goal && space && stats, "generate_grid_swap: NULL argument");
  SCP_REQUIRE(ctx, B >= 1, "generate_grid_swap: B = %d (need B >= 1)", B);
  SCP_REQUIRE(ctx, N >= 1 && N <= 65536, "generate_grid_swap: N = %d (need 1 <= N <= 65536)", N);
  SCP_REQUIRE(ctx, D == 2 || D == 3, "generate_grid_swap: D = %d (need 2 or 3)", D);
  SCP_REQUIRE(ctx, p->block >= 2 && p->block <= 8, "generate_grid_swap: block = %d (need 2 <= block <= 8)", p->block);
  SCP_REQUIRE(ctx, std::isfinite(p->pitch) && std::isfinite(p->jitter) && p->jitter >= 0.0 && std::isfinite(p->layer_gap) &&
                       std::isfinite(p->min_sep) && p->min_sep >= 0.0,
              "generate_grid_swap: pitch / layer_gap must be finite, jitter and min_sep finite and >= 0");
  SCP_REQUIRE(ctx, p->sweeps >= 0 && p->sweeps <= 1000, "generate_grid_swap: sweeps = %d (need 0 .. 1000)", p->sweeps);

  // layout (integer searches: layers^3 >= N, side^2 >= per)
  int layers = 1;
  if (D == 3)
    while ((int64_t)layers * layers * layers < N) ++layers;
  const int per = (N + layers - 1) / layers;
  int side = 1;
  while ((int64_t)side * side < per) ++side;
  const int block = p->block, stride = side / block + 1;
  // blocks: [nblk][4] = first member, m, layer, owner id; members grouped by block; owner = global block id per agent
  std::vector<int> blk, members, owner(N);
  std::vector<int> key_first(stride * stride), key_cnt(stride * stride);
  int nblk = 0;
  for (int L = 0, base = 0; L < layers && base < N; ++L) {
    const int cnt = per < N - base ? per : N - base;
    std::fill(key_cnt.begin(), key_cnt.end(), 0);
    for (int c = 0; c < cnt; ++c) ++key_cnt[(c / side / block) * stride + (c % side) / block];
    int own = 0;
    for (int key = 0; key < stride * stride; ++key) {
      if (!key_cnt[key]) continue;
      key_first[key] = (int)members.size();
      blk.insert(blk.end(), {(int)members.size(), key_cnt[key], L, own++});
      members.resize(members.size() + key_cnt[key]);
      key_cnt[key] = 0;  // (reused as the fill count below)
    }
    for (int c = 0; c < cnt; ++c) {
      const int key = (c / side / block) * stride + (c % side) / block;
      const int slot = key_first[key] + key_cnt[key]++;
      members[slot] = base + c;
    }
    for (int o = 0; o < own; ++o) {
      const int* q = &blk[4 * (nblk + o)];
      for (int s = 0; s < q[1]; ++s) owner[members[q[0] + s]] = nblk + o;
    }
    nblk += own;
    base += cnt;
  }
  const int ntiles = (N + GEN_TILE - 1) / GEN_TILE, ntri = ntiles * (ntiles + 1) / 2;
  SCP_REQUIRE(ctx, (int64_t)B * nblk * GEN_T < INT32_MAX && (int64_t)B * ntri * GEN_TILE < INT32_MAX &&
                       (int64_t)B * N < INT32_MAX,
              "generate_grid_swap: B = %d scenarios of %d agents exceed one call's grid; split the batch", B, N);

  // workspace: seeds, blk, members, owner, flags, unmet, swept, minbits, conflicts
  const size_t o_seeds = 0, o_blk = gen_align(o_seeds + sizeof(uint64_t) * B);
  const size_t o_mem = gen_align(o_blk + sizeof(int) * blk.size()), o_own = gen_align(o_mem + sizeof(int) * N);
  const size_t o_flags = gen_align(o_own + sizeof(int) * N), o_unmet = gen_align(o_flags + sizeof(int) * (size_t)B * nblk);
  const size_t o_swept = gen_align(o_unmet + sizeof(int) * (size_t)B * nblk), o_min = gen_align(o_swept + sizeof(int) * B);
  const size_t o_cnt = gen_align(o_min + 8 * (size_t)B), total = gen_align(o_cnt + 8 * (size_t)B);
  SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = scp_ctx_ensure_bytes(ctx, &ctx->gen_ws, &ctx->gen_ws_bytes, total)) return rc;
  if (!ctx->h_gen_flag) {
    SCP_HIP_CHECK(ctx, hipHostMalloc((void**)&ctx->h_gen_flag, 64, hipHostMallocMapped));
    SCP_HIP_CHECK(ctx, hipHostGetDevicePointer((void**)&ctx->d_gen_flag, ctx->h_gen_flag, 0));
  }
  char* ws = (char*)ctx->gen_ws;
  uint64_t* d_seeds = (uint64_t*)(ws + o_seeds);
  int* d_blk = (int*)(ws + o_blk);
  int* d_mem = (int*)(ws + o_mem);
  int* d_own = (int*)(ws + o_own);
  int* d_flags = (int*)(ws + o_flags);
  int* d_unmet = (int*)(ws + o_unmet);
  int* d_swept = (int*)(ws + o_swept);
  unsigned long long* d_min = (unsigned long long*)(ws + o_min);
  unsigned long long* d_cnt = (unsigned long long*)(ws + o_cnt);
  hipStream_t st = ctx->stream;
  // (host sources: the stream is synchronised before this function returns, on every path after these copies)
  auto bail = [&](hipError_t e, const char* what) {
    (void)hipStreamSynchronize(st);
    return scp_fail(ctx, SCP_ERR_HIP, "generate_grid_swap: %s: %s", what, hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = hipMemcpyAsync(d_seeds, seeds, sizeof(uint64_t) * B, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_blk, blk.data(), sizeof(int) * blk.size(), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_mem, members.data(), sizeof(int) * N, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_own, owner.data(), sizeof(int) * N, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemsetAsync(d_flags, 0, sizeof(int) * (size_t)B * nblk, st)) != hipSuccess)
    return bail(e, "upload");

  GenShape g{N, D, per, side, nblk, p->pitch, p->jitter, p->layer_gap, p->min_sep * p->min_sep};
  const int rounds = p->max_tries / GEN_T > 1 ? p->max_tries / GEN_T : 1;
  const int starts_wg = (int)(((int64_t)B * N + 255) / 256);
  gen_starts_kernel<<<starts_wg, 256, 0, st>>>(g, B, d_seeds, init, goal, d_min, d_cnt, d_swept);
  gen_draw_kernel<<<B * nblk, GEN_T, 0, st>>>(g, 0, rounds, d_seeds, d_blk, d_mem, init, goal, d_flags, d_unmet);
  if ((e = hipGetLastError()) != hipSuccess) return bail(e, "launch");
  volatile int* hflag = ctx->h_gen_flag;
  for (int s = 1; s <= p->sweeps; ++s) {
    *hflag = 0;
    gen_pair_kernel<false><<<B * ntri, GEN_TILE, 0, st>>>(g, ntiles, ntri, s, init, goal, d_own, d_flags, d_swept,
                                                          ctx->d_gen_flag, d_min, d_cnt);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e, "launch");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return bail(e, "sweep");
    if (*hflag == 0) break;
    gen_draw_kernel<<<B * nblk, GEN_T, 0, st>>>(g, s, rounds, d_seeds, d_blk, d_mem, init, goal, d_flags, d_unmet);
  }
  gen_pair_kernel<true><<<B * ntri, GEN_TILE, 0, st>>>(g, ntiles, ntri, 0, init, goal, d_own, d_flags, d_swept,
                                                       ctx->d_gen_flag, d_min, d_cnt);
  gen_finish_kernel<<<B, 256, 0, st>>>(g, p->min_sep, init, goal, d_unmet, d_swept, d_min, d_cnt, space, stats);
  if ((e = hipGetLastError()) != hipSuccess) return bail(e, "launch");
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return bail(e, "finish");
  return SCP_OK;
}
