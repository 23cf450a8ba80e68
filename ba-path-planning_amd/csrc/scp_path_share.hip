// Static obstacles on gfx950, shared paths: the load and the overuse of a path set (scp_path_load) and the kernel that keeps
// the better of two sets for scp_negotiate_paths, whose driver and search live in scp_lattice_search.hip.  The rules are
// stated in include/scp_hip.h ("shared paths"); tests/shared_path_ref.py restates them.  Integers only, plain C++.
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"

namespace {

constexpr int SHARE_THREADS = 256;

// one thread per path entry (a grid-stride loop where there are more entries than threads): an entry of a found path adds one
// to its node.  Integer atomics commute, so the array does not depend on the order.
__global__ __launch_bounds__(SHARE_THREADS) void path_load_kernel(int N, int max_path, int nodes, const int32_t* __restrict__ path,
                                                                   const scp_path_info* __restrict__ info, uint32_t* load) {
  const int64_t entries = (int64_t)N * max_path, step = (int64_t)gridDim.x * SHARE_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * SHARE_THREADS + threadIdx.x; e < entries; e += step) {
    const scp_path_info r = info[e / max_path];
    if (r.status != 0 || e % max_path >= r.n_nodes) continue;
    const int node = path[e];
    if ((unsigned)node < (unsigned)nodes) atomicAdd(&load[node], 1u);
  }
}

// one thread per node: its excess over the capacity, summed over the wave by shuffles and over the workgroup's waves in
// LDS; one 64-bit atomic add per workgroup with an excess (*overuse is zero on entry)
__global__ __launch_bounds__(SHARE_THREADS) void path_overuse_kernel(int nodes, uint32_t capacity, const uint32_t* __restrict__ load,
                                                                      unsigned long long* overuse) {
  __shared__ unsigned long long part[SHARE_THREADS / 64];
  const int tid = threadIdx.x, node = blockIdx.x * SHARE_THREADS + tid;
  const uint32_t have = node < nodes ? load[node] : 0u;
  unsigned long long sum = have > capacity ? have - capacity : 0u;
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d, 64);
  if ((tid & 63) == 0) part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
    for (int w = 0; w < SHARE_THREADS / 64; ++w) total += part[w];
    if (total) atomicAdd(overuse, total);
  }
}

struct WordCopy {  // the four arrays of a path set as 32-bit words
  const uint32_t* src[4];
  uint32_t* dst[4];
  int64_t words[4];
};

// Every thread reads the same overuse words, so the branch is the whole grid's: the workgroups copy or return.  Nobody
// writes a word that anybody reads here (*best_round is only written).
__global__ __launch_bounds__(SHARE_THREADS) void keep_better_kernel(WordCopy c, const unsigned long long* __restrict__ overuse, int r,
                                                                     int32_t* best_round) {
  int best = 0;  // the earliest smallest of the earlier rounds
  for (int q = 1; q < r; ++q)
    if (overuse[q] < overuse[best]) best = q;
  const bool better = r == 0 || overuse[r] < overuse[best];
  if (blockIdx.x == 0 && threadIdx.x == 0) *best_round = better ? r : best;
  if (!better) return;
  const int64_t step = (int64_t)gridDim.x * SHARE_THREADS;
  for (int a = 0; a < 4; ++a)
    for (int64_t w = (int64_t)blockIdx.x * SHARE_THREADS + threadIdx.x; w < c.words[a]; w += step) c.dst[a][w] = c.src[a][w];
}

}  // namespace

int path_load_enqueue(scp_ctx* ctx, int N, int max_path, int nodes, const int32_t* path, const scp_path_info* info, int capacity,
                      uint32_t* load, uint64_t* overuse, bool clear_overuse) {
  SCP_HIP_CHECK(ctx, hipMemsetAsync(load, 0, (size_t)nodes * sizeof(uint32_t), ctx->stream));
  if (clear_overuse) SCP_HIP_CHECK(ctx, hipMemsetAsync(overuse, 0, sizeof(uint64_t), ctx->stream));
  const int64_t entries = (int64_t)N * max_path;
  const int blocks = entries > (int64_t)65536 * SHARE_THREADS ? 65536 : scp_cdiv(entries, SHARE_THREADS);
  hipLaunchKernelGGL(path_load_kernel, dim3(blocks), dim3(SHARE_THREADS), 0, ctx->stream, N, max_path, nodes, path, info, load);
  hipLaunchKernelGGL(path_overuse_kernel, dim3(scp_cdiv(nodes, SHARE_THREADS)), dim3(SHARE_THREADS), 0, ctx->stream, nodes,
                     (uint32_t)capacity, load, (unsigned long long*)overuse);
  return SCP_OK;
}

int keep_better_enqueue(scp_ctx* ctx, int N, int K, int D, int max_path, const PathSet& cur, const PathSet& best,
                        const uint64_t* overuse, int r, int32_t* best_round) {
  WordCopy c;
  const void* src[4] = {cur.ref, cur.path, cur.info, cur.path_cost};
  void* dst[4] = {best.ref, best.path, best.info, best.path_cost};
  const int64_t words[4] = {(int64_t)N * (K + 1) * D * 2, (int64_t)N * max_path, (int64_t)N * 4, (int64_t)N};
  int64_t most = 0;
  for (int a = 0; a < 4; ++a) {
    c.src[a] = (const uint32_t*)src[a];
    c.dst[a] = (uint32_t*)dst[a];
    c.words[a] = words[a];
    most = words[a] > most ? words[a] : most;
  }
  static_assert(sizeof(scp_path_info) == 16, "scp_path_info is four words");
  const int blocks = most > (int64_t)1024 * 4 * SHARE_THREADS ? 1024 : scp_cdiv(most, 4 * SHARE_THREADS);
  hipLaunchKernelGGL(keep_better_kernel, dim3(blocks), dim3(SHARE_THREADS), 0, ctx->stream, c, (const unsigned long long*)overuse, r,
                     best_round);
  return SCP_OK;
}

extern "C" int scp_path_load(scp_ctx* ctx, int N, int max_path, int nodes, const int32_t* path, const scp_path_info* info,
                             int capacity, uint32_t* load, uint64_t* overuse) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, N >= 1 && max_path >= 1, "path_load: bad shape N=%d max_path=%d", N, max_path);
  SCP_REQUIRE(ctx, nodes >= 1 && nodes <= SCP_LATTICE_MAX_NODES, "path_load: nodes=%d (1 .. %d)", nodes, SCP_LATTICE_MAX_NODES);
  SCP_REQUIRE(ctx, capacity >= 1, "path_load: capacity=%d (>= 1 vehicles per node)", capacity);
  SCP_REQUIRE(ctx, path && info && load && overuse, "path_load: null pointer");
  int rc = corridor_begin(ctx);
  if (rc) return rc;
  if ((rc = path_load_enqueue(ctx, N, max_path, nodes, path, info, capacity, load, overuse, true))) return rc;
  return corridor_end(ctx);
}
