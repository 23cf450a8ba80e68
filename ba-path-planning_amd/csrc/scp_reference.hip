// Static obstacles on gfx950: reference paths by a lattice search.  The edge masks of a lattice of blocks of cells (one thread
// per node), and per vehicle a breadth-first search from its goal, the path from its start and the K + 1 reference points
// along it (ONE workgroup per vehicle, dist in LDS).  The rules are stated in include/scp_hip.h ("reference paths by a lattice
// search"); tests/reference_path_ref.py is their restatement (integers exactly, the points bit for bit: no contraction).
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"

#include <cmath>

namespace {

// ----------------------------------------------------------------------------------------------------
// edge masks: one thread per node
// ----------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void lattice_edges_kernel(Lattice lt, CorridorGrid g, const int32_t* __restrict__ sat,
                                                             int clearance, uint32_t* __restrict__ edges) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (node >= lt.nodes) return;
  const int X[3] = {node % lt.L[0], (node / lt.L[0]) % lt.L[1], node / (lt.L[0] * lt.L[1])};
  uint32_t mask = 0;
  for (int n = (D == 3 ? 0 : 9); n < (D == 3 ? 27 : 18); ++n) {
    const int dir[3] = {n % 3 - 1, (n / 3) % 3 - 1, n / 9 - 1};
    int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    bool inside = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int Y = X[d] + dir[d];
      if (Y < 0 || Y >= lt.L[d]) inside = false;
      const int lo = (Y < X[d] ? Y : X[d]) * lt.stride - clearance;
      const int hi = (Y < X[d] ? X[d] : Y) * lt.stride + (lt.stride - 1) + clearance;
      a[d] = lo < 0 ? 0 : lo;
      b[d] = hi > g.dims[d] - 1 ? g.dims[d] - 1 : hi;
    }
    if (inside && occupied_in<D>(sat, g, a, b) == 0) mask |= 1u << n;
  }
  edges[node] = mask;
}

// ----------------------------------------------------------------------------------------------------
// search, path and reference points: one workgroup per vehicle
// ----------------------------------------------------------------------------------------------------
enum { CTL_STATUS = 0, CTL_START, CTL_GOAL, CTL_NODES, CTL_CHANGED /* 3 words */, CTL_REACHED = CTL_CHANGED + 3 /* 3 words */,
       CTL_WORDS = CTL_REACHED + 3 };

template <int D>
__global__ __launch_bounds__(1024) void reference_paths_kernel(int K, Lattice lt, CorridorGrid g,
                                                                const uint32_t* __restrict__ edges,
                                                                const double* __restrict__ p0, const double* __restrict__ pf,
                                                                int max_path, double* __restrict__ ref,
                                                                int32_t* path, scp_path_info* __restrict__ info,
                                                                uint16_t* __restrict__ dist_out,
                                                                unsigned long long* __restrict__ n_failed) {
  __shared__ uint16_t dist[SCP_LATTICE_MAX_NODES];
  __shared__ int ctl[CTL_WORDS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t i = blockIdx.x;
  const double* a0 = p0 + i * D;
  const double* af = pf + i * D;
  int32_t* my_path = path + i * max_path;

  // start and goal: decided once, by one thread
  if (tid == 0) {
    int start = -1, goal = -1;
    const int status = path_endpoints<D>(lt, g, edges, a0, af, start, goal);
    ctl[CTL_STATUS] = status;
    ctl[CTL_START] = start;
    ctl[CTL_GOAL] = goal;
    ctl[CTL_NODES] = 0;
    for (int w = CTL_CHANGED; w < CTL_WORDS; ++w) ctl[w] = 0;
  }
  __syncthreads();
  const int start = ctl[CTL_START], goal = ctl[CTL_GOAL];
  const bool searching = ctl[CTL_STATUS] == 0;
  for (int node = tid; node < lt.nodes; node += T) dist[node] = searching && node == goal ? 0 : DIST_UNREACHED;
  __syncthreads();

  // level by level from the goal, until the start is reached or a level changes nothing
  lattice_search(lt, edges, dist, ctl + CTL_CHANGED, ctl + CTL_REACHED, goal, start, searching && start != goal);

  if (dist_out)
    for (int node = tid; node < lt.nodes; node += T) dist_out[i * lt.nodes + node] = dist[node];

  // the path: one thread walks it
  if (tid == 0) {
    int status = ctl[CTL_STATUS], m = 0;
    if (status == 0) {
      const unsigned ds = dist[start];
      if (ds == DIST_UNREACHED)
        status = 3;
      else if ((int)ds + 1 > max_path)
        status = 4;
      else
        m = (int)ds + 1;
    }
    int node = start;
    for (int t = 0; t < m; ++t) {
      my_path[t] = node;
      if (t + 1 == m) break;
      const uint32_t mask = edges[node];
      const unsigned want = (unsigned)dist[node] - 1u;
      int next = -1;
      for (int k = 0; k < 26 && next < 0; ++k) {
        const int n = DIRECTION_ORDER.code[k];
        const int nb = node + direction_offset(lt, n);
        if ((mask >> n & 1u) && (unsigned)nb < (unsigned)lt.nodes && dist[nb] == want) next = nb;
      }
      if (next < 0) {  // (cannot happen: a reached node other than the goal has such a neighbour)
        status = 3;
        m = 0;
        break;
      }
      node = next;
    }
    ctl[CTL_STATUS] = status;
    ctl[CTL_NODES] = m;
    scp_path_info r;
    r.status = status;
    r.n_nodes = m;
    r.start_node = start;
    r.goal_node = goal;
    info[i] = r;
    if (status != 0) atomicAdd(n_failed, 1ull);
  }
  __syncthreads();  // (the last barrier: nobody has returned before it)
  const int m = ctl[CTL_NODES];
  for (int t = m + tid; t < max_path; t += T) my_path[t] = -1;
  if (ctl[CTL_STATUS] != 0) return;

  // the reference points, side by side
  write_reference_points<D>(lt, g, K, my_path, m, a0, af, ref + i * (K + 1) * D);
}

}  // namespace

extern "C" int scp_lattice_edges(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const int32_t* sat, int stride,
                                 int clearance, uint32_t* edges) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "lattice_edges", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "lattice_edges", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, clearance >= 0, "lattice_edges: clearance=%d (>= 0 cells)", clearance);
  SCP_REQUIRE(ctx, sat && edges, "lattice_edges: null pointer");
  int widest = 1;
  for (int d = 0; d < D; ++d) widest = g.dims[d] > widest ? g.dims[d] : widest;
  if (clearance > widest) clearance = widest;  // (the grown range is clipped to the grid: the same masks, no overflow)
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(D == 2 ? lattice_edges_kernel<2> : lattice_edges_kernel<3>, dim3(scp_cdiv(lt.nodes, 256)), dim3(256), 0,
                     ctx->stream, lt, g, sat, clearance, edges);
  return corridor_end(ctx);
}

extern "C" int scp_reference_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                   const uint32_t* edges, const double* p0, const double* pf, int max_path, double* ref,
                                   int32_t* path, scp_path_info* info, uint16_t* dist_out, uint64_t* n_failed) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "reference_paths", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "reference_paths", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "reference_paths: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, max_path >= 1 && max_path <= lt.nodes, "reference_paths: max_path=%d (1 .. %d nodes)", max_path, lt.nodes);
  SCP_REQUIRE(ctx, edges && p0 && pf && ref && info && n_failed, "reference_paths: null pointer");
  if (!path) {  // the kernel keeps the paths somewhere: the workspace of the continuous-time passes
    rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)N * max_path * sizeof(int32_t));
    if (rc) return rc;
    path = (int32_t*)ctx->sep_ws;
  }
  // measured with 256, 512 and 1024 threads on a 46 x 46 lattice (512 is fastest) and on a 32 x 32 x 32 one (1024 is);
  // nothing in between has been measured, the boundary is a guess
  const int threads = ctx->ref_path_threads ? ctx->ref_path_threads : lt.nodes > 8192 ? 1024 : 512;
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_failed, 0, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(D == 2 ? reference_paths_kernel<2> : reference_paths_kernel<3>, dim3(N), dim3(threads), 0, ctx->stream, K,
                     lt, g, edges, p0, pf, max_path, ref, path, info, dist_out, (unsigned long long*)n_failed);
  return corridor_end(ctx);
}
