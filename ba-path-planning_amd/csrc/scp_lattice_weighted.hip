// Static obstacles on gfx950: the length- and clearance-weighted search on the lattice of scp_lattice_edges.  Node penalties
// from the gap-1 distance field (one thread or one wave per node), and per vehicle / per source the cost field of a weighted
// single-source search run to its fixed point (ONE workgroup each, the field in LDS as uint32), then the path and its
// reference points / the costs to every destination.  Lattice, node of a point, relaxation sweep and point writing are those
// of scp_lattice_device.h; the rules are stated in include/scp_hip.h ("weighted search"), tests/weighted_path_ref.py restates
// them.  Integers only, except the reference points (bit for bit: no contraction).
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"
#include "scp_wave_device.h"

#include <cmath>

namespace {

// ----------------------------------------------------------------------------------------------------
// node penalties: the minimum of the field over a node's block, its integer square root, the penalty
// ----------------------------------------------------------------------------------------------------
// the largest t with t^2 <= v: the rounded square root, then corrected in integers
__device__ inline uint32_t floor_sqrt(uint32_t v) {
  uint64_t t = (uint64_t)sqrt((double)v);
  while (t * t > (uint64_t)v) --t;
  while ((t + 1) * (t + 1) <= (uint64_t)v) ++t;
  return (uint32_t)t;
}

// WAVE: one wave per node (its lanes share the block's cells), else one thread per node
template <int D, bool WAVE>
__global__ __launch_bounds__(256) void lattice_penalties_kernel(Lattice lt, CorridorGrid g, const uint32_t* __restrict__ field,
                                                                 uint32_t prefer, uint32_t weight, uint32_t* __restrict__ pen) {
  const int node = WAVE ? blockIdx.x * 4 + threadIdx.x / 64 : blockIdx.x * 256 + threadIdx.x;
  if (node >= lt.nodes) return;  // (a whole wave at once in the wave form)
  const int s = lt.stride;
  const int X[3] = {node % lt.L[0] * s, (node / lt.L[0]) % lt.L[1] * s, D == 3 ? node / (lt.L[0] * lt.L[1]) * s : 0};
  const int cells = D == 3 ? s * s * s : s * s;  // (a block lies in the grid: at most 2^24 cells)
  uint32_t least = 0xFFFFFFFFu;
  for (int c = WAVE ? threadIdx.x % 64 : 0; c < cells; c += WAVE ? 64 : 1) {
    const int x = X[0] + c % s, y = X[1] + (c / s) % s, z = X[2] + c / (s * s);
    const uint32_t v = field[((int64_t)z * g.dims[1] + y) * g.dims[0] + x];
    least = v < least ? v : least;
  }
  if (WAVE) {
    least = (uint32_t)wave_min_u64(least);  // (in lane 63)
    if (threadIdx.x % 64 != 63) return;
  }
  const uint32_t rho = floor_sqrt(least);
  pen[node] = weight * (prefer - (rho < prefer ? rho : prefer));
}

// ----------------------------------------------------------------------------------------------------
// search, path and reference points: one workgroup per vehicle
// ----------------------------------------------------------------------------------------------------
enum { CTL_STATUS = 0, CTL_START, CTL_GOAL, CTL_NODES, CTL_CHANGED /* 3 words */, CTL_WORDS = CTL_CHANGED + 3 };

// CAP: the nodes the workgroup's LDS field holds (lt.nodes <= CAP: the host chooses the instantiation)
template <int D, int CAP>
__global__ __launch_bounds__(1024) void weighted_paths_kernel(int K, Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                               const uint32_t* __restrict__ pen, const double* __restrict__ p0,
                                                               const double* __restrict__ pf, int max_path, double* __restrict__ ref,
                                                               int32_t* path, scp_path_info* __restrict__ info,
                                                               uint32_t* __restrict__ path_cost, uint32_t* __restrict__ cost_out,
                                                               unsigned long long* __restrict__ n_failed) {
  __shared__ uint32_t cost[CAP];
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
  for (int node = tid; node < lt.nodes; node += T) cost[node] = searching && node == goal ? 0u : COST_UNREACHED;
  __syncthreads();

  // from the goal to the fixed point: the complete field, also when the start is the goal (the last sweep's barrier stands
  // between the sweeps and the reads below)
  lattice_relax(lt, edges, pen, cost, ctl + CTL_CHANGED, goal, searching);

  if (cost_out)
    for (int node = tid; node < lt.nodes; node += T) cost_out[i * lt.nodes + node] = cost[node];

  // the path: one thread walks it, costs fall strictly along it
  if (tid == 0) {
    int status = ctl[CTL_STATUS], m = 0;
    if (status == 0 && cost[start] == COST_UNREACHED) status = 3;
    if (status == 0) {
      int node = start;
      for (;;) {
        if (m == max_path) {  // the goal has not been reached after max_path nodes
          status = 4;
          m = 0;
          break;
        }
        my_path[m++] = node;
        if (node == goal) break;
        const uint32_t mask = edges[node], here = cost[node];
        int next = -1;
        for (int k = 0; k < 26 && next < 0; ++k) {
          const int n = DIRECTION_ORDER.code[k];
          const int nb = node + direction_offset(lt, n);
          if ((mask >> n & 1u) && (unsigned)nb < (unsigned)lt.nodes && cost[nb] != COST_UNREACHED &&
              cost[nb] + edge_cost(pen, node, nb, n) == here)
            next = nb;
        }
        if (next < 0) {  // (cannot happen: a reached node other than the goal has such a neighbour)
          status = 3;
          m = 0;
          break;
        }
        node = next;
      }
    }
    ctl[CTL_STATUS] = status;
    ctl[CTL_NODES] = m;
    scp_path_info r;
    r.status = status;
    r.n_nodes = m;
    r.start_node = start;
    r.goal_node = goal;
    info[i] = r;
    path_cost[i] = status == 0 ? cost[start] : COST_UNREACHED;
    if (status != 0) atomicAdd(n_failed, 1ull);
  }
  __syncthreads();  // (the last barrier: nobody has returned before it)
  const int m = ctl[CTL_NODES];
  for (int t = m + tid; t < max_path; t += T) my_path[t] = -1;
  if (ctl[CTL_STATUS] != 0) return;

  // the reference points, side by side
  write_reference_points<D>(lt, g, K, my_path, m, a0, af, ref + i * (K + 1) * D);
}

// ----------------------------------------------------------------------------------------------------
// costs between two sets of points: one workgroup per source
// ----------------------------------------------------------------------------------------------------
enum { CCTL_SOURCE = 0, CCTL_CHANGED /* 3 words */, CCTL_WORDS = CCTL_CHANGED + 3 };

template <int D, int CAP>
__global__ __launch_bounds__(1024) void lattice_costs_kernel(Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                              const uint32_t* __restrict__ pen, const double* __restrict__ src,
                                                              int n_dst, const double* __restrict__ dst, uint32_t* __restrict__ costs,
                                                              int32_t* __restrict__ src_node, int32_t* __restrict__ dst_node,
                                                              uint32_t* __restrict__ cost_out) {
  __shared__ uint32_t cost[CAP];
  __shared__ int ctl[CCTL_WORDS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t a = blockIdx.x;

  if (tid == 0) {  // the source's node: decided once, by one thread
    const int node = passable_node_of<D>(lt, g, edges, src + a * D);
    ctl[CCTL_SOURCE] = node;
    src_node[a] = node;
    for (int w = CCTL_CHANGED; w < CCTL_WORDS; ++w) ctl[w] = 0;
  }
  __syncthreads();
  const int source = ctl[CCTL_SOURCE];
  for (int node = tid; node < lt.nodes; node += T) cost[node] = node == source ? 0u : COST_UNREACHED;
  __syncthreads();

  lattice_relax(lt, edges, pen, cost, ctl + CCTL_CHANGED, source, source >= 0);

  if (cost_out)
    for (int node = tid; node < lt.nodes; node += T) cost_out[a * lt.nodes + node] = cost[node];
  // every workgroup finds the destinations' nodes for itself (a cell lookup and one mask); the first one reports them
  for (int b = tid; b < n_dst; b += T) {
    const int node = passable_node_of<D>(lt, g, edges, dst + (int64_t)b * D);
    if (a == 0) dst_node[b] = node;
    costs[a * n_dst + b] = source >= 0 && node >= 0 ? cost[node] : COST_UNREACHED;
  }
}

// Lattices of at most this many nodes run the instantiation with a 32 KiB field (several workgroups per CU), larger ones
// the one with the full 128 KiB field (one workgroup per CU)
constexpr int SMALL_FIELD_NODES = 8192;

// the workgroup width: the rule of scp_reference_paths, whose boundary is a guess there and has not been measured for these
// kernels either ("Weighted search")
int weighted_threads(const scp_ctx* ctx, const Lattice& lt) {
  return ctx->ref_path_threads ? ctx->ref_path_threads : lt.nodes > 8192 ? 1024 : 512;
}

}  // namespace

extern "C" int scp_lattice_penalties(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const uint32_t* field, int stride,
                                     int prefer, int weight, uint32_t* pen) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "lattice_penalties", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "lattice_penalties", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, prefer >= 0 && weight >= 0, "lattice_penalties: prefer=%d weight=%d (both >= 0)", prefer, weight);
  SCP_REQUIRE(ctx, (int64_t)prefer * weight <= SCP_PENALTY_MAX_PRODUCT,
              "lattice_penalties: weight * prefer = %lld exceeds %d (costs are 32-bit)", (long long)prefer * weight,
              SCP_PENALTY_MAX_PRODUCT);
  SCP_REQUIRE(ctx, field && pen, "lattice_penalties: null pointer");
  int64_t cells = 1;
  for (int d = 0; d < D; ++d) cells *= stride;
  if ((rc = corridor_begin(ctx))) return rc;
  const bool wave = cells >= 64;
  auto kernel = D == 2 ? (wave ? lattice_penalties_kernel<2, true> : lattice_penalties_kernel<2, false>)
                       : (wave ? lattice_penalties_kernel<3, true> : lattice_penalties_kernel<3, false>);
  hipLaunchKernelGGL(kernel, dim3(scp_cdiv(lt.nodes, wave ? 4 : 256)), dim3(256), 0, ctx->stream, lt, g, field, (uint32_t)prefer,
                     (uint32_t)weight, pen);
  return corridor_end(ctx);
}

extern "C" int scp_reference_paths_weighted(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                            const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf,
                                            int max_path, double* ref, int32_t* path, scp_path_info* info, uint32_t* path_cost,
                                            uint32_t* cost_out, uint64_t* n_failed) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "reference_paths_weighted", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "reference_paths_weighted", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "reference_paths_weighted: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, max_path >= 1 && max_path <= lt.nodes, "reference_paths_weighted: max_path=%d (1 .. %d nodes)", max_path,
              lt.nodes);
  SCP_REQUIRE(ctx, edges && p0 && pf && ref && info && path_cost && n_failed, "reference_paths_weighted: null pointer");
  if (!path) {  // the kernel keeps the paths somewhere: the workspace of the continuous-time passes
    rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)N * max_path * sizeof(int32_t));
    if (rc) return rc;
    path = (int32_t*)ctx->sep_ws;
  }
  const int threads = weighted_threads(ctx, lt);
  const bool small = lt.nodes <= SMALL_FIELD_NODES;
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_failed, 0, sizeof(uint64_t), ctx->stream));
  auto kernel = D == 2 ? (small ? weighted_paths_kernel<2, SMALL_FIELD_NODES> : weighted_paths_kernel<2, SCP_LATTICE_MAX_NODES>)
                       : (small ? weighted_paths_kernel<3, SMALL_FIELD_NODES> : weighted_paths_kernel<3, SCP_LATTICE_MAX_NODES>);
  hipLaunchKernelGGL(kernel, dim3(N), dim3(threads), 0, ctx->stream, K, lt, g, edges, pen, p0, pf, max_path, ref, path, info,
                     path_cost, cost_out, (unsigned long long*)n_failed);
  return corridor_end(ctx);
}

extern "C" int scp_lattice_costs(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                                 const uint32_t* pen, int n_src, const double* src, int n_dst, const double* dst, uint32_t* costs,
                                 int32_t* src_node, int32_t* dst_node, uint32_t* cost_out) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "lattice_costs", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "lattice_costs", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, n_src >= 1 && n_dst >= 1, "lattice_costs: bad shape n_src=%d n_dst=%d", n_src, n_dst);
  SCP_REQUIRE(ctx, edges && src && dst && costs && src_node && dst_node, "lattice_costs: null pointer");
  const int threads = weighted_threads(ctx, lt);
  const bool small = lt.nodes <= SMALL_FIELD_NODES;
  if ((rc = corridor_begin(ctx))) return rc;
  auto kernel = D == 2 ? (small ? lattice_costs_kernel<2, SMALL_FIELD_NODES> : lattice_costs_kernel<2, SCP_LATTICE_MAX_NODES>)
                       : (small ? lattice_costs_kernel<3, SMALL_FIELD_NODES> : lattice_costs_kernel<3, SCP_LATTICE_MAX_NODES>);
  hipLaunchKernelGGL(kernel, dim3(n_src), dim3(threads), 0, ctx->stream, lt, g, edges, pen, src, n_dst, dst, costs, src_node,
                     dst_node, cost_out);
  return corridor_end(ctx);
}
