// Static obstacles on gfx950: the searches on the lattice of scp_lattice_edges, by hops (breadth first, a uint16 field) and
// by the length- and clearance-weighted cost (run to its fixed point, a uint32 field).  Per vehicle the search from its goal,
// the path from its start and the K + 1 reference points along it; per source the search and the values at every
// destination.  ONE workgroup per vehicle / per source, the field in LDS; one kernel of either kind, instantiated per metric
// (HopField / CostField of scp_lattice_device.h, where the sweep lives).  The rules are stated in include/scp_hip.h
// ("reference paths by a lattice search", "lattice distances", "weighted search"); tests/reference_path_ref.py,
// tests/assign_paths_ref.py and tests/weighted_path_ref.py restate them.  Integers only, except the reference points (bit for
// bit: no contraction).
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"

#include <cmath>

namespace {

// ----------------------------------------------------------------------------------------------------
// search, path and reference points: one workgroup per vehicle
// ----------------------------------------------------------------------------------------------------
enum { CTL_STATUS = 0, CTL_START, CTL_GOAL, CTL_NODES, CTL_FLAGS /* Field::FLAG_WORDS words */ };

// CAP: the nodes the workgroup's LDS field holds (lt.nodes <= CAP: the host chooses the instantiation).  pen and path_cost
// belong to the weighted metric (pen NULL: zeros); the hop metric reads and writes neither.
template <int D, class Field, int CAP>
__global__ __launch_bounds__(1024) void lattice_paths_kernel(int K, Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                              const uint32_t* __restrict__ pen, const double* __restrict__ p0,
                                                              const double* __restrict__ pf, int max_path, double* __restrict__ ref,
                                                              int32_t* path, scp_path_info* __restrict__ info,
                                                              uint32_t* __restrict__ path_cost,
                                                              typename Field::Word* __restrict__ field_out,
                                                              unsigned long long* __restrict__ n_failed) {
  using Word = typename Field::Word;
  __shared__ Word field[CAP];
  __shared__ int ctl[CTL_FLAGS + Field::FLAG_WORDS];
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
    for (int w = 0; w < Field::FLAG_WORDS; ++w) ctl[CTL_FLAGS + w] = 0;
  }
  __syncthreads();
  const int start = ctl[CTL_START], goal = ctl[CTL_GOAL];
  const bool searching = ctl[CTL_STATUS] == 0;
  for (int node = tid; node < lt.nodes; node += T) field[node] = searching && node == goal ? (Word)0 : Field::UNREACHED;
  __syncthreads();

  // from the goal: until the start is reached or a sweep changes nothing, or -- where the metric has no stop -- to the
  // complete field, also when the start is the goal
  lattice_sweeps(lt, edges, Field::rule(field, pen, Field::STOPS_AT_START ? start : -1), ctl + CTL_FLAGS, goal,
                 searching && !(Field::STOPS_AT_START && start == goal));

  if (field_out)
    for (int node = tid; node < lt.nodes; node += T) field_out[i * lt.nodes + node] = field[node];

  // The path: one thread walks it from the start over the first neighbour in DIRECTION_ORDER that leads on, until the goal;
  // status 4 when max_path nodes did not reach it (the tail loop below overwrites what it wrote).  The field falls strictly
  // along the walk.  By hops each step lowers it by exactly one, so the walk has field[start] + 1 nodes, and every level
  // below field[start] is complete even where the search stopped at the start: the same path and the same status 4 as
  // counting field[start] + 1 against max_path beforehand.
  if (tid == 0) {
    int status = ctl[CTL_STATUS], m = 0;
    if (status == 0 && field[start] == Field::UNREACHED) status = 3;
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
        const uint32_t mask = edges[node], here = field[node];
        int next = -1;
        for (int k = 0; k < 26 && next < 0; ++k) {
          const int n = DIRECTION_ORDER.code[k];
          const int nb = node + direction_offset(lt, n);
          if ((mask >> n & 1u) && (unsigned)nb < (unsigned)lt.nodes && Field::leads_on(field, pen, node, here, nb, n)) next = nb;
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
    if (Field::HAS_PATH_COST) path_cost[i] = status == 0 ? (uint32_t)field[start] : COST_UNREACHED;
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
// values between two sets of points: one workgroup per source
// ----------------------------------------------------------------------------------------------------
enum { PCTL_SOURCE = 0, PCTL_FLAGS /* Field::FLAG_WORDS words */ };

template <int D, class Field, int CAP>
__global__ __launch_bounds__(1024) void lattice_pairs_kernel(Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                              const uint32_t* __restrict__ pen, const double* __restrict__ src,
                                                              int n_dst, const double* __restrict__ dst,
                                                              typename Field::Word* __restrict__ values,
                                                              int32_t* __restrict__ src_node, int32_t* __restrict__ dst_node,
                                                              typename Field::Word* __restrict__ field_out) {
  using Word = typename Field::Word;
  __shared__ Word field[CAP];
  __shared__ int ctl[PCTL_FLAGS + Field::FLAG_WORDS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t a = blockIdx.x;

  if (tid == 0) {  // the source's node: decided once, by one thread
    const int node = passable_node_of<D>(lt, g, edges, src + a * D);
    ctl[PCTL_SOURCE] = node;
    src_node[a] = node;
    for (int w = 0; w < Field::FLAG_WORDS; ++w) ctl[PCTL_FLAGS + w] = 0;
  }
  __syncthreads();
  const int source = ctl[PCTL_SOURCE];
  for (int node = tid; node < lt.nodes; node += T) field[node] = node == source ? (Word)0 : Field::UNREACHED;
  __syncthreads();

  // the complete field: no node stops the search
  lattice_sweeps(lt, edges, Field::rule(field, pen, -1), ctl + PCTL_FLAGS, source, source >= 0);

  if (field_out)
    for (int node = tid; node < lt.nodes; node += T) field_out[a * lt.nodes + node] = field[node];
  // every workgroup finds the destinations' nodes for itself (a cell lookup and one mask); the first one reports them
  for (int b = tid; b < n_dst; b += T) {
    const int node = passable_node_of<D>(lt, g, edges, dst + (int64_t)b * D);
    if (a == 0) dst_node[b] = node;
    values[a * n_dst + b] = source >= 0 && node >= 0 ? field[node] : Field::UNREACHED;
  }
}

// ----------------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------------
// The workgroup width of the four searches.  Measured with 256, 512 and 1024 threads for the hop paths on a 46 x 46 lattice
// (512 is fastest) and on a 32 x 32 x 32 one (1024 is); nothing in between and no other kernel has been measured, the
// boundary is a guess
int search_threads(const scp_ctx* ctx, const Lattice& lt) {
  return ctx->ref_path_threads ? ctx->ref_path_threads : lt.nodes > 8192 ? 1024 : 512;
}

// scp_reference_paths (pen, path_cost NULL) and scp_reference_paths_weighted
template <class Field>
int reference_paths(scp_ctx* ctx, const char* who, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                    const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf, int max_path, double* ref,
                    int32_t* path, scp_path_info* info, uint32_t* path_cost, typename Field::Word* field_out, uint64_t* n_failed) {
  CorridorGrid g;
  Lattice lt;
  int rc = lattice_begin(ctx, who, D, grid, stride, g, lt);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "%s: bad shape N=%d K=%d", who, N, K);
  SCP_REQUIRE(ctx, max_path >= 1 && max_path <= lt.nodes, "%s: max_path=%d (1 .. %d nodes)", who, max_path, lt.nodes);
  SCP_REQUIRE(ctx, edges && p0 && pf && ref && info && (path_cost || !Field::HAS_PATH_COST) && n_failed, "%s: null pointer", who);
  if ((rc = path_table(ctx, N, max_path, path))) return rc;
  const bool small = lt.nodes <= Field::SMALL_CAP;
  auto kernel = D == 2 ? (small ? lattice_paths_kernel<2, Field, Field::SMALL_CAP> : lattice_paths_kernel<2, Field, SCP_LATTICE_MAX_NODES>)
                       : (small ? lattice_paths_kernel<3, Field, Field::SMALL_CAP> : lattice_paths_kernel<3, Field, SCP_LATTICE_MAX_NODES>);
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_failed, 0, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(kernel, dim3(N), dim3(search_threads(ctx, lt)), 0, ctx->stream, K, lt, g, edges, pen, p0, pf, max_path, ref,
                     path, info, path_cost, field_out, (unsigned long long*)n_failed);
  return corridor_end(ctx);
}

// scp_lattice_distances (pen NULL) and scp_lattice_costs
template <class Field>
int lattice_pairs(scp_ctx* ctx, const char* who, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                  const uint32_t* pen, int n_src, const double* src, int n_dst, const double* dst, typename Field::Word* values,
                  int32_t* src_node, int32_t* dst_node, typename Field::Word* field_out) {
  CorridorGrid g;
  Lattice lt;
  int rc = lattice_begin(ctx, who, D, grid, stride, g, lt);
  if (rc) return rc;
  SCP_REQUIRE(ctx, n_src >= 1 && n_dst >= 1, "%s: bad shape n_src=%d n_dst=%d", who, n_src, n_dst);
  SCP_REQUIRE(ctx, edges && src && dst && values && src_node && dst_node, "%s: null pointer", who);
  const bool small = lt.nodes <= Field::SMALL_CAP;
  auto kernel = D == 2 ? (small ? lattice_pairs_kernel<2, Field, Field::SMALL_CAP> : lattice_pairs_kernel<2, Field, SCP_LATTICE_MAX_NODES>)
                       : (small ? lattice_pairs_kernel<3, Field, Field::SMALL_CAP> : lattice_pairs_kernel<3, Field, SCP_LATTICE_MAX_NODES>);
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(kernel, dim3(n_src), dim3(search_threads(ctx, lt)), 0, ctx->stream, lt, g, edges, pen, src, n_dst, dst,
                     values, src_node, dst_node, field_out);
  return corridor_end(ctx);
}

}  // namespace

extern "C" int scp_reference_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                   const uint32_t* edges, const double* p0, const double* pf, int max_path, double* ref,
                                   int32_t* path, scp_path_info* info, uint16_t* dist_out, uint64_t* n_failed) {
  return reference_paths<HopField>(ctx, "reference_paths", N, K, D, grid, stride, edges, nullptr, p0, pf, max_path, ref, path, info,
                                   nullptr, dist_out, n_failed);
}

extern "C" int scp_reference_paths_weighted(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                            const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf,
                                            int max_path, double* ref, int32_t* path, scp_path_info* info, uint32_t* path_cost,
                                            uint32_t* cost_out, uint64_t* n_failed) {
  return reference_paths<CostField>(ctx, "reference_paths_weighted", N, K, D, grid, stride, edges, pen, p0, pf, max_path, ref, path,
                                    info, path_cost, cost_out, n_failed);
}

extern "C" int scp_lattice_distances(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                                     int n_src, const double* src, int n_dst, const double* dst, uint16_t* hops,
                                     int32_t* src_node, int32_t* dst_node, uint16_t* dist_out) {
  return lattice_pairs<HopField>(ctx, "lattice_distances", D, grid, stride, edges, nullptr, n_src, src, n_dst, dst, hops, src_node,
                                 dst_node, dist_out);
}

extern "C" int scp_lattice_costs(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                                 const uint32_t* pen, int n_src, const double* src, int n_dst, const double* dst, uint32_t* costs,
                                 int32_t* src_node, int32_t* dst_node, uint32_t* cost_out) {
  return lattice_pairs<CostField>(ctx, "lattice_costs", D, grid, stride, edges, pen, n_src, src, n_dst, dst, costs, src_node,
                                  dst_node, cost_out);
}
