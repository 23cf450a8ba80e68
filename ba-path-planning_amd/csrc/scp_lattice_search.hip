// Static obstacles on gfx950: the searches on the lattice of scp_lattice_edges, by hops (breadth first, a uint16 field) and
// by the length- and clearance-weighted cost (run to its fixed point, a uint32 field).  Per vehicle the search from its goal,
// the path from its start and the K + 1 reference points along it; per source the search and the values at every
// destination.  ONE workgroup per vehicle / per source, the field in LDS; one kernel of either kind, instantiated per metric
// (HopField / CostField / SharedField of scp_lattice_device.h, where the sweep lives).  The third metric is the weighted one
// under a penalty per vehicle that counts the other vehicles' paths: it re-routes one group of a path set in place
// (scp_reference_paths_shared), and scp_negotiate_paths drives it over the rounds with the load and keep kernels of
// scp_path_share.hip.  The rules are stated in include/scp_hip.h ("reference paths by a lattice search", "lattice distances",
// "weighted search", "shared paths"); tests/reference_path_ref.py, tests/assign_paths_ref.py, tests/weighted_path_ref.py and
// tests/shared_path_ref.py restate them.  Integers only, except the reference points (bit for bit: no contraction).
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"

#include <cmath>

namespace {

// ----------------------------------------------------------------------------------------------------
// search, path and reference points: one workgroup per vehicle
// ----------------------------------------------------------------------------------------------------
enum { CTL_STATUS = 0, CTL_START, CTL_GOAL, CTL_NODES, CTL_FLAGS /* Field::FLAG_WORDS words */ };

// CAP: the nodes the workgroup's LDS field holds (lt.nodes <= CAP: the host chooses the instantiation).  args: the metric's
// (Field::Args: pen for the weighted metric, NULL: zeros; the shared metric's load, weights and group besides); path_cost
// belongs to the weighted metrics, the hop metric reads and writes neither.  n_failed is the plain metrics' (a re-routing
// changes no status).
template <int D, class Field, int CAP>
__global__ __launch_bounds__(1024) void lattice_paths_kernel(int K, Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                              typename Field::Args args, const double* __restrict__ p0,
                                                              const double* __restrict__ pf, int max_path, double* __restrict__ ref,
                                                              int32_t* path, scp_path_info* info,
                                                              uint32_t* __restrict__ path_cost,
                                                              typename Field::Word* __restrict__ field_out,
                                                              unsigned long long* __restrict__ n_failed) {
  using Word = typename Field::Word;
  __shared__ Word field[CAP];
  __shared__ uint32_t own[Field::REROUTES ? CAP / 32 : 1];  // the nodes of the vehicle's path on entry, a bit each
  __shared__ int ctl[CTL_FLAGS + Field::FLAG_WORDS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t i = Field::vehicle(args, blockIdx.x);
  const double* a0 = p0 + i * D;
  const double* af = pf + i * D;
  int32_t* my_path = path + i * max_path;
  int32_t* walk_row = Field::walk_row(args, blockIdx.x, max_path, my_path);
  const typename Field::Pen pen = Field::penalty(args, own);

  if (Field::REROUTES) {
    // a vehicle without a path is skipped, nothing of it is written (the same word in every thread: the workgroup returns);
    // the others mark their path in the bitmap before anything overwrites the row (the barrier: the one below)
    const scp_path_info was = info[i];
    if (was.status != 0) return;
    for (int w = tid; w < (lt.nodes + 31) / 32; w += T) own[w] = 0u;
    __syncthreads();
    const int m0 = was.n_nodes < max_path ? was.n_nodes : max_path;
    for (int t = tid; t < m0; t += T) {
      const int node = my_path[t];
      if ((unsigned)node < (unsigned)lt.nodes) atomicOr(&own[node >> 5], 1u << (node & 31));
    }
  }

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
        walk_row[m++] = node;
        if (node == goal) break;
        const uint32_t mask = edges[node], here = field[node], pen_node = Field::own_penalty(pen, node);
        int next = -1;
        for (int k = 0; k < 26 && next < 0; ++k) {
          const int n = DIRECTION_ORDER.code[k];
          const int nb = node + direction_offset(lt, n);
          if ((mask >> n & 1u) && (unsigned)nb < (unsigned)lt.nodes && Field::leads_on(field, pen, pen_node, here, nb, n)) next = nb;
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
    if (Field::REROUTES && status != 0) {
      Field::kept(args);  // the vehicle keeps its path row, info, reference points and cost entirely
    } else {
      scp_path_info r;
      r.status = status;
      r.n_nodes = m;
      r.start_node = start;
      r.goal_node = goal;
      info[i] = r;
      if (Field::HAS_PATH_COST) path_cost[i] = status == 0 ? (uint32_t)field[start] : COST_UNREACHED;
      if (!Field::REROUTES && status != 0) atomicAdd(n_failed, 1ull);
    }
  }
  __syncthreads();  // (the last barrier: only a skipped vehicle's workgroup has returned before it, as a whole)
  const int m = ctl[CTL_NODES];
  if (Field::REROUTES) {
    if (ctl[CTL_STATUS] != 0) return;
    for (int t = tid; t < m; t += T) my_path[t] = walk_row[t];
  }
  for (int t = m + tid; t < max_path; t += T) my_path[t] = -1;
  if (ctl[CTL_STATUS] != 0) return;

  // the reference points, side by side (from the walk's row: thread 0 wrote it before the barrier)
  write_reference_points<D>(lt, g, K, walk_row, m, a0, af, ref + i * (K + 1) * D);
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

// what the three path searches check alike (n_failed apart) and the lattice they run on
struct PathCall {
  CorridorGrid g;
  Lattice lt;
};
template <class Field>
int path_call(scp_ctx* ctx, const char* who, int N, int K, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
              const double* p0, const double* pf, int max_path, const double* ref, const scp_path_info* info,
              const uint32_t* path_cost, PathCall& c) {
  const int rc = lattice_begin(ctx, who, D, grid, stride, c.g, c.lt);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "%s: bad shape N=%d K=%d", who, N, K);
  SCP_REQUIRE(ctx, max_path >= 1 && max_path <= c.lt.nodes, "%s: max_path=%d (1 .. %d nodes)", who, max_path, c.lt.nodes);
  SCP_REQUIRE(ctx, edges && p0 && pf && ref && info && (path_cost || !Field::HAS_PATH_COST), "%s: null pointer", who);
  return SCP_OK;
}

// the one launch of a path search: `blocks` workgroups of the metric's kernel (inside the caller's timing bracket)
template <class Field>
void launch_paths(scp_ctx* ctx, int blocks, int K, int D, const PathCall& c, const uint32_t* edges, typename Field::Args args,
                  const double* p0, const double* pf, int max_path, double* ref, int32_t* path, scp_path_info* info,
                  uint32_t* path_cost, typename Field::Word* field_out, uint64_t* n_failed) {
  const bool small = c.lt.nodes <= Field::SMALL_CAP;
  auto kernel = D == 2 ? (small ? lattice_paths_kernel<2, Field, Field::SMALL_CAP> : lattice_paths_kernel<2, Field, SCP_LATTICE_MAX_NODES>)
                       : (small ? lattice_paths_kernel<3, Field, Field::SMALL_CAP> : lattice_paths_kernel<3, Field, SCP_LATTICE_MAX_NODES>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(search_threads(ctx, c.lt)), 0, ctx->stream, K, c.lt, c.g, edges, args, p0, pf,
                     max_path, ref, path, info, path_cost, field_out, (unsigned long long*)n_failed);
}

// scp_reference_paths (pen, path_cost NULL) and scp_reference_paths_weighted
template <class Field>
int reference_paths(scp_ctx* ctx, const char* who, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                    const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf, int max_path, double* ref,
                    int32_t* path, scp_path_info* info, uint32_t* path_cost, typename Field::Word* field_out, uint64_t* n_failed) {
  if (!ctx) return SCP_ERR_INVALID;
  PathCall c;
  int rc = path_call<Field>(ctx, who, N, K, D, grid, stride, edges, p0, pf, max_path, ref, info, path_cost, c);
  if (rc) return rc;
  SCP_REQUIRE(ctx, n_failed, "%s: null pointer", who);
  if ((rc = path_table(ctx, N, max_path, path))) return rc;
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_failed, 0, sizeof(uint64_t), ctx->stream));
  launch_paths<Field>(ctx, N, K, D, c, edges, pen, p0, pf, max_path, ref, path, info, path_cost, field_out, n_failed);
  return corridor_end(ctx);
}

// ----------------------------------------------------------------------------------------------------
// shared paths: one group re-routed under the others' load, and the negotiation over the rounds
// ----------------------------------------------------------------------------------------------------
int shared_checks(scp_ctx* ctx, const char* who, int N, int share_weight, int capacity, int groups) {
  SCP_REQUIRE(ctx, share_weight >= 0 && share_weight <= SCP_PENALTY_MAX_PRODUCT, "%s: share_weight=%d (0 .. %d)", who, share_weight,
              SCP_PENALTY_MAX_PRODUCT);
  SCP_REQUIRE(ctx, capacity >= 1, "%s: capacity=%d (>= 1 vehicles per node)", who, capacity);
  SCP_REQUIRE(ctx, groups >= 1 && groups <= N, "%s: groups=%d (1 .. N = %d)", who, groups, N);
  return SCP_OK;
}

inline int group_size(int N, int groups, int group) { return (N - group + groups - 1) / groups; }  // vehicles i = group + b groups < N

// the bytes of a workspace part, kept to 16 so that every part begins aligned
inline size_t part_bytes(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

int reference_paths_shared(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                           const uint32_t* pen, const double* p0, const double* pf, int max_path, double* ref, int32_t* path,
                           scp_path_info* info, uint32_t* path_cost, uint32_t* cost_out, const uint32_t* load, int share_weight,
                           int capacity, int groups, int group, uint64_t* n_kept) {
  const char* who = "reference_paths_shared";
  if (!ctx) return SCP_ERR_INVALID;
  PathCall c;
  int rc = path_call<SharedField>(ctx, who, N, K, D, grid, stride, edges, p0, pf, max_path, ref, info, path_cost, c);
  if (rc) return rc;
  SCP_REQUIRE(ctx, path && load && n_kept, "%s: null pointer (path is required: it holds the set the load was made from)", who);
  if ((rc = shared_checks(ctx, who, N, share_weight, capacity, groups))) return rc;
  SCP_REQUIRE(ctx, group >= 0 && group < groups, "%s: group=%d (0 .. groups - 1 = %d)", who, group, groups - 1);
  const int blocks = group_size(N, groups, group);
  if ((rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)blocks * max_path * sizeof(int32_t)))) return rc;
  const SharedField::Args args = {pen, load, (uint32_t)share_weight, (uint32_t)capacity, groups, group, (int32_t*)ctx->sep_ws,
                                  (unsigned long long*)n_kept};
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_kept, 0, sizeof(uint64_t), ctx->stream));
  launch_paths<SharedField>(ctx, blocks, K, D, c, edges, args, p0, pf, max_path, ref, path, info, path_cost, cost_out, nullptr);
  return corridor_end(ctx);
}

// The workspace: the current set (ref, path, info, path_cost), the load, the walks' rows of the largest group and, where the
// caller wants no path table, the best set's.  Every word is written by this call before it is read.
int negotiate_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                    const uint32_t* pen, const double* p0, const double* pf, int max_path, double* ref, int32_t* path,
                    scp_path_info* info, uint32_t* path_cost, uint64_t* n_failed, int share_weight, int capacity, int groups,
                    int rounds, uint64_t* overuse_out, int32_t* best_round, uint64_t* n_kept) {
  const char* who = "negotiate_paths";
  if (!ctx) return SCP_ERR_INVALID;
  PathCall c;
  int rc = path_call<SharedField>(ctx, who, N, K, D, grid, stride, edges, p0, pf, max_path, ref, info, path_cost, c);
  if (rc) return rc;
  SCP_REQUIRE(ctx, n_failed && overuse_out && best_round && n_kept, "%s: null pointer", who);
  if ((rc = shared_checks(ctx, who, N, share_weight, capacity, groups))) return rc;
  SCP_REQUIRE(ctx, rounds >= 0 && rounds <= SCP_NEGOTIATE_MAX_ROUNDS, "%s: rounds=%d (0 .. %d)", who, rounds, SCP_NEGOTIATE_MAX_ROUNDS);

  const size_t ref_bytes = part_bytes((size_t)N * (K + 1) * D * sizeof(double));
  const size_t path_bytes = part_bytes((size_t)N * max_path * sizeof(int32_t));
  const size_t info_bytes = part_bytes((size_t)N * sizeof(scp_path_info)), cost_bytes = part_bytes((size_t)N * sizeof(uint32_t));
  const size_t load_bytes = part_bytes((size_t)c.lt.nodes * sizeof(uint32_t));
  const size_t walk_bytes = part_bytes((size_t)group_size(N, groups, 0) * max_path * sizeof(int32_t));
  const size_t need = ref_bytes + path_bytes + info_bytes + cost_bytes + load_bytes + walk_bytes + (path ? 0 : path_bytes);
  if ((rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, need))) return rc;
  char* at = (char*)ctx->sep_ws;
  PathSet cur;
  cur.ref = (double*)at, at += ref_bytes;
  cur.path = (int32_t*)at, at += path_bytes;
  cur.info = (scp_path_info*)at, at += info_bytes;
  cur.path_cost = (uint32_t*)at, at += cost_bytes;
  uint32_t* load = (uint32_t*)at;
  at += load_bytes;
  int32_t* walk_rows = (int32_t*)at;
  at += walk_bytes;
  const PathSet best = {ref, path ? path : (int32_t*)at, info, path_cost};

  if ((rc = corridor_begin(ctx))) return rc;
  // round 0: the weighted search into the current set, whose reference points begin as the caller's
  SCP_HIP_CHECK(ctx, hipMemcpyAsync(cur.ref, ref, (size_t)N * (K + 1) * D * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_failed, 0, sizeof(uint64_t), ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_kept, 0, sizeof(uint64_t), ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemsetAsync(overuse_out, 0, (size_t)(rounds + 1) * sizeof(uint64_t), ctx->stream));
  launch_paths<CostField>(ctx, N, K, D, c, edges, pen, p0, pf, max_path, cur.ref, cur.path, cur.info, cur.path_cost, nullptr, n_failed);
  for (int r = 0;; ++r) {
    if ((rc = path_load_enqueue(ctx, N, max_path, c.lt.nodes, cur.path, cur.info, capacity, load, overuse_out + r, false))) return rc;
    if ((rc = keep_better_enqueue(ctx, N, K, D, max_path, cur, best, overuse_out, r, best_round))) return rc;
    if (r == rounds) break;
    const int group = r % groups;  // round r + 1 re-routes group r mod groups
    const SharedField::Args args = {pen, load, (uint32_t)share_weight, (uint32_t)capacity, groups, group, walk_rows,
                                    (unsigned long long*)n_kept};
    launch_paths<SharedField>(ctx, group_size(N, groups, group), K, D, c, edges, args, p0, pf, max_path, cur.ref, cur.path, cur.info,
                              cur.path_cost, nullptr, nullptr);
  }
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

extern "C" int scp_reference_paths_shared(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                          const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf,
                                          int max_path, double* ref, int32_t* path, scp_path_info* info, uint32_t* path_cost,
                                          uint32_t* cost_out, const uint32_t* load, int share_weight, int capacity, int groups,
                                          int group, uint64_t* n_kept) {
  return reference_paths_shared(ctx, N, K, D, grid, stride, edges, pen, p0, pf, max_path, ref, path, info, path_cost, cost_out, load,
                                share_weight, capacity, groups, group, n_kept);
}

extern "C" int scp_negotiate_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, int stride,
                                   const uint32_t* edges, const uint32_t* pen, const double* p0, const double* pf, int max_path,
                                   double* ref, int32_t* path, scp_path_info* info, uint32_t* path_cost, uint64_t* n_failed,
                                   int share_weight, int capacity, int groups, int rounds, uint64_t* overuse_out,
                                   int32_t* best_round, uint64_t* n_kept) {
  return negotiate_paths(ctx, N, K, D, grid, stride, edges, pen, p0, pf, max_path, ref, path, info, path_cost, n_failed, share_weight,
                         capacity, groups, rounds, overuse_out, best_round, n_kept);
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
