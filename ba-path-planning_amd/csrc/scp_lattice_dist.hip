// Static obstacles on gfx950: lattice distances between two sets of points.  Per source a breadth-first search over the edge
// masks of scp_lattice_edges that runs until a level changes nothing (ONE workgroup per source, dist in LDS), then the hop
// counts to every destination.  The lattice, the node of a point and the level sweep are those of scp_reference.hip
// (scp_lattice_device.h); the rule is stated in include/scp_hip.h ("lattice distances"), tests/assign_paths_ref.py restates
// it.  Integers only.
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"

namespace {

enum { DCTL_SOURCE = 0, DCTL_CHANGED /* 3 words */, DCTL_REACHED = DCTL_CHANGED + 3 /* 3 words */, DCTL_WORDS = DCTL_REACHED + 3 };

template <int D>
__global__ __launch_bounds__(1024) void lattice_distances_kernel(Lattice lt, CorridorGrid g, const uint32_t* __restrict__ edges,
                                                                  const double* __restrict__ src, int n_dst,
                                                                  const double* __restrict__ dst, uint16_t* __restrict__ hops,
                                                                  int32_t* __restrict__ src_node, int32_t* __restrict__ dst_node,
                                                                  uint16_t* __restrict__ dist_out) {
  __shared__ uint16_t dist[SCP_LATTICE_MAX_NODES];
  __shared__ int ctl[DCTL_WORDS];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t a = blockIdx.x;

  if (tid == 0) {  // the source's node: decided once, by one thread
    const int node = passable_node_of<D>(lt, g, edges, src + a * D);
    ctl[DCTL_SOURCE] = node;
    src_node[a] = node;
    for (int w = DCTL_CHANGED; w < DCTL_WORDS; ++w) ctl[w] = 0;
  }
  __syncthreads();
  const int source = ctl[DCTL_SOURCE];
  for (int node = tid; node < lt.nodes; node += T) dist[node] = node == source ? 0 : DIST_UNREACHED;
  __syncthreads();

  // the complete field: no node stops the search (the last level's barrier stands between the sweeps and the reads below)
  lattice_search(lt, edges, dist, ctl + DCTL_CHANGED, ctl + DCTL_REACHED, source, -1, source >= 0);

  if (dist_out)
    for (int node = tid; node < lt.nodes; node += T) dist_out[a * lt.nodes + node] = dist[node];
  // every workgroup finds the destinations' nodes for itself (a cell lookup and one mask); the first one reports them
  for (int b = tid; b < n_dst; b += T) {
    const int node = passable_node_of<D>(lt, g, edges, dst + (int64_t)b * D);
    if (a == 0) dst_node[b] = node;
    hops[a * n_dst + b] = (uint16_t)(source >= 0 && node >= 0 ? dist[node] : DIST_UNREACHED);
  }
}

}  // namespace

extern "C" int scp_lattice_distances(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int stride, const uint32_t* edges,
                                     int n_src, const double* src, int n_dst, const double* dst, uint16_t* hops,
                                     int32_t* src_node, int32_t* dst_node, uint16_t* dist_out) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  Lattice lt;
  int rc = corridor_grid(ctx, "lattice_distances", D, grid, g);
  if (rc) return rc;
  if ((rc = lattice_of(ctx, "lattice_distances", D, g, stride, lt))) return rc;
  SCP_REQUIRE(ctx, n_src >= 1 && n_dst >= 1, "lattice_distances: bad shape n_src=%d n_dst=%d", n_src, n_dst);
  SCP_REQUIRE(ctx, edges && src && dst && hops && src_node && dst_node, "lattice_distances: null pointer");
  // the widths of scp_reference_paths; here every sweep soon covers the whole lattice
  const int threads = lt.nodes > 8192 ? 1024 : 512;
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(D == 2 ? lattice_distances_kernel<2> : lattice_distances_kernel<3>, dim3(n_src), dim3(threads), 0,
                     ctx->stream, lt, g, edges, src, n_dst, dst, hops, src_node, dst_node, dist_out);
  return corridor_end(ctx);
}
