// Static obstacles on gfx950: what the lattice searches read of a map, made once per map.  The edge masks of a lattice of
// blocks of cells (one thread per node) and the node penalties of the weighted search from the gap-1 distance field (one
// thread or one wave per node).  The rules are stated in include/scp_hip.h ("reference paths by a lattice search", "weighted
// search"); tests/reference_path_ref.py and tests/weighted_path_ref.py restate them.  Integers only.
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_lattice_device.h"
#include "scp_wave_device.h"

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

}  // namespace

extern "C" int scp_lattice_edges(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const int32_t* sat, int stride,
                                 int clearance, uint32_t* edges) {
  CorridorGrid g;
  Lattice lt;
  int rc = lattice_begin(ctx, "lattice_edges", D, grid, stride, g, lt);
  if (rc) return rc;
  SCP_REQUIRE(ctx, clearance >= 0, "lattice_edges: clearance=%d (>= 0 cells)", clearance);
  SCP_REQUIRE(ctx, sat && edges, "lattice_edges: null pointer");
  clearance = clipped_clearance(D, g, clearance);
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(D == 2 ? lattice_edges_kernel<2> : lattice_edges_kernel<3>, dim3(scp_cdiv(lt.nodes, 256)), dim3(256), 0,
                     ctx->stream, lt, g, sat, clearance, edges);
  return corridor_end(ctx);
}

extern "C" int scp_lattice_penalties(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const uint32_t* field, int stride,
                                     int prefer, int weight, uint32_t* pen) {
  CorridorGrid g;
  Lattice lt;
  int rc = lattice_begin(ctx, "lattice_penalties", D, grid, stride, g, lt);
  if (rc) return rc;
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
