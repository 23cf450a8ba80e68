// The search lattice shared by scp_reference.hip and scp_shorten.hip: its shape, node coordinates, block centres and the
// vertices of a lattice path (the rules are stated in include/scp_hip.h, "reference paths by a lattice search").
#pragma once
#include "scp_common.h"
#include "scp_corridor_device.h"

struct Lattice {
  int L[3];    // nodes per coordinate (L[2] = 1 in 2-D)
  int nodes;   // L[0] L[1] L[2] <= SCP_LATTICE_MAX_NODES
  int stride;  // cells per block edge
};

// coordinate d of a node
__device__ inline int lattice_coord(const Lattice& lt, int node, int d) {
  return d == 0 ? node % lt.L[0] : d == 1 ? (node / lt.L[0]) % lt.L[1] : node / (lt.L[0] * lt.L[1]);
}

// coordinate d of the centre of a node's block
__device__ inline double lattice_centre(const Lattice& lt, const CorridorGrid& g, int node, int d) {
#pragma clang fp contract(off)
  const int X = lattice_coord(lt, node, d);
  const double half = 0.5 * (double)lt.stride;
  const double mid = (double)(X * lt.stride) + half;
  const double off = g.cell * mid;
  return g.origin[d] + off;
}

// V_t of vehicle i, coordinate d: p0, the centres of the path's nodes, pf
__device__ inline double reference_vertex(const Lattice& lt, const CorridorGrid& g, const int32_t* path, int m,
                                          const double* p0, const double* pf, int t, int d) {
  if (t == 0) return p0[d];
  if (t == m + 1) return pf[d];
  return lattice_centre(lt, g, path[t - 1], d);
}

// the lattice of a grid; SCP_ERR_INVALID with a message where it is not supported
inline int lattice_of(scp_ctx* ctx, const char* who, int D, const CorridorGrid& g, int stride, Lattice& lt) {
  SCP_REQUIRE(ctx, stride >= 1, "%s: stride=%d (>= 1 cells)", who, stride);
  int64_t nodes = 1;
  for (int d = 0; d < 3; ++d) {
    lt.L[d] = d < D ? g.dims[d] / stride : 1;
    SCP_REQUIRE(ctx, lt.L[d] >= 1, "%s: stride=%d exceeds grid dimension %d (%d cells)", who, stride, d, g.dims[d]);
    nodes *= lt.L[d];
    SCP_REQUIRE(ctx, nodes <= SCP_LATTICE_MAX_NODES, "%s: the lattice has more than %d nodes: use a larger stride", who,
                SCP_LATTICE_MAX_NODES);
  }
  lt.nodes = (int)nodes;
  lt.stride = stride;
  return SCP_OK;
}
