// The search lattice shared by scp_reference.hip, scp_lattice_dist.hip and scp_shorten.hip: its shape, node coordinates, the
// node of a point, the directions, the level-by-level search, block centres and the vertices of a lattice path (the rules
// are stated in include/scp_hip.h, "reference paths by a lattice search").
#pragma once
#include "scp_common.h"
#include "scp_corridor_device.h"

struct Lattice {
  int L[3];    // nodes per coordinate (L[2] = 1 in 2-D)
  int nodes;   // L[0] L[1] L[2] <= SCP_LATTICE_MAX_NODES
  int stride;  // cells per block edge
};

constexpr int LATTICE_SELF = 13;  // the direction code of the node itself
constexpr unsigned DIST_UNREACHED = 0xFFFFu;

// direction order: the codes other than 13 by |dx| + |dy| + |dz|, then by code
struct DirectionOrder {
  int code[26];
  constexpr DirectionOrder() : code{} {
    int k = 0;
    for (int len = 1; len <= 3; ++len)
      for (int n = 0; n < 27; ++n) {
        const int dx = n % 3 - 1, dy = (n / 3) % 3 - 1, dz = n / 9 - 1;
        if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz) == len) code[k++] = n;
      }
  }
};
static __constant__ DirectionOrder DIRECTION_ORDER;

// the id offset of the neighbour in direction n
__device__ inline int direction_offset(const Lattice& lt, int n) {
  const int dx = n % 3 - 1, dy = (n / 3) % 3 - 1, dz = n / 9 - 1;
  return (dz * lt.L[1] + dy) * lt.L[0] + dx;
}

// the node of a point; false: a coordinate is not inside the grid or lies beyond the lattice
template <int D>
__device__ inline bool node_of(const Lattice& lt, const CorridorGrid& g, const double* p, int& node) {
  int X[3] = {0, 0, 0};
  bool ok = true;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    int c = 0;
    if (!cell_of(g, d, p[d], c)) ok = false;
    X[d] = c / lt.stride;
    if (X[d] >= lt.L[d]) ok = false;
  }
  node = (X[2] * lt.L[1] + X[1]) * lt.L[0] + X[0];
  return ok;
}

// the node of a point if it lies on the lattice and is passable, else -1
template <int D>
__device__ inline int passable_node_of(const Lattice& lt, const CorridorGrid& g, const uint32_t* __restrict__ edges,
                                       const double* p) {
  int node = -1;
  if (!node_of<D>(lt, g, p, node)) return -1;
  return (edges[node] >> LATTICE_SELF & 1u) ? node : -1;
}

// The breadth-first search of one workgroup (every thread calls it with the same arguments), level by level from `origin`
// with dist[origin] = 0 and every other entry DIST_UNREACHED on entry, behind a barrier.  In level l a node becomes l + 1 if
// it is unreached and has a neighbour at l over a set edge bit; a concurrent store turns 0xFFFF into l + 1 and neither equals
// l, so the reads of a level need no order among themselves.  The two flags of a level live in slot l mod 3 of `changed` /
// `reached` (3 LDS words each, zero on entry): written in the sweep, read by everybody after the barrier, cleared by thread 0
// two levels later (after everybody has read them, before anybody writes them again).
// A move changes every coordinate by at most one, so a node at l + 1 lies within l + 1 of the origin per coordinate: the
// sweep of level l walks that box only (the same dist as a sweep over every node).
// The search ends after the level that changes nothing or -- the stop condition -- reaches the node `stop_at` (-1: none, the
// field is then complete).  One barrier per level, at most `nodes` levels.
__device__ __forceinline__ void lattice_search(const Lattice& lt, const uint32_t* __restrict__ edges, uint16_t* dist, int* changed_flag,
                                      int* reached_flag, int origin, int stop_at, bool go) {
  const int tid = threadIdx.x, T = blockDim.x;
  const int G[3] = {origin % lt.L[0], (origin / lt.L[0]) % lt.L[1], origin / (lt.L[0] * lt.L[1])};
  for (int level = 0; level < lt.nodes && go; ++level) {  // (go is the same in every thread: both exits are the workgroup's)
    const int slot = level % 3;
    int lo[3], w[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = G[d] - (level + 1) > 0 ? G[d] - (level + 1) : 0;
      const int hi = G[d] + (level + 1) < lt.L[d] - 1 ? G[d] + (level + 1) : lt.L[d] - 1;
      w[d] = hi - lo[d] + 1;
    }
    const int count = w[0] * w[1] * w[2];
    const bool whole = count == lt.nodes;
    bool changed = false, reached = false;
    for (int idx = tid; idx < count; idx += T) {
      const int node = whole ? idx : ((lo[2] + idx / (w[0] * w[1])) * lt.L[1] + lo[1] + (idx / w[0]) % w[1]) * lt.L[0] + lo[0] + idx % w[0];
      if (dist[node] != DIST_UNREACHED) continue;
      uint32_t m = edges[node];
      if (!(m >> LATTICE_SELF & 1u)) continue;
      m &= ~(1u << LATTICE_SELF) & 0x7FFFFFFu;
      while (m) {
        const int n = __ffs(m) - 1;
        m &= m - 1;
        const int nb = node + direction_offset(lt, n);  // (in the lattice wherever the masks belong to this lattice)
        if ((unsigned)nb < (unsigned)lt.nodes && dist[nb] == level) {
          dist[node] = (uint16_t)(level + 1);
          changed = true;
          if (node == stop_at) reached = true;
          break;
        }
      }
    }
    if (changed) changed_flag[slot] = 1;
    if (reached) reached_flag[slot] = 1;
    __syncthreads();
    go = changed_flag[slot] != 0 && reached_flag[slot] == 0;
    if (tid == 0) changed_flag[(level + 2) % 3] = reached_flag[(level + 2) % 3] = 0;
  }
}

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
