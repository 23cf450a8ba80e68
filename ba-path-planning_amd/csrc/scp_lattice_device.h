// The search lattice shared by scp_lattice_graph.hip, scp_lattice_search.hip and scp_shorten.hip: its shape, node
// coordinates, the node of a point, the directions, the sweep scaffold of the searches with its hop rule and its cost rule,
// the field description of either metric, block centres, the vertices of a lattice path and the reference points along it
// (the rules are stated in include/scp_hip.h, "reference paths by a lattice search"), and the host side every call on a
// lattice begins with.
#pragma once
#include "scp_common.h"
#include "scp_corridor_device.h"

struct Lattice {
  int L[3];    // nodes per coordinate (L[2] = 1 in 2-D)
  int nodes;   // L[0] L[1] L[2] <= SCP_LATTICE_MAX_NODES
  int stride;  // cells per block edge
};

constexpr int LATTICE_SELF = 13;  // the direction code of the node itself
constexpr uint16_t DIST_UNREACHED = 0xFFFFu;      // an entry of a hop field / of a cost field that the search has not
constexpr uint32_t COST_UNREACHED = 0xFFFFFFFFu;  // reached

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

// twice the move weight W[|dx| + |dy| + |dz|] of every direction code (W = 70, 99, 121; 0 for the node itself)
struct MoveCost {
  uint32_t twice[27];
  constexpr MoveCost() : twice{} {
    constexpr uint32_t W[4] = {0, 70, 99, 121};
    for (int n = 0; n < 27; ++n) twice[n] = 2 * W[(n % 3 != 1) + ((n / 3) % 3 != 1) + (n / 9 != 1)];
  }
};
static __constant__ MoveCost MOVE_COST;

// the penalty of a node under the map's penalties (pen NULL: zeros)
__device__ inline uint32_t node_penalty(const uint32_t* __restrict__ pen, int u) { return pen ? pen[u] : 0u; }

// The penalty vehicle i pays at a node once the other vehicles' paths count ("shared penalty" of include/scp_hip.h): the
// map's pen (NULL: zeros), plus share_weight per vehicle by which the node's load without the vehicle itself, and one for
// it, exceeds capacity; clamped to SCP_PENALTY_MAX_PRODUCT in 64 bits, before anything can wrap.  `own`: the bitmap of the
// vehicle's own path (the workgroup's LDS), bit u mod 32 of word u div 32.
struct SharedPenalty {
  const uint32_t* __restrict__ pen;
  const uint32_t* __restrict__ load;
  const uint32_t* own;
  uint32_t share_weight, capacity;
  __device__ __forceinline__ uint32_t at(int u) const {
    const uint32_t mine = own[u >> 5] >> (u & 31) & 1u, all = load[u];
    const uint64_t with_me = (uint64_t)(all > mine ? all - mine : 0u) + 1u;  // others_i[u] + 1
    const uint64_t over = with_me > capacity ? with_me - capacity : 0u;
    const uint64_t sum = (uint64_t)(pen ? pen[u] : 0u) + (uint64_t)share_weight * over;
    return sum < (uint64_t)SCP_PENALTY_MAX_PRODUCT ? (uint32_t)sum : (uint32_t)SCP_PENALTY_MAX_PRODUCT;
  }
};

__device__ inline uint32_t node_penalty(const SharedPenalty& pen, int u) { return pen.at(u); }

// The cost w of the edge between two neighbours a and b, n the direction code from one to the other, under either kind of
// penalty; pen_a = node_penalty(pen, a), which a caller that looks at several neighbours of a fetches once.
template <class Pen>
__device__ __forceinline__ uint32_t edge_cost(const Pen& pen, uint32_t pen_a, int b, int n) {
  return MOVE_COST.twice[n] + pen_a + node_penalty(pen, b);
}

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

// Status 0, 1 or 2 of a vehicle's end points (scp_reference_paths): 1 if the start lies off the lattice or is not passable,
// 2 the same for the goal, tested only if the start passed.  start / goal: the node's id wherever the point lies on the
// lattice and was tested, else -1.
template <int D>
__device__ inline int path_endpoints(const Lattice& lt, const CorridorGrid& g, const uint32_t* __restrict__ edges, const double* a0,
                                     const double* af, int& start, int& goal) {
  goal = -1;
  if (!node_of<D>(lt, g, a0, start)) {
    start = -1;
    return 1;
  }
  if (!(edges[start] >> LATTICE_SELF & 1u)) return 1;
  if (!node_of<D>(lt, g, af, goal)) {
    goal = -1;
    return 2;
  }
  return (edges[goal] >> LATTICE_SELF & 1u) ? 0 : 2;
}

// ----------------------------------------------------------------------------------------------------
// the searches: one sweep scaffold, a rule per metric
// ----------------------------------------------------------------------------------------------------
struct SweepVisit {  // what the visit of one node did
  bool changed, reached;  // its entry of the field changed / it is the rule's stop node and has just been reached
};

// The search of one workgroup (every thread calls it with the same arguments): sweeps from `origin`, whose entry of the
// rule's field is 0 and every other entry the field's UNREACHED on entry, behind a barrier.  A sweep offers every passable
// node of its box that the rule has not settled to rule.visit, with the node's edge mask less the self bit; what a visit
// reads and stores, and why the threads of a sweep need no order among themselves, is the rule's.
// The box: a move changes every coordinate by at most one, so a node reachable in k moves lies within k of the origin per
// coordinate: sweep k walks the box of k + 1 only.  If it changes nothing, the box's outer shell is unreached and nothing
// beyond it can be reached: the same field as sweeps over every node.
// The flags: sweep k's live in slot k mod 3 of `flags` (three "changed" words, then three "reached" words if the rule has a
// stop node; all zero on entry): written in the sweep, read by everybody after the barrier, cleared by thread 0 two sweeps
// later (after everybody has read them, before anybody writes them again).
// The search ends after the sweep that changes nothing or reaches the rule's stop node.  One barrier per sweep (it also
// stands between the last sweep and the caller's reads), at most `nodes` sweeps.
template <class Rule>
__device__ __forceinline__ void lattice_sweeps(const Lattice& lt, const uint32_t* __restrict__ edges, const Rule& rule, int* flags,
                                               int origin, bool go) {
  const int tid = threadIdx.x, T = blockDim.x;
  int* changed_flag = flags;
  int* reached_flag = flags + 3;  // (only where Rule::HAS_STOP)
  const int G[3] = {origin % lt.L[0], (origin / lt.L[0]) % lt.L[1], origin / (lt.L[0] * lt.L[1])};
  for (int sweep = 0; sweep < lt.nodes && go; ++sweep) {  // (go is the same in every thread: both exits are the workgroup's)
    const int slot = sweep % 3;
    int lo[3], w[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = G[d] - (sweep + 1) > 0 ? G[d] - (sweep + 1) : 0;
      const int hi = G[d] + (sweep + 1) < lt.L[d] - 1 ? G[d] + (sweep + 1) : lt.L[d] - 1;
      w[d] = hi - lo[d] + 1;
    }
    const int count = w[0] * w[1] * w[2];
    const bool whole = count == lt.nodes;
    bool changed = false, reached = false;
    for (int idx = tid; idx < count; idx += T) {
      const int node = whole ? idx : ((lo[2] + idx / (w[0] * w[1])) * lt.L[1] + lo[1] + (idx / w[0]) % w[1]) * lt.L[0] + lo[0] + idx % w[0];
      if (rule.settled(node)) continue;
      uint32_t m = edges[node];
      if (!(m >> LATTICE_SELF & 1u)) continue;
      m &= ~(1u << LATTICE_SELF) & 0x7FFFFFFu;
      const SweepVisit v = rule.visit(lt, sweep, node, m);
      if (v.changed) changed = true;
      if (Rule::HAS_STOP && v.reached) reached = true;
    }
    if (changed) changed_flag[slot] = 1;
    if (Rule::HAS_STOP && reached) reached_flag[slot] = 1;
    __syncthreads();
    go = changed_flag[slot] != 0 && !(Rule::HAS_STOP && reached_flag[slot] != 0);
    if (tid == 0) {
      changed_flag[(sweep + 2) % 3] = 0;
      if (Rule::HAS_STOP) reached_flag[(sweep + 2) % 3] = 0;
    }
  }
}

// The hop rule: breadth first, sweep l is level l.  A node becomes l + 1 if it is unreached and has a neighbour at l over a
// set edge bit; a concurrent store turns 0xFFFF into l + 1 and neither equals l, so the reads of a level need no order among
// themselves.  A reached node is settled.  `stop_at`: the node whose reaching ends the search (-1: none, the field is then
// complete).
struct HopRule {
  static constexpr bool HAS_STOP = true;
  uint16_t* dist;
  int stop_at;
  __device__ __forceinline__ bool settled(int node) const { return dist[node] != DIST_UNREACHED; }
  __device__ __forceinline__ SweepVisit visit(const Lattice& lt, int level, int node, uint32_t m) const {
    while (m) {
      const int n = __ffs(m) - 1;
      m &= m - 1;
      const int nb = node + direction_offset(lt, n);  // (in the lattice wherever the masks belong to this lattice)
      if ((unsigned)nb < (unsigned)lt.nodes && dist[nb] == level) {
        dist[node] = (uint16_t)(level + 1);
        return {true, node == stop_at};
      }
    }
    return {false, false};
  }
};

// The cost rule: the weighted search, run to its fixed point (no stop node, no node is ever settled).  Pull form: a thread
// owns the nodes it writes; a node reads its neighbours over its set edge bits and stores min(own, cost[nb] + w), w =
// edge_cost.  No two threads write one word and a 32-bit LDS read does not tear, so a racing read sees an older or a newer
// upper bound: every stored value is the cost of a real walk (a simple one: a walk back through the node costs more than the
// node holds), values only fall, and a sweep that changes nothing has read final values everywhere -- the fixed point, which
// is the shortest-cost field whatever the schedule.  With weight * prefer <= 32768 an edge costs at most 65778 and a simple
// path at most 32767 of them, so no sum (a candidate included) wraps.  Sweep k leaves every node at least as good as k + 1
// synchronous Bellman-Ford rounds.
template <class Pen>
struct CostRuleOf {
  static constexpr bool HAS_STOP = false;
  uint32_t* cost;
  Pen pen;  // what edge_cost reads: the map's penalties (const uint32_t*, NULL: zeros) or one vehicle's SharedPenalty
  __device__ __forceinline__ bool settled(int) const { return false; }
  __device__ __forceinline__ SweepVisit visit(const Lattice& lt, int, int node, uint32_t m) const {
    const uint32_t own = cost[node], pen_node = node_penalty(pen, node);  // (the node's own term: once, not per neighbour)
    uint32_t best = own;
    while (m) {
      const int n = __ffs(m) - 1;
      m &= m - 1;
      const int nb = node + direction_offset(lt, n);  // (in the lattice wherever the masks belong to this lattice)
      if ((unsigned)nb >= (unsigned)lt.nodes) continue;
      const uint32_t c = cost[nb];
      if (c == COST_UNREACHED) continue;
      const uint32_t via = c + edge_cost(pen, pen_node, nb, n);
      best = via < best ? via : best;
    }
    if (best < own) {
      cost[node] = best;
      return {true, false};
    }
    return {false, false};
  }
};
using CostRule = CostRuleOf<const uint32_t*>;

// What the kernels of scp_lattice_search.hip know of a metric: the field's word, its UNREACHED, the rule of its search, the
// flag words that rule needs, whether a path search stops once it reaches the start and has a cost to report, for the walk
// from the start to the goal whether the neighbour nb in direction n leads on from a node that holds `here` and pays pen_node
// = own_penalty (fetched once per node of the walk), and SMALL_CAP:
// a lattice of at most so many nodes runs an instantiation whose LDS field holds just these (the cost field: 32 KiB and
// several workgroups per CU instead of the full 128 KiB and one; the hop field is 64 KiB whatever the lattice).
// Args is what the path kernel is launched with for the metric and Pen what its rule and its walk read penalties through,
// made by penalty() from the Args and the workgroup's bitmap of its own path.  REROUTES: the kernel improves a path set in
// place (the rules "re-routing" and "groups" of include/scp_hip.h) -- workgroup b is vehicle(b), a vehicle without a path on
// entry is skipped, the walk goes to walk_row() and replaces the path row only once it has reached the goal, and a vehicle
// that keeps its path counts in kept().  The two plain metrics route every vehicle b afresh, straight into its row.
struct PlainRoutes {
  using Args = const uint32_t*;  // pen (the hop metric reads none)
  using Pen = const uint32_t*;
  static constexpr bool REROUTES = false;
  __device__ static Pen penalty(Args pen, const uint32_t*) { return pen; }
  __device__ static int64_t vehicle(Args, int b) { return b; }
  __device__ static int32_t* walk_row(Args, int, int, int32_t* my_path) { return my_path; }
  __device__ static void kept(Args) {}
};

struct HopField : PlainRoutes {
  using Word = uint16_t;
  using Rule = HopRule;
  static constexpr Word UNREACHED = DIST_UNREACHED;
  static constexpr int FLAG_WORDS = 6, SMALL_CAP = SCP_LATTICE_MAX_NODES;
  static constexpr bool STOPS_AT_START = true, HAS_PATH_COST = false;
  __device__ static Rule rule(Word* field, const uint32_t*, int stop_at) { return {field, stop_at}; }
  __device__ static uint32_t own_penalty(const uint32_t*, int) { return 0u; }
  __device__ static bool leads_on(const Word* field, const uint32_t*, uint32_t, unsigned here, int nb, int) {
    return field[nb] == here - 1u;
  }
};

struct CostField : PlainRoutes {
  using Word = uint32_t;
  using Rule = CostRule;
  static constexpr Word UNREACHED = COST_UNREACHED;
  static constexpr int FLAG_WORDS = 3, SMALL_CAP = 8192;
  static constexpr bool STOPS_AT_START = false, HAS_PATH_COST = true;
  __device__ static Rule rule(Word* field, const uint32_t* pen, int) { return {field, pen}; }
  __device__ static uint32_t own_penalty(const uint32_t* pen, int node) { return node_penalty(pen, node); }
  __device__ static bool leads_on(const Word* field, const uint32_t* pen, uint32_t pen_node, uint32_t here, int nb, int n) {
    return field[nb] != UNREACHED && field[nb] + edge_cost(pen, pen_node, nb, n) == here;
  }
};

// the cost field under one vehicle's shared penalty (scp_reference_paths_shared): the CostField's sizes, a bitmap of CAP / 32
// words beside it
struct SharedField {
  using Word = uint32_t;
  using Pen = SharedPenalty;
  using Rule = CostRuleOf<SharedPenalty>;
  struct Args {
    const uint32_t* pen;   // [nodes] or NULL
    const uint32_t* load;  // [nodes]: scp_path_load of the set on entry
    uint32_t share_weight, capacity;
    int groups, group;
    int32_t* walk_rows;          // [workgroups][max_path]: where a walk goes until it has reached the goal
    unsigned long long* n_kept;  // vehicles whose walk did not
  };
  static constexpr Word UNREACHED = COST_UNREACHED;
  static constexpr int FLAG_WORDS = 3, SMALL_CAP = 8192;
  static constexpr bool STOPS_AT_START = false, HAS_PATH_COST = true, REROUTES = true;
  __device__ static Pen penalty(const Args& a, const uint32_t* own) { return {a.pen, a.load, own, a.share_weight, a.capacity}; }
  __device__ static int64_t vehicle(const Args& a, int b) { return a.group + (int64_t)b * a.groups; }
  __device__ static int32_t* walk_row(const Args& a, int b, int max_path, int32_t*) { return a.walk_rows + (int64_t)b * max_path; }
  __device__ static void kept(const Args& a) { atomicAdd(a.n_kept, 1ull); }
  __device__ static Rule rule(Word* field, const Pen& pen, int) { return {field, pen}; }
  __device__ static uint32_t own_penalty(const Pen& pen, int node) { return node_penalty(pen, node); }
  __device__ static bool leads_on(const Word* field, const Pen& pen, uint32_t pen_node, uint32_t here, int nb, int n) {
    return field[nb] != UNREACHED && field[nb] + edge_cost(pen, pen_node, nb, n) == here;
  }
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

// The K + 1 reference points of vehicle i along p0, the centres of its path's m nodes, pf (the rule "reference points" of
// include/scp_hip.h), written side by side by the workgroup's threads.
template <int D>
__device__ __forceinline__ void write_reference_points(const Lattice& lt, const CorridorGrid& g, int K, const int32_t* my_path, int m,
                                                       const double* a0, const double* af, double* ref_i) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t E = (int64_t)m + 1;
  for (int j = tid; j <= K; j += T) {
    const int64_t q = (int64_t)j * E / K, r = (int64_t)j * E % K;
    double* out = ref_i + (int64_t)j * D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double v0 = reference_vertex(lt, g, my_path, m, a0, af, (int)q, d);
      if (q == E) {
        out[d] = v0;
      } else {
        const double v1 = reference_vertex(lt, g, my_path, m, a0, af, (int)q + 1, d);
        const double w = (double)r / (double)K;
        const double step = w * (v1 - v0);
        out[d] = v0 + step;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------------
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

// what every call on a lattice begins with: the ctx, the grid, the lattice (who: the call's name in messages)
inline int lattice_begin(scp_ctx* ctx, const char* who, int D, const scp_occupancy_grid* grid, int stride, CorridorGrid& g,
                         Lattice& lt) {
  if (!ctx) return SCP_ERR_INVALID;
  const int rc = corridor_grid(ctx, who, D, grid, g);
  return rc ? rc : lattice_of(ctx, who, D, g, stride, lt);
}

// a clearance beyond the widest dimension clipped to it (the grown ranges are clipped to the grid: the same answers, no
// overflow)
inline int clipped_clearance(int D, const CorridorGrid& g, int clearance) {
  int widest = 1;
  for (int d = 0; d < D; ++d) widest = g.dims[d] > widest ? g.dims[d] : widest;
  return clearance > widest ? widest : clearance;
}

// ---- shared paths: what scp_path_share.hip launches for the driver in scp_lattice_search.hip (enqueue only: the caller has
// checked the arguments and holds the timing bracket) ----
struct PathSet {  // the four per-vehicle outputs of a path search: [N][K+1][D], [N][max_path], [N], [N]
  double* ref;
  int32_t* path;
  scp_path_info* info;
  uint32_t* path_cost;
};
// load and *overuse of a set (written, not accumulated; `clear_overuse` false: the word is zero already)
int path_load_enqueue(scp_ctx* ctx, int N, int max_path, int nodes, const int32_t* path, const scp_path_info* info, int capacity,
                      uint32_t* load, uint64_t* overuse, bool clear_overuse);
// round r of a negotiation is over: `cur` replaces `best` iff r == 0 or overuse[r] is smaller than every earlier entry,
// decided on the device; *best_round = the earliest smallest of overuse[0 .. r]
int keep_better_enqueue(scp_ctx* ctx, int N, int K, int D, int max_path, const PathSet& cur, const PathSet& best,
                        const uint64_t* overuse, int r, int32_t* best_round);

// An N x max_path int32 table a kernel keeps for itself where the caller wants none of it (`table` NULL): the workspace of
// the continuous-time passes.
inline int path_table(scp_ctx* ctx, int N, int max_path, int32_t*& table) {
  if (table) return SCP_OK;
  const int rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)N * max_path * sizeof(int32_t));
  if (rc) return rc;
  table = (int32_t*)ctx->sep_ws;
  return SCP_OK;
}
