// Arithmetic shared by the kernels of scp_corridor.hip, the lattice files (scp_lattice_device.h) and scp_obstacle_dist.hip (the rules are stated in
// include/scp_hip.h, "static obstacles").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct CorridorGrid {  // scp_occupancy_grid by value, as the kernels take it
  double origin[3];
  double cell;
  int dims[3];
};

__device__ inline int sat_at(const int32_t* __restrict__ sat, const CorridorGrid& g, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0) return 0;
  return sat[((int64_t)z * g.dims[1] + y) * g.dims[0] + x];
}

// occupied cells in the inclusive range [a, b]
template <int D>
__device__ inline int occupied_in(const int32_t* __restrict__ sat, const CorridorGrid& g, const int* a, const int* b) {
  int n = sat_at(sat, g, b[0], b[1], b[2]) - sat_at(sat, g, a[0] - 1, b[1], b[2]) - sat_at(sat, g, b[0], a[1] - 1, b[2]) +
          sat_at(sat, g, a[0] - 1, a[1] - 1, b[2]);
  if (D == 3)
    n -= sat_at(sat, g, b[0], b[1], a[2] - 1) - sat_at(sat, g, a[0] - 1, b[1], a[2] - 1) -
         sat_at(sat, g, b[0], a[1] - 1, a[2] - 1) + sat_at(sat, g, a[0] - 1, a[1] - 1, a[2] - 1);
  return n;
}

// the cell of a coordinate; false: not inside the grid (or not finite)
__device__ inline bool cell_of(const CorridorGrid& g, int d, double x, int& c) {
#pragma clang fp contract(off)
  const double f = floor((x - g.origin[d]) / g.cell);
  if (!(f >= 0.0 && f < (double)g.dims[d])) return false;  // (a NaN fails both)
  c = (int)f;
  return true;
}

// host side of every call on an occupancy grid (scp_corridor.hip): the grid's validation (who: the call's name in messages),
// the start of the timing bracket, and -- after the call's last launch -- launch errors and the end of the bracket
struct scp_ctx;
struct scp_occupancy_grid;
int corridor_grid(scp_ctx* ctx, const char* who, int D, const scp_occupancy_grid* grid, CorridorGrid& g);
int corridor_begin(scp_ctx* ctx);
int corridor_end(scp_ctx* ctx);

// the record of one segment: lo[0..3), hi[0..3), inclusive cell indices; blocked: (0, 0, 0, -1, -1, -1)
struct CorridorCells {
  int lo[3], hi[3];
};

__device__ inline CorridorCells corridor_load_cells(const int32_t* __restrict__ cells, int64_t seg) {
  CorridorCells c;
  const int32_t* r = cells + seg * 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c.lo[d] = r[d];
    c.hi[d] = r[3 + d];
  }
  return c;
}

__device__ inline bool corridor_blocked(const CorridorCells& c) { return c.hi[0] < c.lo[0]; }

// the segment box in metres: L_d = origin_d + cell * (double)lo_d, H_d = origin_d + cell * (double)(hi_d + 1)
__device__ inline void corridor_metres(const CorridorGrid& g, const CorridorCells& c, int d, double& L, double& H) {
#pragma clang fp contract(off)
  const double a = g.cell * (double)c.lo[d];
  const double b = g.cell * (double)(c.hi[d] + 1);
  L = g.origin[d] + a;
  H = g.origin[d] + b;
}

// max / min that take the first operand unless the second is strictly greater / smaller
__device__ inline double corridor_max(double a, double b) { return b > a ? b : a; }
__device__ inline double corridor_min(double a, double b) { return b < a ? b : a; }

// the extremes of one coordinate p + t v + t^2/2 a over [t0, t1]: the candidates are t0, t1 and t* = -v / a if a != 0 and
// t0 < t* < t1; the value at t is p + (t * v + ((0.5 * t) * t) * a); lo_v / hi_v by corridor_min / corridor_max in that order
__device__ inline void corridor_extremes(double p, double v, double a, double t0, double t1, double& lo_v, double& hi_v) {
#pragma clang fp contract(off)
  lo_v = p + (t0 * v + ((0.5 * t0) * t0) * a);
  hi_v = lo_v;
  const double end = p + (t1 * v + ((0.5 * t1) * t1) * a);
  lo_v = corridor_min(lo_v, end);
  hi_v = corridor_max(hi_v, end);
  if (a != 0.0) {
    const double ts = -v / a;
    if (ts > t0 && ts < t1) {
      const double mid = p + (ts * v + ((0.5 * ts) * ts) * a);
      lo_v = corridor_min(lo_v, mid);
      hi_v = corridor_max(hi_v, mid);
    }
  }
}
