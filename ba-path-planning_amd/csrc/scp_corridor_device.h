// Arithmetic shared by the kernels of scp_corridor.hip (the rules are stated in include/scp_hip.h, "static obstacles").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct CorridorGrid {  // scp_occupancy_grid by value, as the kernels take it
  double origin[3];
  double cell;
  int dims[3];
};

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
