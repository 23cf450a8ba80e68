// The straight-line closest approach of the header's "Block draw" rule (include/scp_hip.h): ONE definition for the scenario
// generator (scp_scenario.hip) and the straight-line check (scp_assign.hip), so that both produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

// squared closest approach of two straight-line motions in the plane: r0 = a_i - a_j, g = g_i - g_j
// (straight_line_min_distance's arithmetic without the sqrt; x terms before y terms)
__device__ inline double gen_d2(double r0x, double r0y, double gx, double gy) {
#pragma clang fp contract(off)
  const double drx = gx - r0x, dry = gy - r0y;
  const double den = drx * drx + dry * dry;
  double s = -(r0x * drx + r0y * dry) / (den > 0.0 ? den : 1.0);
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  const double cx = r0x + s * drx, cy = r0y + s * dry;
  return cx * cx + cy * cy;
}

// the same in 3-D (z terms last): equal to gen_d2 bit for bit when both agents share a layer (their z terms are 0)
__device__ inline double gen_d2_3(double r0x, double r0y, double r0z, double gx, double gy, double gz) {
#pragma clang fp contract(off)
  const double drx = gx - r0x, dry = gy - r0y, drz = gz - r0z;
  const double den = drx * drx + dry * dry + drz * drz;
  double s = -(r0x * drx + r0y * dry + r0z * drz) / (den > 0.0 ? den : 1.0);
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  const double cx = r0x + s * drx, cy = r0y + s * dry, cz = r0z + s * drz;
  return cx * cx + cy * cy + cz * cz;
}
