// The predicates of scp_rasterize_shapes (scp_rasterize.hip), one cell against one shape; the rules are stated in
// include/scp_hip.h ("shapes into an occupancy grid") and restated in tests/rasterize_ref.py.  Every function evaluates its
// doubles operation by operation (no contraction).  Host and device: the arithmetic is plain C++, so a CPU build can run it.
#pragma once
#include <hip/hip_runtime.h>

#define RAST_FN __host__ __device__ inline

RAST_FN double rast_max(double a, double b) { return b > a ? b : a; }

// sq(g) of the gaps between the closed cell [lo, hi] and the closed box [pmin, pmax] (a point: pmin == pmax)
template <int D>
RAST_FN double rast_box_g2(const double* lo, const double* hi, const double* pmin, const double* pmax) {
#pragma clang fp contract(off)
  double total = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double g = rast_max(rast_max(lo[d] - pmax[d], pmin[d] - hi[d]), 0.0);
    total = total + g * g;
  }
  return total;
}

// f(t): sq(g) of the point a + t e against the closed cell
template <int D>
RAST_FN double rast_segment_f(const double* lo, const double* hi, const double* a, const double* e, double t) {
#pragma clang fp contract(off)
  double total = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double x = a[d] + t * e[d];
    const double g = rast_max(rast_max(lo[d] - x, x - hi[d]), 0.0);
    total = total + g * g;
  }
  return total;
}

// The CAPSULE's g2: the minimum of f over {0, 1}, the breakpoints strictly inside (0, 1) and the clamped stationary point of
// every interval between consecutive members (the interval's middle where f is constant on it).  A breakpoint that does not
// exist or lies outside enters as a second 1.0 (a member twice is a member once), so the set always has 2 + 2 D slots; they
// are sorted by an odd-even transposition network with constant indices (registers, no scratch), and an interval with
// t0 == t1 adds nothing.
template <int D>
RAST_FN double rast_segment_g2(const double* lo, const double* hi, const double* a, const double* e) {
#pragma clang fp contract(off)
  constexpr int M = 2 + 2 * D;
  double t[M];
  t[0] = 0.0;
  t[1] = 1.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    double u = 1.0, w = 1.0;
    if (e[d] != 0.0) {
      u = (lo[d] - a[d]) / e[d];
      w = (hi[d] - a[d]) / e[d];
      u = (u > 0.0 && u < 1.0) ? u : 1.0;
      w = (w > 0.0 && w < 1.0) ? w : 1.0;
    }
    t[2 + 2 * d] = u;
    t[3 + 2 * d] = w;
  }
#pragma unroll
  for (int round = 0; round < M; ++round) {
#pragma unroll
    for (int k = round & 1; k + 1 < M; k += 2) {
      const double p = t[k], q = t[k + 1];
      const bool swap = q < p;
      t[k] = swap ? q : p;
      t[k + 1] = swap ? p : q;
    }
  }
  double g2 = __builtin_huge_val();
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const double v = rast_segment_f<D>(lo, hi, a, e, t[k]);
    if (v < g2) g2 = v;
  }
#pragma unroll
  for (int k = 0; k + 1 < M; ++k) {
    const double t0 = t[k], t1 = t[k + 1];
    if (!(t0 < t1)) continue;
    const double tm = 0.5 * (t0 + t1);
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double x = a[d] + tm * e[d];
      const bool below = x < lo[d], above = x > hi[d];
      const double c = below ? a[d] - lo[d] : a[d] - hi[d];
      num = num + ((below || above) ? c * e[d] : 0.0);
      den = den + ((below || above) ? e[d] * e[d] : 0.0);
    }
    double ts = tm;  // (den == 0: f is constant on the interval, and tm carries no rounding of a breakpoint)
    if (den != 0.0) {
      ts = -num / den;
      if (ts < t0) ts = t0;
      if (ts > t1) ts = t1;
    }
    const double v = rast_segment_f<D>(lo, hi, a, e, ts);
    if (v < g2) g2 = v;
  }
  return g2;
}

// is the edge p -> q crossed by the ray from the centre (cx, cy) towards +x?
RAST_FN bool rast_crossed(double px, double py, double qx, double qy, double cx, double cy) {
#pragma clang fp contract(off)
  if ((py <= cy) == (qy <= cy)) return false;
  return cx < px + ((cy - py) * (qx - px)) / (qy - py);
}
