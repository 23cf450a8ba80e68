// Device functions of the trajectory kernels (scp_traj.hip) that the one-launch pairwise passes of small problems
// (scp_kernels.hip) repeat inside their own launch: ONE definition of each, the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// one term of scp_rel_step's two sums (scp.py:157-159): ONE definition for rel_step_partial_kernel and for the tail of the
// small-problem violations pass, which emulates that kernel's blocks one after the other (same sums, same bits)
__device__ inline void rel_accum(double x, double y, double& d2, double& b2) {
  d2 += (x - y) * (x - y);
  b2 += y * y;
}
__host__ __device__ inline int rel_step_blocks(int64_t n) {
  const int b = (int)((n + 256 * 8 - 1) / (256 * 8));
  return b < 32 ? b : 32;
}

// position (and velocity) of one coordinate at step k from its acceleration samples a[0], a[stride], ...: ONE definition for
// the kinematics kernel and for the small-problem violations pass that derives its positions from the QP's time-major
// solution itself (pair_pass_kernel<.., SMALL>), so that both produce the same bits
__device__ inline void kin_point(const double* __restrict__ a, int64_t stride, int k, double h, double pi, double vi,
                                 double& p_out, double& v_out) {
#pragma clang fp contract(off)  // every product below is rounded before it is added, as numpy does
  double v = vi;
  const double hk = h * (double)k;
  const double hkv = hk * vi;
  double p = pi + hkv;  // p0 + (h*k)*v0   scp.py:393
  const double hh = h * h;
  constexpr int KIN_CHUNK = 32;  // loads in flight per pass; the sums stay in the reference's order
  for (int j0 = 0; j0 < k; j0 += KIN_CHUNK) {
    double av[KIN_CHUNK];
#pragma unroll
    for (int u = 0; u < KIN_CHUNK; ++u) av[u] = j0 + u < k ? a[(int64_t)(j0 + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < KIN_CHUNK; ++u) {
      if (j0 + u < k) {
        const int j = j0 + u;
        const double aj = av[u];
        const double hv = h * aj;
        v = v + hv;  // scp.py:390
        const double w = hh * ((double)(k - j) - 0.5);
        const double wa = w * aj;
        p = p + wa;  // scp.py:395
      }
    }
  }
  p_out = p;
  v_out = v;
}
