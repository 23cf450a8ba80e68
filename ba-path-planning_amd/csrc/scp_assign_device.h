// What the two auctions share (scp_assign.hip: one workgroup per scenario; scp_assign_wide.hip: one scenario on the whole
// chip): ONE definition of the quantised cost, of the wave sum of the final costs and of the mapped host word both raise on
// unusable input, so that both produce the same bits.
#pragma once
#include "scp_common.h"

#include <cmath>

namespace {

// c_ij of the rule: floor(ldexp(d2, s)) with d2 summed in coordinate order, every product rounded
__device__ inline long long asg_cost(const double* __restrict__ a, const double* __restrict__ g, int D, int sh) {
#pragma clang fp contract(off)
  const double dx = a[0] - g[0], dy = a[1] - g[1];
  double d2 = dx * dx + dy * dy;
  if (D == 3) {
    const double dz = a[2] - g[2];
    d2 = d2 + dz * dz;
  }
  return (long long)ldexp(d2, sh);  // (non-negative and below 2^31: the conversion truncates = floor)
}

__device__ inline long long asg_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the mapped host words the kernels raise on unusable input (shared with the generator's sweep flag: calls do not overlap).
// Word 0: "a coordinate / an index is unusable"; word 1: "every scenario of this call is done" (scp_assign_goals_wide).
inline int asg_host_flag(scp_ctx* ctx) {
  if (!ctx->h_gen_flag) {
    SCP_HIP_CHECK(ctx, hipHostMalloc((void**)&ctx->h_gen_flag, 64, hipHostMallocMapped));
    SCP_HIP_CHECK(ctx, hipHostGetDevicePointer((void**)&ctx->d_gen_flag, ctx->h_gen_flag, 0));
  }
  return SCP_OK;
}

}  // namespace
