// Per-trajectory kernels of the SCP hot path on gfx950: the layout changes, kinematics (a4/a7), fixed bounds (a2) and the
// SCP relative step (a1).  Reference: src/path_planning/solvers/scp.py (line numbers cited per kernel).
#include "scp_common.h"
#include "scp_traj_device.h"

#include <cmath>

// ----------------------------------------------------------------------------------------------------
// layout changes [N][K][D] <-> [K][N*D]
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void to_time_major_kernel(int N, int K, int D, const double* __restrict__ src,
                                                             double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // destination index (coalesced writes)
  const int64_t C = (int64_t)N * D;
  if (t >= C * K) return;
  const int k = (int)(t / C);
  const int c = (int)(t % C);
  const int i = c / D, d = c % D;
  dst[t] = src[((int64_t)i * K + k) * D + d];
}

__global__ __launch_bounds__(256) void from_time_major_kernel(int N, int K, int D, const double* __restrict__ src,
                                                               double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // source index (coalesced reads)
  const int64_t C = (int64_t)N * D;
  if (t >= C * K) return;
  const int k = (int)(t / C);
  const int c = (int)(t % C);
  const int i = c / D, d = c % D;
  dst[((int64_t)i * K + k) * D + d] = src[t];
}

int scp_launch_to_time_major(scp_ctx* ctx, int N, int K, int D, const double* src, double* dst) {
  const int64_t n = (int64_t)N * K * D;
  hipLaunchKernelGGL(to_time_major_kernel, dim3(scp_cdiv(n, 256)), dim3(256), 0, ctx->stream, N, K, D, src, dst);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

int scp_launch_from_time_major(scp_ctx* ctx, int N, int K, int D, const double* src, double* dst) {
  const int64_t n = (int64_t)N * K * D;
  hipLaunchKernelGGL(from_time_major_kernel, dim3(scp_cdiv(n, 256)), dim3(256), 0, ctx->stream, N, K, D, src, dst);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

// ----------------------------------------------------------------------------------------------------
// a4 / a7 kinematics (scp.py:371-397, :559-595).  One thread per output sample; the inner sum runs in the
// reference's order with separately rounded multiply and add (no FMA) so the result is bitwise the
// reference's.
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kinematics_kernel(int N, int K, int D, double h,
                                                          const double* __restrict__ acc,
                                                          const double* __restrict__ p0,
                                                          const double* __restrict__ v0, double* __restrict__ pos,
                                                          double* __restrict__ vel, double* __restrict__ acc_copy) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N * K * D) return;
  if (acc_copy) acc_copy[t] = acc[t];  // (the solver's final launch also hands the accelerations out: no copy launch)
  const int d = (int)(t % D);
  const int k = (int)((t / D) % K);
  const int i = (int)(t / ((int64_t)D * K));
  double p, v;
  kin_point(acc + (int64_t)i * K * D + d, D, k, h, p0[i * D + d], v0[i * D + d], p, v);
  pos[t] = p;
  if (vel) vel[t] = v;
}

extern "C" int scp_kinematics(scp_ctx* ctx, int N, int K, int D, double h, const double* acc, const double* p0,
                              const double* v0, double* pos_out, double* vel_out) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, N > 0 && K > 0 && (D == 2 || D == 3), "kinematics: bad shape N=%d K=%d D=%d", N, K, D);
  SCP_REQUIRE(ctx, acc && p0 && v0 && pos_out, "kinematics: null pointer");
  const int64_t n = (int64_t)N * K * D;
  hipLaunchKernelGGL(kinematics_kernel, dim3(scp_cdiv(n, 256)), dim3(256), 0, ctx->stream, N, K, D, h, acc, p0,
                     v0, pos_out, vel_out, (double*)nullptr);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

// scp_kinematics + a copy of `acc` to acc_copy in the same launch (scp_common.h)
int scp_launch_kinematics_copy(scp_ctx* ctx, int N, int K, int D, double h, const double* acc, const double* p0,
                               const double* v0, double* pos_out, double* vel_out, double* acc_copy) {
  const int64_t n = (int64_t)N * K * D;
  hipLaunchKernelGGL(kinematics_kernel, dim3(scp_cdiv(n, 256)), dim3(256), 0, ctx->stream, N, K, D, h, acc, p0,
                     v0, pos_out, vel_out, acc_copy);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

// ----------------------------------------------------------------------------------------------------
// a2 bounds (scp.py:189-190, :194-195, :206-224, :234-257)
// ----------------------------------------------------------------------------------------------------
struct BoundParams {
  double vel_min, vel_max, acc_min, acc_max, jerk_min, jerk_max;
  double pmin[3], pmax[3];
};

__device__ inline void bound_of(const BoundParams& bp, int block, int i, int k, int d, int K, int D, double h,
                                const double* p0, const double* v0, const double* pf, const double* vf,
                                double& lo, double& hi) {
#pragma clang fp contract(off)
  const int s = i * D + d;
  if (block == 0) {  // jerk
    lo = bp.jerk_min;
    hi = bp.jerk_max;
  } else if (block == 1) {  // acc
    lo = bp.acc_min;
    hi = bp.acc_max;
  } else if (block == 2) {  // vel: row k is the state k+1
    if (k < K - 1) {
      lo = bp.vel_min - v0[s];  // scp.py:218-221
      hi = bp.vel_max - v0[s];
    } else {
      lo = hi = vf[s] - v0[s];  // scp.py:223-224
    }
  } else {  // pos
    const double hk = h * (double)(k + 1);
    const double hkv = hk * v0[s];
    const double off = p0[s] + hkv;  // scp.py:246-247
    if (k < K - 1) {
      lo = bp.pmin[d] - off;  // scp.py:251-254
      hi = bp.pmax[d] - off;
    } else {
      lo = hi = pf[s] - off;  // scp.py:256-257
    }
  }
}

// reference stacking order: [jerk (N,K-1,D) | acc (N,K,D) | vel | pos]
__global__ __launch_bounds__(256) void bounds_ref_order_kernel(BoundParams bp, int N, int K, int D, double h,
                                                                const double* p0, const double* v0,
                                                                const double* pf, const double* vf,
                                                                double* __restrict__ l, double* __restrict__ u) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nj = (int64_t)N * (K - 1) * D, na = (int64_t)N * K * D;
  if (t >= nj + 3 * na) return;
  int block, i, k, d;
  if (t < nj) {
    block = 0;
    d = (int)(t % D);
    k = (int)((t / D) % (K - 1));
    i = (int)(t / ((int64_t)D * (K - 1)));
  } else {
    const int64_t r = t - nj;
    block = 1 + (int)(r / na);
    const int64_t e = r % na;
    d = (int)(e % D);
    k = (int)((e / D) % K);
    i = (int)(e / ((int64_t)D * K));
  }
  double lo, hi;
  bound_of(bp, block, i, k, d, K, D, h, p0, v0, pf, vf, lo, hi);
  l[t] = lo;
  u[t] = hi;
}

// time-major stacked layout used by the QP: row = block offset + k, column c = i*D + d
__global__ __launch_bounds__(256) void bounds_time_major_kernel(BoundParams bp, int N, int K, int D, double h,
                                                                 const double* p0, const double* v0,
                                                                 const double* pf, const double* vf,
                                                                 double* __restrict__ l, double* __restrict__ u,
                                                                 double* __restrict__ states_out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t C = (int64_t)N * D;
  const int rows = 4 * K - 1;
  if (states_out && t < 4 * C) {  // the QP's own copy of [p0 | v0 | pf | vf] (lean persistent kernels), no copy launches
    const int which = (int)(t / C);
    const int64_t c = t - which * C;
    states_out[t] = which == 0 ? p0[c] : (which == 1 ? v0[c] : (which == 2 ? pf[c] : vf[c]));
  }
  if (t >= C * rows) return;
  const int row = (int)(t / C);
  const int c = (int)(t % C);
  int block, k;
  if (row < K - 1) {
    block = 0;
    k = row;
  } else {
    block = 1 + (row - (K - 1)) / K;
    k = (row - (K - 1)) % K;
  }
  double lo, hi;
  bound_of(bp, block, c / D, k, c % D, K, D, h, p0, v0, pf, vf, lo, hi);
  l[t] = lo;
  u[t] = hi;
}

static void fill_bound_params(BoundParams& bp, int D, const double* limits, const double* space) {
  bp.vel_min = limits[0];
  bp.vel_max = limits[1];
  bp.acc_min = limits[2];
  bp.acc_max = limits[3];
  bp.jerk_min = limits[4];
  bp.jerk_max = limits[5];
  for (int d = 0; d < 3; ++d) {
    bp.pmin[d] = d < D ? space[d] : 0.0;
    bp.pmax[d] = d < D ? space[D + d] : 0.0;
  }
}

extern "C" int scp_fixed_bounds(scp_ctx* ctx, int N, int K, int D, double h, const double* limits,
                                const double* space, const double* p0, const double* v0, const double* pf,
                                const double* vf, double* l_out, double* u_out) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, N > 0 && K > 1 && (D == 2 || D == 3), "fixed_bounds: bad shape N=%d K=%d D=%d", N, K, D);
  SCP_REQUIRE(ctx, limits && space && p0 && v0 && pf && vf && l_out && u_out, "fixed_bounds: null pointer");
  BoundParams bp;
  fill_bound_params(bp, D, limits, space);
  const int64_t m = (int64_t)N * D * (4 * K - 1);
  hipLaunchKernelGGL(bounds_ref_order_kernel, dim3(scp_cdiv(m, 256)), dim3(256), 0, ctx->stream, bp, N, K, D, h,
                     p0, v0, pf, vf, l_out, u_out);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

int scp_launch_bounds_time_major(scp_ctx* ctx, int N, int K, int D, double h, const double* limits,
                                 const double* space, const double* p0, const double* v0, const double* pf,
                                 const double* vf, double* l_tm, double* u_tm, double* states_out) {
  BoundParams bp;
  fill_bound_params(bp, D, limits, space);
  const int64_t m = (int64_t)N * D * (4 * K - 1);  // (4K - 1 >= 4 rows: the grid covers the 4 N D states too)
  hipLaunchKernelGGL(bounds_time_major_kernel, dim3(scp_cdiv(m, 256)), dim3(256), 0, ctx->stream, bp, N, K, D, h,
                     p0, v0, pf, vf, l_tm, u_tm, states_out);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

// ----------------------------------------------------------------------------------------------------
// a1: relative step (scp.py:157-159)
// ----------------------------------------------------------------------------------------------------
// partial[2 b], partial[2 b + 1] = block b's sums; the partials live in mapped host memory and the LAST block to finish
// (a ticket counter in device memory, at most 32 tickets) raises the completion word, so the host needs neither a copy
// launch nor a stream drain to read them.  copy_out (or NULL): a[] is also handed out there, as kinematics_kernel hands out
// its accelerations -- the loop visits every element anyway, and the step's result needs no copy launch of its own.
__global__ __launch_bounds__(256) void rel_step_partial_kernel(int64_t n, const double* __restrict__ a,
                                                                const double* __restrict__ b,
                                                                double* __restrict__ copy_out,
                                                                double* __restrict__ partial,
                                                                unsigned* __restrict__ ticket,
                                                                unsigned long long* __restrict__ done,
                                                                unsigned long long seq) {
  __shared__ double s0[4], s1[4];
  double d2 = 0.0, b2 = 0.0;
  // (four elements' loads in flight before the first is used; the sums take them in the order of the plain loop)
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; t + 3 * stride < n; t += 4 * stride) {
    double av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = a[t + u * stride];
      bv[u] = b[t + u * stride];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (copy_out) copy_out[t + u * stride] = av[u];
      rel_accum(av[u], bv[u], d2, b2);
    }
  }
  for (; t < n; t += stride) {
    const double at = a[t];
    if (copy_out) copy_out[t] = at;
    rel_accum(at, b[t], d2, b2);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d2 += __shfl_xor(d2, o);
    b2 += __shfl_xor(b2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s0[threadIdx.x >> 6] = d2;
    s1[threadIdx.x >> 6] = b2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store((unsigned long long*)&partial[2 * blockIdx.x],
                       (unsigned long long)__double_as_longlong((s0[0] + s0[1]) + (s0[2] + s0[3])), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((unsigned long long*)&partial[2 * blockIdx.x + 1],
                       (unsigned long long)__double_as_longlong((s1[0] + s1[1]) + (s1[2] + s1[3])), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
      *ticket = 0u;  // (the next launch on this stream starts after this kernel has ended)
      __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// scp_rel_step + a copy of a_new to copy_out (or NULL: none) in the same launch (scp_common.h).  The copy is stream-ordered
// like any kernel's output; the host's wait below returns once every workgroup has drawn its ticket.
int scp_launch_rel_step_copy(scp_ctx* ctx, int64_t n, const double* a_new, const double* a_prev, double* out, double* copy_out) {
  const int blocks = rel_step_blocks(n);
  // the (at most 64) partial sums go straight to the mapped host scratch: no copy launch
  const unsigned long long seq = ++ctx->rel_seq;
  hipLaunchKernelGGL(rel_step_partial_kernel, dim3(blocks), dim3(256), 0, ctx->stream, n, a_new, a_prev, copy_out,
                     ctx->h_scratch_dev, (unsigned*)(ctx->d_scratch + 64), (unsigned long long*)(ctx->h_scratch_dev + 64), seq);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  {
    volatile unsigned long long* flag = (volatile unsigned long long*)(ctx->h_scratch + 64);
    if (!scp_wait_host_word(flag, seq, 30)) SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // a fault surfaces here
    if (*flag != seq) return scp_fail(ctx, SCP_ERR_HIP, "rel_step: completion word not written");
  }
  double d2 = 0.0, b2 = 0.0;
  for (int b = 0; b < blocks; ++b) {
    d2 += ctx->h_scratch[2 * b];
    b2 += ctx->h_scratch[2 * b + 1];
  }
  out[0] = std::sqrt(d2);
  out[1] = std::sqrt(b2);
  out[2] = out[0] / out[1];
  return SCP_OK;
}

extern "C" int scp_rel_step(scp_ctx* ctx, int64_t n, const double* a_new, const double* a_prev, double* out) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_REQUIRE(ctx, n > 0 && a_new && a_prev && out, "rel_step: bad arguments");
  return scp_launch_rel_step_copy(ctx, n, a_new, a_prev, out, nullptr);
}
