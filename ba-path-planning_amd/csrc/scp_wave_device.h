// Wavefront primitives on data-parallel-primitive (DPP) moves and the double-precision atomics that take a wave's result
// to global memory.  gfx950 only (64 lanes).
#pragma once
#include <hip/hip_runtime.h>

// One DPP move of a 32-bit value and of the 64-bit types built from two of them.  KEEP: lanes without a source keep their
// own value (reductions with idempotent operators); otherwise they read 0 (sums, shifts).
template <int CTRL, int ROW_MASK, bool KEEP>
__device__ inline int dpp_move(int v) {
  return __builtin_amdgcn_update_dpp(KEEP ? v : 0, v, CTRL, ROW_MASK, 0xF, !KEEP);
}
template <int CTRL, int ROW_MASK, bool KEEP>
__device__ inline unsigned long long dpp_move(unsigned long long v) {
  const unsigned int lo = (unsigned int)dpp_move<CTRL, ROW_MASK, KEEP>((int)(v & 0xFFFFFFFFu));
  const unsigned int hi = (unsigned int)dpp_move<CTRL, ROW_MASK, KEEP>((int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL, int ROW_MASK, bool KEEP>
__device__ inline double dpp_move(double v) {
  const int lo = dpp_move<CTRL, ROW_MASK, KEEP>(__double2loint(v));
  const int hi = dpp_move<CTRL, ROW_MASK, KEEP>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Wavefront reductions on DPP moves (row_shr 1, 2, 4, 8, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows
// 2, 3): result in LANE 63.  Lanes without a source keep their own value (idempotent operators only).  The
// __shfl_xor butterfly goes through the LDS crossbar and costs about ten times as much.
template <typename Op>
__device__ inline unsigned long long wave_reduce_u64(unsigned long long v, Op op) {
  v = op(v, dpp_move<0x111, 0xF, true>(v));
  v = op(v, dpp_move<0x112, 0xF, true>(v));
  v = op(v, dpp_move<0x114, 0xF, true>(v));
  v = op(v, dpp_move<0x118, 0xF, true>(v));
  v = op(v, dpp_move<0x142, 0xA, true>(v));
  v = op(v, dpp_move<0x143, 0xC, true>(v));
  return v;
}
__device__ inline double wave_min(double v) {
  return __longlong_as_double((long long)wave_reduce_u64((unsigned long long)__double_as_longlong(v),
      [](unsigned long long a, unsigned long long b) {
        return (unsigned long long)__double_as_longlong(fmin(__longlong_as_double((long long)a), __longlong_as_double((long long)b)));
      }));
}
__device__ inline double wave_max(double v) {
  return __longlong_as_double((long long)wave_reduce_u64((unsigned long long)__double_as_longlong(v),
      [](unsigned long long a, unsigned long long b) {
        return (unsigned long long)__double_as_longlong(fmax(__longlong_as_double((long long)a), __longlong_as_double((long long)b)));
      }));
}
__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
  return wave_reduce_u64(v, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
}

// positive doubles compare like their bit patterns
__device__ inline void atomic_min_pos_double(double* addr, double v) {
  atomicMin((unsigned long long*)addr, (unsigned long long)__double_as_longlong(v));
}
__device__ inline void atomic_max_double(double* addr, double v) {
  // general sign: CAS loop (rare: once per wave)
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a;
  while (__longlong_as_double((long long)old) < v) {
    const unsigned long long assumed = old;
    old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(v));
    if (old == assumed) break;
  }
}
