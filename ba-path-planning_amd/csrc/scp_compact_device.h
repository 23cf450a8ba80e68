// Bitmap -> sorted row list inside ONE workgroup, and the stats mirror: shared by the compaction kernels and by the tail
// of the one-launch pairwise passes (both in scp_kernels.hip).
#pragma once
#include "scp_common.h"

constexpr int CMP_THREADS = 256;
constexpr int CMP_WPT = 4;                              // bitmap words per thread
constexpr int CMP_WORDS = CMP_THREADS * CMP_WPT;        // per workgroup
constexpr int64_t CMP1_MAX_WORDS = 64 * 1024;           // bitmap words (2 M rows) one workgroup compacts (compact_small_body)

// exclusive scan of one value per thread over a workgroup of CMP_THREADS threads (all of them must call it); *total: their sum
__device__ inline int block_exclusive_scan(int v, int* total) {
  __shared__ int wsum[CMP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < CMP_THREADS / 64; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// The finished stats of a pass with a row list also go to the ctx's mapped host mirror (sequence number last): the
// native SCP loop reads them from there without a copy launch and without draining the stream.
__device__ inline void publish_stats(const scp_pair_stats* stats, unsigned long long n_selected, scp_stats_mirror* mirror,
                                     unsigned long long seq) {
  if (!mirror) return;
  const double mind = __hip_atomic_load(&stats->min_dist, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double maxv = __hip_atomic_load(&stats->max_violation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long fv =
      __hip_atomic_load((const unsigned long long*)&stats->first_violation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store((unsigned long long*)&mirror->stats.min_dist, (unsigned long long)__double_as_longlong(mind),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store((unsigned long long*)&mirror->stats.first_violation, fv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store((unsigned long long*)&mirror->stats.n_selected, n_selected, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store((unsigned long long*)&mirror->stats.max_violation, (unsigned long long)__double_as_longlong(maxv),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store((unsigned long long*)&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Count, scan, write of a small map (up to CMP1_MAX_WORDS words) for THREADS threads of ONE workgroup (all of them must call it): returns the number of set bits.
// OVERWRITE: merge_into := map (every word, also the empty ones: the working-set bitmap of a NEW linearisation, no clearing
// launch), map := 0.  COHERENT: the bits were set by other workgroups of the SAME kernel (the small-problem passes run this
// as their tail): the words are read past this XCD's L2.
template <int THREADS, bool COHERENT>
__device__ inline int compact_small_body(uint32_t* __restrict__ map, int64_t words, int64_t nq, int64_t q_begin,
                                         int64_t pairs, int64_t* __restrict__ rows, int64_t cap,
                                         uint32_t* __restrict__ merge_into, bool overwrite) {
  __shared__ int wsum[THREADS / 64];
  __shared__ int total_sh;
  constexpr int CHUNK = THREADS * CMP_WPT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto load = [&](int64_t w) -> uint32_t {
    return COHERENT ? __hip_atomic_load(map + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : map[w];
  };
  // pass 1: the total (decides whether a merging pass may merge at all)
  int c_all = 0;
  for (int64_t w = threadIdx.x; w < words; w += THREADS) c_all += __popc(load(w));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c_all += __shfl_xor(c_all, o);
  __syncthreads();  // (wsum / total_sh of an earlier call in the same kernel have been read)
  if (lane == 0) wsum[wave] = c_all;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < THREADS / 64; ++w) t += wsum[w];
    total_sh = t;
  }
  __syncthreads();
  const int total = total_sh;
  const bool overflow = merge_into != nullptr && !overwrite && (int64_t)total > cap;
  // pass 2: chunk by chunk in row order, block scan per chunk
  int64_t carry = 0;
  for (int64_t base = 0; base < words && (total > 0 || overwrite); base += CHUNK) {
    const int64_t w0 = base + (int64_t)threadIdx.x * CMP_WPT;
    uint32_t wd[CMP_WPT];
    int c = 0;
#pragma unroll
    for (int i = 0; i < CMP_WPT; ++i) {
      wd[i] = (w0 + i < words) ? load(w0 + i) : 0u;
      c += __popc(wd[i]);
    }
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    __syncthreads();  // wsum of the previous chunk (or of pass 1) has been read by everyone
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
      if (w < wave) before += wsum[w];
      tot += wsum[w];
    }
    int64_t slot = carry + before + incl - c;
    carry += tot;
    if (overwrite) {
#pragma unroll
      for (int i = 0; i < CMP_WPT; ++i)
        if (w0 + i < words) merge_into[w0 + i] = wd[i];
    }
    if (c == 0) continue;
#pragma unroll
    for (int i = 0; i < CMP_WPT; ++i) {
      uint32_t m = wd[i];
      if (m && merge_into) {
        if (!overflow && !overwrite) merge_into[w0 + i] |= m;
        map[w0 + i] = 0u;
      }
      if (m) {
        // local row lr = 32 (w0 + i) + bit -> global id (lr / nq) pairs + q_begin + lr % nq with ONE 64-bit division per
        // word (its bits belong to at most two time steps when nq >= 32; the inner loop covers tiny pair ranges)
        const int64_t base = (w0 + i) * 32;
        const int64_t kk = base / nq, rr = base - kk * nq;
        while (m) {
          const int bit = __ffs((int)m) - 1;
          m &= m - 1;
          int64_t k2 = kk, r2 = rr + bit;
          while (r2 >= nq) {
            r2 -= nq;
            ++k2;
          }
          if (!overflow && slot < cap) rows[slot] = k2 * pairs + q_begin + r2;
          ++slot;
        }
      }
    }
  }
  return total;
}
