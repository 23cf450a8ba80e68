// Device-side helpers shared by the column kernels of the joint QP (scp_qp_columns.hip, scp_qp_rows.hip, scp_qp_persist.hip): wave-wide
// scans on data-parallel-primitive (DPP) moves, MFMA operand prefetch, LDS padding, and the blocks of a column kernel built
// on them (column_At, column_forward, admm_project; the last also used by scp_qp_generic.hip).  gfx950 only.
#pragma once
#include "scp_qp_internal.h"
#include "scp_wave_device.h"

namespace scpdev {

constexpr int CB = 16;    // columns per workgroup of the column kernels (one MFMA tile wide)
constexpr int CHB = 16;   // operand registers (k steps) held at once by a tile product

typedef double double4_t __attribute__((ext_vector_type(4)));

// Operands of the first CH k-steps of row tile t of a packed matrix (QpDev::pMinv ...: [row tile][k step][lane]):
// fetched at kernel entry, long before the vector they multiply exists.
template <int CH>
__device__ inline void tile_prefetch(const double* __restrict__ P, int nks, int t, int ks0, int ks1, double (&a)[CH]) {
  const double* Ap = P + (size_t)t * nks * 64 + (threadIdx.x & 63);
#pragma unroll
  for (int s = 0; s < CH; ++s) a[s] = Ap[(size_t)min(ks0 + s, ks1 - 1) * 64];
}

// ---- wave-wide prefix sums over the time index: the integrator blocks V, S, S0 and their transposes are first and
// second cumulative sums.  DPP moves (scp_wave_device.h; no LDS round trip, unlike __shfl): lanes without a source read 0
// inclusive sum over the 64 lanes: row_shr 1, 2, 4, 8, then row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2, 3
__device__ inline double wave_incl_sum(double v) {
  v += dpp_move<0x111, 0xF, false>(v);
  v += dpp_move<0x112, 0xF, false>(v);
  v += dpp_move<0x114, 0xF, false>(v);
  v += dpp_move<0x118, 0xF, false>(v);
  v += dpp_move<0x142, 0xA, false>(v);
  v += dpp_move<0x143, 0xC, false>(v);
  return v;
}
// maximum of non-negative values over the 64 lanes, valid in lane 63
__device__ inline double wave_max_nn(double v) {
  v = fmax(v, dpp_move<0x111, 0xF, false>(v));
  v = fmax(v, dpp_move<0x112, 0xF, false>(v));
  v = fmax(v, dpp_move<0x114, 0xF, false>(v));
  v = fmax(v, dpp_move<0x118, 0xF, false>(v));
  v = fmax(v, dpp_move<0x142, 0xA, false>(v));
  v = fmax(v, dpp_move<0x143, 0xC, false>(v));
  return v;
}
__device__ inline double lane_below(double v) { return dpp_move<0x138, 0xF, false>(v); }  // wave_shr:1 (lane 0 <- 0)
__device__ inline double lane_above(double v) { return dpp_move<0x130, 0xF, false>(v); }  // wave_shl:1 (lane 63 <- 0)

__device__ inline double read_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// inclusive SUFFIX sum over the 64 lanes (lane l <- sum of lanes >= l): row_shl 1, 2, 4, 8 inside the rows of 16, then
// the totals of the higher rows (lanes 16, 32, 48 after the row scans) are added through scalar registers
__device__ inline double wave_incl_rsum(double v) {
  v += dpp_move<0x101, 0xF, false>(v);
  v += dpp_move<0x102, 0xF, false>(v);
  v += dpp_move<0x104, 0xF, false>(v);
  v += dpp_move<0x108, 0xF, false>(v);
  const double t1 = read_lane(v, 16), t2 = read_lane(v, 32), t3 = read_lane(v, 48);
  const int lane = threadIdx.x & 63;
  const double t23 = t2 + t3;
  const double add = lane < 16 ? t1 + t23 : (lane < 32 ? t23 : (lane < 48 ? t3 : 0.0));
  return v + add;
}

// inclusive and exclusive prefix sums over the index i = lane E + e (ascending)
template <int E>
__device__ inline void wave_scan(const double (&v)[E], double (&incl)[E], double (&excl)[E]) {
  double run = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    excl[e] = run;
    run += v[e];
    incl[e] = run;
  }
  const double off = lane_below(wave_incl_sum(run));  // total of the lower lanes
#pragma unroll
  for (int e = 0; e < E; ++e) {
    incl[e] += off;
    excl[e] += off;
  }
}
// value at index i - 1 / i + 1 (0 outside)
template <int E>
__device__ inline void wave_prev(const double (&v)[E], double (&o)[E]) {
  o[0] = lane_below(v[E - 1]);
#pragma unroll
  for (int e = 1; e < E; ++e) o[e] = v[e - 1];
}
template <int E>
__device__ inline void wave_next(const double (&v)[E], double (&o)[E]) {
  o[E - 1] = lane_above(v[0]);
#pragma unroll
  for (int e = 0; e + 1 < E; ++e) o[e] = v[e + 1];
}

// per-column LDS rows are padded to a length = 2 (mod 32) doubles: the (column, time) accesses of the coalesced
// global <-> LDS copies (16 columns x 2 steps per half wave) and of the MFMA operand reads then hit 32 distinct banks
__host__ __device__ inline int pad_col(int n) { return ((n + 29) / 32) * 32 + 2; }

// incidence-list cell of (time step k, agent): agent-major, so that the entries of a block of consecutive agents are one
// contiguous range (the persistent kernel keeps them in LDS)
__host__ __device__ inline int cell_of(int k, int agent, int K) { return agent * K + k; }

// ---- the blocks of a column kernel (scp_qp_columns.hip): one wave per column c = (agent, axis), E time steps per lane, the
// column's vectors in LDS.  F = [J ; I ; V ; S] and S0 are the jerk stencil and the first / second cumulative sums of the
// integrator (scp.py:10-28, :489-491), so each block costs wave-wide scans instead of a dense product.  The order of every
// sum below is the one oracle/qp_oracle.py:admm_structured restates; the persistent kernels hold their own lane-per-step
// copies of the same formulas (scp_qp_persist_device.h).

// A^T v = F^T v_f + S0^T G for one column, v_f in Vc[0, 4K - 1), G (the gathered collision-row values) in Gc[0, K):
//   J^T v_j + v_a + rsum(h v_v + h^2/2 (v_p - g)) + h^2/2 g + h^2 rsum_excl(rsum(v_p + g))
// Index i = lane E + e runs over the time steps in DESCENDING order (k = 64 E - 1 - i), so the reverse cumulative sums are
// ascending scans over the lanes; out[e] belongs to that k.  WITH_G = false (no collision rows: Gc is not read) drops the
// terms in g instead of adding zeros, which could flip the sign of a zero.
template <int E, bool WITH_G>
__device__ __forceinline__ void column_At(int K, double h, const double* Vc, const double* Gc, double (&out)[E]) {
  const int lane = threadIdx.x & 63, KM = 64 * E - 1;
  const double hh = h * h;
  double vj[E], va[E], u1[E], u2[E], g[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = KM - (lane * E + e);
    const bool ok = k < K;
    vj[e] = k < K - 1 ? Vc[k] : 0.0;
    va[e] = ok ? Vc[K - 1 + k] : 0.0;
    const double vv = ok ? Vc[2 * K - 1 + k] : 0.0;
    const double vp = ok ? Vc[3 * K - 1 + k] : 0.0;
    if constexpr (WITH_G) {
      g[e] = ok ? Gc[k] : 0.0;
      u1[e] = h * vv + 0.5 * hh * (vp - g[e]);
      u2[e] = vp + g[e];
    } else {
      u2[e] = vp;
      u1[e] = h * vv + 0.5 * hh * u2[e];
    }
  }
  double d1[E], d2[E], s1[E], s2[E], vjp[E];
  wave_scan<E>(u1, d1, s1);   // d1 = rsum(u1)
  wave_scan<E>(u2, s1, s2);   // s1 = rsum(u2)
  wave_scan<E>(s1, s2, d2);   // d2 = rsum_excl(rsum(u2))
  wave_next<E>(vj, vjp);      // v_j[k - 1]
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if constexpr (WITH_G) out[e] = ((vjp[e] - vj[e]) / h + va[e]) + (d1[e] + 0.5 * hh * g[e]) + hh * d2[e];
    else out[e] = ((vjp[e] - vj[e]) / h + va[e]) + d1[e] + hh * d2[e];
  }
}

// F p -> Wc[0, 4K - 1) and, WITH_S0, S0 p -> Qc[0, K) for one column, p[e] = p at time step k = lane E + e (0 beyond K):
//   J p = (p[k+1] - p[k]) / h,  I p,  V p = h csum(p),  S p = h^2 (csum_excl(csum p) + csum(p)/2),
//   S0 p = h^2 (csum_excl(csum p) - csum(p)[k-1]/2)
template <int E, bool WITH_S0>
__device__ __forceinline__ void column_forward(int K, double h, const double (&p)[E], double* Wc, double* Qc) {
  const int lane = threadIdx.x & 63;
  const double hh = h * h;
  double c1[E], c2[E], t1[E], t2[E], c1p[E], pn[E];
  wave_scan<E>(p, c1, t1);   // c1 = csum(p)
  wave_scan<E>(c1, t2, c2);  // c2 = csum_excl(csum(p))
  if constexpr (WITH_S0) wave_prev<E>(c1, c1p);
  wave_next<E>(p, pn);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = lane * E + e;
    if (k < K) {
      if constexpr (WITH_S0) Qc[k] = hh * (c2[e] - 0.5 * c1p[e]);
      if (k < K - 1) Wc[k] = (pn[e] - p[e]) / h;
      Wc[K - 1 + k] = p[e];
      Wc[2 * K - 1 + k] = h * c1[e];
      Wc[3 * K - 1 + k] = hh * (c2[e] + 0.5 * c1[e]);
    }
  }
}

// Projection and dual update of one row from its relaxed value zh (OSQP steps 5-6):
//   zn = clamp(zh + y / rho_r, lo, hi),  yn = y + rho_r (zh - zn);   without hi: a collision row (u = +inf)
__device__ __forceinline__ void admm_project(double zh, double y, double rho_r, double lo, double hi, double& zn, double& yn) {
  zn = fmin(fmax(zh + y / rho_r, lo), hi);
  yn = y + rho_r * (zh - zn);
}
__device__ __forceinline__ void admm_project(double zh, double y, double rho_r, double lo, double& zn, double& yn) {
  zn = fmax(zh + y / rho_r, lo);
  yn = y + rho_r * (zh - zn);
}

}  // namespace scpdev
