// Everything the joint QP rebuilds per rho.  The fixed part of the KKT matrix, H_f = (2 + sigma) I + rho F^T w F, is one
// K x K block for every column; this file owns G0 = F^T w F (once per object), H_f, its exact inverse (one workgroup in
// LDS up to K = SCP_INV_LDS_MAX_K, two launches per pivot beyond), T = S0 H_f^{-1}, the MFMA operand packing of both, and
// the per-object cache of these blocks by rho (adaptive rho moves on a grid, so the same few values recur).
#include "scp_qp_internal.h"

#include <algorithm>

// G0[a][b] = sum_r w_r F[r][a] F[r][b]  (constant per problem shape: once at create)
__global__ __launch_bounds__(256) void build_g0_kernel(int K, int Rf, const double* __restrict__ F,
                                                        const double* __restrict__ wrow, double* __restrict__ G0) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * K) return;
  const int a = t / K, b = t % K;
  double s = 0.0;
  for (int r = 0; r < Rf; ++r) s += wrow[r] * F[(int64_t)r * K + a] * F[(int64_t)r * K + b];
  G0[t] = s;
}

// Hf[a][b] = (2 + sigma) delta_ab + rho G0[a][b];  HS = [Hf ; S0];  aug = [Hf | I]
__global__ __launch_bounds__(256) void build_hf_kernel(int K, double rho, double sigma, const double* __restrict__ G0,
                                                        const double* __restrict__ S0, double* __restrict__ Hf,
                                                        double* __restrict__ HS, double* __restrict__ aug) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * K) return;
  const int a = t / K, b = t % K;
  const double v = rho * G0[t] + (a == b ? 2.0 + sigma : 0.0);
  Hf[t] = v;
  HS[t] = v;
  HS[K * K + t] = S0[t];
  aug[(int64_t)a * 2 * K + b] = v;
  aug[(int64_t)a * 2 * K + K + b] = a == b ? 1.0 : 0.0;
}

// Gauss-Jordan inverse with [Hf | I] resident in LDS (K <= SCP_INV_LDS_MAX_K); same operations as the global one.
// Thread (ty, tx): column tx of the augmented matrix, rows ty, ty + TY, ... (no integer divisions in the pivot loop).
__global__ __launch_bounds__(1024) void spd_inverse_lds_kernel(int K, const double* __restrict__ Hf, double* __restrict__ Minv) {
  extern __shared__ double sh[];  // aug[K][2K] | prow[2K] | col[K]
  const int W = 2 * K;
  double* aug = sh;
  double* prow = aug + K * W;
  double* col = prow + W;
  const int TX = W <= 128 ? 128 : 256, TY = 1024 / TX;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
  if (tx < W)
    for (int r = ty; r < K; r += TY) aug[r * W + tx] = tx < K ? Hf[r * K + tx] : (tx - K == r ? 1.0 : 0.0);
  __syncthreads();
  for (int p = 0; p < K; ++p) {
    const double piv = aug[p * W + p];
    if (threadIdx.x < W) prow[threadIdx.x] = aug[p * W + threadIdx.x] / piv;
    else if (threadIdx.x >= 512 && threadIdx.x - 512 < K) col[threadIdx.x - 512] = aug[(threadIdx.x - 512) * W + p];
    __syncthreads();
    if (tx < W) {
      const double pr = prow[tx];
      for (int r = ty; r < K; r += TY) {
        if (r == p) aug[r * W + tx] = pr;
        else aug[r * W + tx] -= col[r] * pr;
      }
    }
    __syncthreads();
  }
  if (tx < K)
    for (int r = ty; r < K; r += TY) Minv[r * K + tx] = aug[r * W + K + tx];
}

// Gauss-Jordan inverse for K > SCP_INV_LDS_MAX_K, two small launches per pivot over the whole chip: the pivot row (scaled)
// and the pivot column are first copied out, then every element of aug = [Hf | I] is updated from them -- the same
// operation per element as the one-workgroup kernels (bit-identical result), but a pivot's K x 2K update is spread over
// all CUs instead of dragging the 4 MB matrix (K = 500) through one CU 500 times (61 ms -> ~3 ms per inverse; the
// reference's demo, K = 500, spent 88 % of its 0.65 s there).
__global__ __launch_bounds__(256) void gj_extract_kernel(int K, int p, const double* __restrict__ aug, double* __restrict__ prow,
                                                          double* __restrict__ pcol) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int W = 2 * K;
  if (t < W) prow[t] = aug[(int64_t)p * W + t] / aug[(int64_t)p * W + p];
  else if (t - W < K) pcol[t - W] = aug[(int64_t)(t - W) * W + p];
}
__global__ __launch_bounds__(256) void gj_update_kernel(int K, int p, double* __restrict__ aug, const double* __restrict__ prow,
                                                         const double* __restrict__ pcol) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W = 2 * K;
  if (e >= (int64_t)K * W) return;
  const int r = (int)(e / W), c = (int)(e % W);
  if (r == p) aug[e] = prow[c];
  else aug[e] -= pcol[r] * prow[c];
}
__global__ __launch_bounds__(256) void gj_finish_kernel(int K, const double* __restrict__ aug, double* __restrict__ Minv) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < K * K) Minv[t] = aug[(int64_t)(t / K) * 2 * K + K + (t % K)];
}

// H_f^{-1} and T of a slot into the MFMA A-operand order (see QpDev::pMinv): both matrices in one launch
namespace {
struct PackDesc {
  const double* src;
  double* dst;
  int R, M;
};
struct PackArgs {
  PackDesc m[2];
};
__global__ __launch_bounds__(256) void pack_operands_kernel(PackArgs a) {
  const PackDesc d = a.m[blockIdx.y];
  const int nks = (d.M + 3) >> 2;
  const int64_t total = (int64_t)((d.R + 15) >> 4) * nks * 64;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int lane = (int)(e & 63);
    const int64_t q = e >> 6;
    const int ks = (int)(q % nks), t = (int)(q / nks);
    const int row = t * 16 + (lane & 15), k = 4 * ks + (lane >> 4);
    d.dst[e] = (row < d.R && k < d.M) ? d.src[(size_t)row * d.M + k] : 0.0;
  }
}

size_t al32(size_t n) { return (n + 31) / 32 * 32; }  // doubles, to a 256-byte boundary

size_t kkt_slot_doubles(int K) {  // Hf, HS, Minv, T + packed Minv, T, each 256-byte aligned
  return al32((size_t)K * K) * 3 + al32((size_t)2 * K * K) + 2 * al32(scp_packed_count(K, K));
}

// Adaptive rho moves on a geometric grid (steps of 2^(1/4)), so a solver object that is reused from scenario to scenario
// (compute-trajectories-batch) keeps meeting the same values: short horizons get enough slots to hold them all.
int kkt_slots(int K) {
  const size_t per = kkt_slot_doubles(K) * sizeof(double);
  const size_t fit = SCP_KKT_POOL_BYTES / per;
  return (int)std::min<size_t>(SCP_KKT_SLOTS_MAX, std::max<size_t>(SCP_KKT_SLOTS, fit));
}

// the active slot's H_f^{-1} and T in the MFMA operand order (see QpDev::pMinv)
int pack_operands(scp_qp* qp) {
  const QpDev& d = qp->d;
  const int K = qp->K;
  PackArgs a;
  a.m[0] = {d.Minv, d.pMinv, K, K};
  a.m[1] = {d.T, d.pT, K, K};
  return qp_launch(qp, pack_operands_kernel, dim3(16, 2), dim3(256), 0, a);
}

}  // namespace

size_t scp_qp_kkt_pool_doubles(int K) { return (size_t)kkt_slots(K) * kkt_slot_doubles(K); }

void scp_qp_kkt_init_slots(scp_qp* qp) {
  const int K = qp->K;
  double* base = qp->d.kkt_pool;
  qp->n_kkt = kkt_slots(K);
  for (int i = 0; i < qp->n_kkt; ++i) {
    auto& k = qp->kkt[i];
    double* q = base;
    k.rho = k.sigma = 0.0;
    k.used = 0;
    k.Hf = q; q += al32((size_t)K * K);
    k.Minv = q; q += al32((size_t)K * K);
    k.T = q; q += al32((size_t)K * K);
    k.HS = q; q += al32((size_t)2 * K * K);
    k.pMinv = q; q += al32(scp_packed_count(K, K));
    k.pT = q;
    base += kkt_slot_doubles(K);
  }
  qp->kkt_clock = 0;
}

int scp_qp_build_g0(scp_qp* qp) {
  const QpDev& d = qp->d;
  return qp_launch(qp, build_g0_kernel, grid1((int64_t)qp->K * qp->K), dim3(256), 0, qp->K, qp->Rf, d.F, d.wrow, d.G0);
}

int scp_qp_build_kkt(scp_qp* qp) {
  QpDev& d = qp->d;
  const int K = qp->K;
  const dim3 b256(256);
  // cache lookup: the blocks of this (rho, sigma) may still be resident
  scp_qp::KktSlot* slot = nullptr;
  for (int i = 0; i < qp->n_kkt; ++i)
    if (qp->kkt[i].used && qp->kkt[i].rho == qp->rho && qp->kkt[i].sigma == qp->st.sigma) slot = &qp->kkt[i];
  const bool hit = slot != nullptr;
  if (!hit) {
    slot = &qp->kkt[0];
    for (int i = 0; i < qp->n_kkt; ++i)
      if (qp->kkt[i].used < slot->used) slot = &qp->kkt[i];  // empty (0) or least recently used
  }
  slot->used = ++qp->kkt_clock;
  d.Hf = slot->Hf; d.HS = slot->HS; d.Minv = slot->Minv; d.T = slot->T;
  d.pMinv = slot->pMinv; d.pT = slot->pT;
  if (hit) return SCP_OK;
  slot->rho = qp->rho;
  slot->sigma = qp->st.sigma;
  QP_CHECK(qp_launch(qp, build_hf_kernel, grid1((int64_t)K * K), b256, 0, K, qp->rho, qp->st.sigma, d.G0, d.S0, d.Hf, d.HS, d.aug));
  if (K <= SCP_INV_LDS_MAX_K) {
    const size_t lds = ((size_t)K * 2 * K + 3 * K) * sizeof(double);  // (beyond 64 KiB from K = 64)
    QP_CHECK(qp_launch(qp, spd_inverse_lds_kernel, dim3(1), dim3(1024), lds, K, d.Hf, d.Minv));
  } else {
    double* prow = d.gj_tmp;
    double* pcol = d.gj_tmp + 2 * K;
    for (int p = 0; p < K; ++p) {
      QP_CHECK(qp_launch(qp, gj_extract_kernel, grid1((int64_t)3 * K), b256, 0, K, p, d.aug, prow, pcol));
      QP_CHECK(qp_launch(qp, gj_update_kernel, grid1((int64_t)K * 2 * K), b256, 0, K, p, d.aug, prow, pcol));
    }
    QP_CHECK(qp_launch(qp, gj_finish_kernel, grid1((int64_t)K * K), b256, 0, K, d.aug, d.Minv));
  }
  // T = S0 H_f^{-1}: the persistent kernel forms S0 p = T r on spare matrix-core waves next to p = H_f^{-1} r
  QP_CHECK(scp_launch_gemm(qp->ctx, 1, K, K, K, 1.0, d.S0, d.Minv, 0.0, d.T));
  return pack_operands(qp);
}
