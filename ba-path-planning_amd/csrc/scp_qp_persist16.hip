// Lean form of the persistent single-step ADMM kernel: SIXTEEN agents (= waves) per workgroup, so that 2-D problems of up to
// 16 x 256 = 4096 agents keep one workgroup per compute unit and stay on the persistent path (config 4 of BASELINE.json on
// one GPU; the 8-agent kernel of scp_qp_persist.hip stops at 2048 agents and the three-launch pipeline behind it costs
// 51 us per ADMM step at 4096 x 50 against ~10 us here).  Replaces osqp's solve loop at
// /root/reference/src/path_planning/solvers/scp.py:441-445 like its sibling; same algorithm, same exchanges, same exit
// protocol (scp_qp_persist_device.h) -- what changes is the register diet that four waves per SIMD (128 registers each)
// demand:
//   * ONE double per fixed row instead of two: v = z~ + y / rho, the point the projection is applied to.  ADMM's update
//     z' = Pi(v'), y' = rho (v' - Pi(v')) with v' = alpha F x~ + (1 - alpha) z + y / rho keeps z = Pi(v), y = rho (v - Pi(v)) as an
//     invariant, so v' = v + alpha (F x~ - Pi(v)) and z, y are two clamps away wherever they are needed ("one
//     state double per row").  The invariant holds after any ADMM update but not after scp_qp_reset (z = A x0 unprojected,
//     y = 0): the first step of a QP takes z = v itself (PersistArgs::first_step).  Rounding-level differences only;
//   * x and its first / second prefix sums c1 = cumsum(x), c2 = cumsum(c1) (exclusive) are carried, and F x, S0 x re-derived
//     from them where the 8-agent kernel carries the F x slab (16 registers) and S0 x; F (x + a p) likewise comes from
//     (c1 + a cumsum p, c2 + a cumsum^2 p), so F p is never formed.  Same quantities, sums associated differently;
//   * the jerk / acceleration limits are scalars (scp.py:188-195: the same for every row), only the velocity / position
//     bounds are per row;
//   * H_f^{-1} (packed MFMA operands, 26 KB at K = 50) lives in LDS and is streamed into the matrix cores, not held in 32
//     registers per lane; eight waves run the 4 row tiles x 2 column tiles of p = H_f^{-1} r; S0 p comes from two more
//     prefix scans (no T = S0 H_f^{-1} tiles: the matrix pipes are the busiest unit with four waves per SIMD).  <2, 8>
//     instead forms S0 p = T r on the four waves its single column tile leaves idle and publishes the cells from the
//     accumulators, so the hand-off starts before any scan (t_on_mfma);
//   * a collision row carries its value at x, c . (S0 x_own - S0 x_partner), instead of both S0 x cells: z~ and the next
//     row value are fma(a, s, ax), fma(alpha a, s, ax) with s the row value of p the row loop forms anyway, and the
//     check refreshes it exactly;
//   * delta-y of a batch's last step (primal infeasibility certificate) is reduced on the spot -- |dy|, the support value and
//     |A^T dy| per lane -- instead of being kept in 16 registers until the check;
//   * y / rho and (.) / h are multiplications by reciprocals (fp64 division is ~14 VALU instructions a piece, eight of them
//     per lane and step).
// Entry tables: 68 B per incident row in 2-D (76 B in 3-D) in the LDS that is left (1280 rows around a block of 16 agents
// at 4096 x 50, 1088 around one of 8 at 1024 x 50; more -> EXIT_OVERFLOW -> three-launch pipeline for that working set).
#include "scp_qp_persist_device.h"

namespace {
using namespace scpdev;
using namespace scp_persist;

// Developer build (make prof): 100 MHz wall-clock ticks per phase, summed over the steps of one launch, middle workgroup,
// thread 0; the accumulators live in LDS (the kernel has no registers to spare).
#ifdef SCP_PHASE_PROFILE
__device__ unsigned long long scp_persist16_clk[16];
#define PSTAMP(slot)                                           \
  do {                                                         \
    if (prof_t) {                                              \
      const unsigned long long now_ = wall_clock64();          \
      pacc_s[slot] += now_ - pacc_s[15];                       \
      pacc_s[15] = now_;                                       \
    }                                                          \
  } while (0)
#else
#define PSTAMP(slot) ((void)0)
#endif

// Instantiations: <2, 16> the lean kernel proper (2-D, 2048 < N <= 4096: four waves per SIMD, 128 registers);
// <3, 8> 3-D with eight agents per workgroup (1024 < N <= 2048: the 4-agent 3-D kernel of scp_qp_persist.hip stops at 1024);
// <2, 8> the same state diet at two waves per SIMD (settings.persistent = 3: measurements against the 8-agent kernel).
constexpr int nct_of(int D, int APB) { return (D * APB + 15) / 16; }  // 16-column MFMA tiles of a workgroup
constexpr int AB_STRIDE = 32;  // per-agent bound table: 8 groups of 4 doubles

// <2, 8> has four of its eight waves idle in the MFMA phase (one column tile): they form S0 p = T r (T = S0 H_f^{-1}, packed
// like H_f^{-1}) next to p = H_f^{-1} r and publish the cells straight from the accumulators, before any prefix scan.  (<2, 16>
// would have the waves too, but not the registers or the LDS; <3, 8> has none.)
constexpr bool t_on_mfma(int D, int APB) { return 4 * nct_of(D, APB) < APB && APB <= 8; }
// K slices of the MFMA phase whose operand loads are in flight together (4 registers each).  <2, 16> takes none: at 128
// registers every form of the ring, even one slot deep, spills two registers more than the plain loop (65).  Eight-agent
// kernels at 1024 x 50: 2, 3 and 4 slots measure within 0.1 us per step of each other, 5 and 8 slower again
// (DESIGN.md 3.3).
constexpr int mfma_slices(int D, int APB) { return APB > 8 ? 1 : 4; }
// entry tables, doubles per incident row: signed eta [D], l, z, y, g, c . (S0 x_own - S0 x_partner), c . (S0 p_own - S0 p_partner)
constexpr int ent_doubles(int D) { return D + 6; }

struct Lds16 {  // carve-up shared by the kernel and the host's size computation (doubles, then ints)
  int RSK, tK, nks;
  size_t rt, pt, qt, ml, tl, gp, ab, gchk, ent, n_dbl;
  __host__ __device__ Lds16(int K, int cap, int nblk, int D, int APB) {
    const int NC16 = 16 * nct_of(D, APB), APB16 = APB;
    const bool tq = t_on_mfma(D, APB);
    RSK = pad_col(K);
    tK = (K + 15) >> 4;
    nks = (K + 3) >> 2;
    size_t o = 0;
    rt = o; o += (size_t)NC16 * RSK;
    pt = o; o += (size_t)NC16 * RSK;
    ml = o; o += (size_t)tK * nks * 64;
    qt = pt;  // (scan path: S0 p overwrites p in place)
    tl = ml;
    if (tq) {
      qt = o; o += (size_t)NC16 * RSK;
      tl = o; o += (size_t)tK * nks * 64;
    }
    gp = o; o += (size_t)2 * nblk;
    ab = o; o += (size_t)APB16 * AB_STRIDE;
    // the nine-value all-gather of a termination check reuses the r / p tiles when they are large enough
    if ((size_t)2 * NC16 * RSK >= (size_t)NCHK * nblk) gchk = rt;
    else { gchk = o; o += (size_t)NCHK * nblk; }
    ent = o; o += (size_t)cap * ent_doubles(D);
    n_dbl = o;
  }
};

template <int D, int APB16>
__global__ __launch_bounds__(64 * APB16) void cg1_persist16_kernel(PersistArgs A) {
  constexpr int NT16 = 64 * APB16;             // threads: one wave per agent
  constexpr int NCT = nct_of(D, APB16);        // column tiles of the MFMA phase
  constexpr int NC16 = 16 * NCT;               // tile columns (D APB16 of them in use)
  constexpr bool TQ = t_on_mfma(D, APB16);     // S0 p = T r on the matrix waves the column tiles leave idle
  constexpr int MU = mfma_slices(D, APB16);    // K slices per batch of operand loads
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double red[NCHK][APB16];
  __shared__ double cert_s[3][APB16];  // per wave: |dy|, support value, |A^T dy| of the batch's last step (fixed rows)
  __shared__ double chk_s[NCHK];       // the nine results of the latest check (read again only at the exit)
  __shared__ int fail_s;
#ifdef SCP_PHASE_PROFILE
  __shared__ unsigned long long pacc_s[16];
  const bool prof_t = blockIdx.x == gridDim.x / 2 && threadIdx.x == 0;
  if (prof_t) {
    for (int i = 0; i < 15; ++i) pacc_s[i] = 0;
    pacc_s[15] = wall_clock64();
  }
#endif
  const int K = A.K, N = A.N;
  const int64_t C = A.C;
  const int cap = A.ent_cap, nblk = A.nblk;
  const Lds16 L(K, cap, nblk, D, APB16);
  const int RSK = L.RSK, tK = L.tK, nks = L.nks;
  double* Rt = lds + L.rt;            // [32][RSK] r, MFMA B operand
  double* Pt = lds + L.pt;            // [32][RSK] p (scan path: overwritten in place by the lane's S0 p cell)
  double* Qt = lds + L.qt;            // [32][RSK] the S0 p cells the row loop reads (TQ: T r; else = Pt)
  double* Ml = lds + L.ml;            // [tK][nks][64] packed H_f^{-1}
  double* Tl = lds + L.tl;            // [tK][nks][64] packed T = S0 H_f^{-1} (TQ only)
  double* gp = lds + L.gp;            // [nblk][2] all-gathered line-search partials
  double* ab = lds + L.ab;            // [APB][8 groups of 4] per agent, per axis: l_vel, u_vel, vf - v0, pos_min, pos_max, pf, -1e300, +1e300
  double* gck = lds + L.gchk;         // [nblk][9] all-gathered check results
  double* e_c = lds + L.ent;          // [cap][2] signed eta
  double* e_l = e_c + (size_t)cap * D;
  double* e_z = e_l + cap;
  double* e_y = e_z + cap;
  double* e_g = e_y + cap;            // row value of the next right-hand side
  double* e_ax = e_g + cap;           // row value at x: c . (S0 x_own - S0 x_partner), exact after a check, carried in between
  double* e_s = e_ax + cap;           // row value of this step's p: c . (S0 p_own - S0 p_partner); then delta-y parked for the check
  int* e_code = (int*)(lds + L.n_dbl);    // [cap] k | local agent << 6 | side << 10 | partner agent << 11
  int* cptr = e_code + cap;               // [16 K + 1] cell offsets relative to this workgroup's first entry

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a0 = blockIdx.x * APB16;
  const int agent = a0 + wave;
  const bool aok = agent < N;
  const int k = lane;
  const bool live = aok && k < K;
  const bool jok = live && k < K - 1;   // the jerk row of this lane exists
  const bool lastk = k == K - 1;        // the velocity / position rows of this lane are the final-state equalities
  const double h = A.h, hh = h * h, ih = 1.0 / h, alpha = A.alpha;
  double rho = A.rho, rho_c = A.rho_c;  // (an in-kernel rho switch changes them)
  unsigned n_rho = 0;

  // ---- entries of this block of agents (contiguous in the agent-major incidence lists) --------------------------
  const int a1 = min(a0 + APB16, N);
  // (own_lists: built here from the raw rows, with the r / p tiles, gp and e_s as scratch; else the slice of the host's lists)
  int ebase0 = 0, ne;
  if (A.own_lists) {
    ne = build_entry_tables<APB16, NT16>(A, a0, a1, cptr, e_code, (int*)e_s, (int*)Rt, (int*)gp);
    if (ne < 0) return;
  } else {
    ebase0 = A.cell_ptr[cell_of(0, a0, K)];
    ne = A.cell_ptr[cell_of(0, a1, K)] - ebase0;
    if (entries_overflow<APB16>(A)) return;
    for (int i = threadIdx.x; i <= (a1 - a0) * K; i += NT16) cptr[i] = A.cell_ptr[cell_of(0, a0, K) + i] - ebase0;
  }
  if (threadIdx.x == 0) fail_s = 0;
  for (int e = threadIdx.x; e < ne; e += NT16) {
    const bool own_lists = A.own_lists != 0;
    const int code = own_lists ? e_code[e] : A.ent_code[ebase0 + e];
    if (own_lists) A.own_code[(size_t)blockIdx.x * cap + e] = code;  // (n per entry again at the exit)
    const int n = code >> 1, side = code & 1;
    const int wi = A.w_i[n], wj = A.w_j[n], wk = A.w_k[n];
    const int own = side ? wj : wi, par = side ? wi : wj;
    e_code[e] = wk | ((own - a0) << 6) | (side << 10) | (par << 11);
    const int64_t bo = (int64_t)wk * C + (int64_t)own * D, bp = (int64_t)wk * C + (int64_t)par * D;
    double ax = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double eta = A.w_eta[(size_t)n * D + d];
      const double c = side ? -eta : eta;
      e_c[(size_t)e * D + d] = c;
      ax += c * (A.Qx[bo + d] - A.Qx[bp + d]);
    }
    e_ax[e] = ax;
    e_l[e] = A.w_l[n];
    const double zc = A.zc[n], yc = A.yc[n];
    e_z[e] = zc;
    e_y[e] = yc;
    e_g[e] = !own_lists ? A.gval[ebase0 + e] : (A.vals_carried ? A.grow[n] : first_row_value(rho_c, zc, yc, ax));
  }
  for (int i = threadIdx.x; i < NC16 * RSK; i += NT16) Rt[i] = 0.0;  // columns beyond the block stay zero
  for (int i = threadIdx.x; i < tK * nks * 64; i += NT16) {
    Ml[i] = A.pMinv[i];
    if constexpr (TQ) Tl[i] = A.pT[i];
  }

  // ---- column state: lane k of the agent's wave holds the rows of time step k --------------------------------------
  // row types t = 0 jerk (k < K - 1), 1 acc, 2 vel, 3 pos;  slab row of (t, k): t = 0: k, else t K - 1 + k
  double v[D][4], off[D], x[D], c1[D], c2[D];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool rok = t == 0 ? jok : live;
    const int row = t == 0 ? k : t * K - 1 + k;
    const double rr = (t >= 2 && lastk) ? rho * A.rho_eq : rho;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      v[d][t] = 0.0;
      if (rok) {
        const int64_t g = (int64_t)row * C + (int64_t)agent * D + d;
        v[d][t] = A.zf[g] + A.yf[g] / rr;
      }
    }
  }
  // The velocity / position bounds of this lane's rows are re-derived where they are needed -- bound_of() of scp_traj.hip,
  // the same arithmetic on the same operands (scp.py:212-224, :242-257), so the same bits as the lf / uf slabs -- from 4
  // registers (the free position of the row's state, k + 1) and eight per-agent scalars in LDS, instead of being held in 16.
  if (threadIdx.x < APB16 * D) {
    const int al = threadIdx.x / D, d = threadIdx.x % D, ag = a0 + al;
    double* o = ab + al * AB_STRIDE;
    const bool there = ag < N;
    const double v0 = there ? A.states[((size_t)N + ag) * D + d] : 0.0;
    o[d] = A.vel_lo - v0;                                                        // l_vel, k < K - 1
    o[4 + d] = A.vel_hi - v0;                                                    // u_vel
    o[8 + d] = (there ? A.states[((size_t)3 * N + ag) * D + d] : 0.0) - v0;      // final velocity equality: vf - v0
    o[12 + d] = A.pmin[d];
    o[16 + d] = A.pmax[d];
    o[20 + d] = there ? A.states[((size_t)2 * N + ag) * D + d] : 0.0;            // pf
    o[24 + d] = -1e300;                                                          // rows beyond the horizon: no bound at all,
    o[28 + d] = 1e300;                                                           // so that v = 0 stays 0 there
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
#pragma clang fp contract(off)
    const double p0 = aok ? A.states[(size_t)agent * D + d] : 0.0, v0 = aok ? A.states[((size_t)N + agent) * D + d] : 0.0;
    const double hk = h * (double)(k + 1);
    const double hkv = hk * v0;
    off[d] = p0 + hkv;  // scp.py:246-247
  }
  // which table entries bound this lane's velocity / position rows: the inequalities, the final-state equalities
  // (k = K - 1: lower = upper), or nothing (beyond the horizon) -- an address per lane instead of selects per use
  const double* const tb = ab + wave * AB_STRIDE;
  const double* const b_vl = tb + (live ? (lastk ? 8 : 0) : 24);
  const double* const b_vh = tb + (live ? (lastk ? 8 : 4) : 28);
  const double* const b_pl = tb + (live ? (lastk ? 20 : 12) : 24);
  const double* const b_ph = tb + (live ? (lastk ? 20 : 16) : 28);
  auto bounds = [&](int d, double (&lo)[2], double (&hi)[2]) {
    lo[0] = b_vl[d];
    hi[0] = b_vh[d];
    lo[1] = b_pl[d] - off[d];
    hi[1] = b_ph[d] - off[d];
  };
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = live ? A.x[(int64_t)k * C + (int64_t)agent * D + d] : 0.0;
    const double s1 = wave_incl_sum(x[d]);            // exact prefix sums of x (refreshed at every check)
    const double s2 = lane_below(wave_incl_sum(s1));
    c1[d] = live ? s1 : 0.0;                           // lanes beyond the horizon would hold the running totals: zero, so
    c2[d] = live ? s2 : 0.0;                           // that their (non-existent) rows contribute nothing to the suffix sums
  }
  const double jlo = A.jerk_lo, jhi = A.jerk_hi, alo = A.acc_lo, ahi = A.acc_hi;
  __syncthreads();
  // incidence-list range of this lane's cell (time step k of this wave's agent); cells without entries publish nothing
  const int c0 = aok ? cptr[wave * K + min(k, K - 1)] : 0;
  const int c1e = (aok && k < K) ? cptr[wave * K + k + 1] : c0;
  const bool has_rows = c1e > c0;
  u64* my_cell = A.cells + ((size_t)((int64_t)min(k, K - 1) * N + (aok ? agent : 0)) * D) * 2;
  double* my_pt = Pt + (size_t)(wave * D) * RSK + k;   // + d RSK: this lane's slot of column (agent, d)
  double* my_rt = Rt + (size_t)(wave * D) * RSK + k;
  // TQ, the waves that form T r: which of this lane's four accumulator rows (tile 16 + lk + 4 q of column li) belong to a
  // cell with rows, i.e. get published -- cptr does not change during a launch, so the step's epilogue looks nothing up
  unsigned pub_rows = 0;
  if constexpr (TQ) {
    const int li = lane & 15, al = li / D;
    if (wave >= 4 * NCT && wave < 4 * NCT + 4 && li < D * APB16 && a0 + al < N) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = (wave & 3) * 16 + (lane >> 4) + 4 * q;
        if (row < K && cptr[al * K + row + 1] > cptr[al * K + row]) pub_rows |= 1u << q;
      }
    }
  }

  PSTAMP(0);
  bool ok = true;
  int it_done = A.it0;      // ADMM iterations of this solve completed so far
  unsigned steps = 0;       // steps run by this launch
  unsigned exit_code = 0;
  const bool with_dy = A.eps_prim_inf > 0.0;
  if (threadIdx.x < 3 * APB16) (&cert_s[0][0])[threadIdx.x] = 0.0;
  int cad = A.cad0;  // steps between two checks: check_every, or check_fine once the residuals are close / rho has changed
  for (;;) {  // one batch of steps up to the next termination check, then the check and the decision to go on
  int nit = cad - it_done % cad;
  if (it_done + nit > A.max_iter) nit = A.max_iter - it_done;
  for (int it = 0; it < nit; ++it, ++steps) {
    const unsigned tag = A.epoch0 + steps + 1u;
    const bool last = it == nit - 1;
    // The one-double-per-row state presumes z = Pi(v).  Right after scp_qp_reset z = A x0 is NOT projected (and y = 0, so
    // v = z): the first step of a QP therefore takes z = v instead of Pi(v) -- W' = rho (v - F x), v' = alpha F x~ +
    // (1 - alpha) v, which is the standard update from (z, y) = (v, 0) -- and establishes the invariant for all later steps.
    const bool first = A.first_step && steps == 0u;
    u64* gpart = A.gpart + (size_t)(tag & 1u) * nblk * 4;
    const double rv = lastk ? rho * A.rho_eq : rho;   // rho of this lane's velocity / position rows
    // ---- r = -2 x + F^T W' + S0^T G: reverse cumulative sums as suffix scans over the lanes ------------------------
    {
      double r[D];
      double g[D];
#pragma unroll
      for (int d = 0; d < D; ++d) g[d] = 0.0;
      // (one entry per trip: with the loads of 2 - 4 entries in flight per wait -- indices clamped or lanes masked -- the
      // clamps and selects cost more VALU time at two waves per SIMD than the round trips they save)
      for (int e = c0; e < c1e; ++e) {
        const double ge = e_g[e];
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] += e_c[(size_t)e * D + d] * ge;
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        // W' = rho (z - F x) - y with z = Pi(v), y = rho (v - Pi(v))
        double lo[2], hi[2];
        bounds(d, lo, hi);
        const double xn = lane_above(x[d]);
        double cj = fmin(fmax(v[d][0], jlo), jhi), ca = fmin(fmax(v[d][1], alo), ahi);
        double cv = fmin(fmax(v[d][2], lo[0]), hi[0]), cp = fmin(fmax(v[d][3], lo[1]), hi[1]);
        if (first) { cj = v[d][0]; ca = v[d][1]; cv = v[d][2]; cp = v[d][3]; }  // z of a reset is A x0 itself (y = 0, v = z)
        const double wj = jok ? rho * ((cj - (xn - x[d]) * ih) - (v[d][0] - cj)) : 0.0;
        const double wa = rho * ((ca - x[d]) - (v[d][1] - ca));
        const double wv = rv * ((cv - h * c1[d]) - (v[d][2] - cv));
        const double wp = rv * ((cp - hh * (c2[d] + 0.5 * c1[d])) - (v[d][3] - cp));
        const double u1 = h * wv + 0.5 * hh * (wp - g[d]);
        const double u2 = wp + g[d];
        const double d1 = wave_incl_rsum(u1);
        const double s1 = wave_incl_rsum(u2);
        const double d2 = lane_above(wave_incl_rsum(s1));  // exclusive suffix sum
        const double wjm = lane_below(wj);                  // w_j[k - 1]
        r[d] = (((wjm - wj) * ih + wa) + (d1 + 0.5 * hh * g[d]) + hh * d2) - 2.0 * x[d];
        if (live) my_rt[d * RSK] = r[d];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    PSTAMP(1);
    // ---- p = H_f^{-1} r on the matrix cores: 4 row tiles x NCT column tiles, operands streamed from LDS; TQ: the next
    //      four waves form S0 p = T r from the same r tile and publish the cells (those with rows) from the accumulators ----
    if ((wave < 4 * NCT || (TQ && wave < 4 * NCT + 4)) && (wave & 3) < tK) {
      const bool tw = TQ && wave >= 4 * NCT;
      const int li = lane & 15, lk = lane >> 4;
      const int tile = wave & 3, ct = tw ? 0 : wave >> 2;
      const double* Mt = (tw ? Tl : Ml) + (size_t)tile * nks * 64 + lane;
      const double* Bt = Rt + (size_t)(ct * 16 + li) * RSK;
      // K slices s = 0 ... nks - 1 into the one accumulator, in that order.  The operands go through a ring of MU slots: the
      // loads of slice s + MU are issued as soon as the MFMA of slice s has taken its slot's operands, so MU slices' loads
      // are in flight while the MFMAs issue and an MFMA waits for the matrix pipe, not for its own LDS round trip.  Slice
      // indices are clamped (every load is in bounds, whatever it is used for); B beyond the horizon is an exact 0.0 by a
      // select (pad_col(K) < 4 nks for some K: no padding to rely on).
      auto load_slice = [&](int s, double& a, double& b) {  // (b: as loaded; the select is mfma_slice's, after the wait)
        s = min(s, nks - 1);
        a = Mt[(size_t)s * 64];
        b = Bt[min(4 * s + lk, K - 1)];
      };
      auto mfma_slice = [&](int s, double a, double b, double4_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, 4 * s + lk < K ? b : 0.0, c, 0, 0, 0);
      };
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
      if constexpr (MU > 1) {
        double am[MU], bm[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) load_slice(u, am[u], bm[u]);
        int s0 = 0;
        for (; s0 + MU <= nks; s0 += MU) {
#pragma unroll
          for (int u = 0; u < MU; ++u) {
            acc = mfma_slice(s0 + u, am[u], bm[u], acc);
            load_slice(s0 + MU + u, am[u], bm[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < MU - 1; ++u)  // the last nks mod MU slices (nks is uniform: scalar branches)
          if (s0 + u < nks) acc = mfma_slice(s0 + u, am[u], bm[u], acc);
      } else {  // (<2, 16>, no ring: one slice at a time, each MFMA behind its own loads)
        for (int s = 0; s < nks; ++s) {
          const int kk = 4 * s + lk;
          const double b = kk < K ? Bt[kk] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Mt[(size_t)s * 64], b, acc, 0, 0, 0);
        }
      }
      if (TQ && tw) {
        // column li = (local agent al, axis d); row = time step.  The row loop reads the very bits that are published:
        // the hand-off the partner workgroups wait for goes first, the tile writes after it.
        const int al = li / D, d = li % D;
        double* Ot = Qt + (size_t)li * RSK;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = tile * 16 + lk + 4 * q;
          if ((pub_rows >> q) & 1u)  // cells with rows only
            st_granules(A.cells + ((size_t)((int64_t)row * N + a0 + al) * D + d) * 2, tag, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = tile * 16 + lk + 4 * q;
          if (row < K) Ot[row] = acc[q];
        }
      } else {
        double* Ot = Pt + (size_t)(ct * 16 + li) * RSK;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = tile * 16 + lk + 4 * q;
          if (row < K) Ot[row] = acc[q];
        }
      }
    }
    __syncthreads();
    PSTAMP(2);
    // ---- prefix sums of p, r.p; scan path: S0 p from them, published where the cell has rows ----------------------------
    double p[D], s1p[D], s2p[D];
    {
      double rz = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        p[d] = live ? my_pt[d * RSK] : 0.0;
        rz += (live ? my_rt[d * RSK] : 0.0) * p[d];  // r of this lane, re-read from its tile
        const double cs1 = wave_incl_sum(p[d]);
        const double cs2 = lane_below(wave_incl_sum(cs1));
        s1p[d] = live ? cs1 : 0.0;
        s2p[d] = live ? cs2 : 0.0;
        if constexpr (!TQ) {
          const double qp = hh * (cs2 - 0.5 * lane_below(cs1));
          if (has_rows) {
            st_granules(my_cell + 2 * d, tag, qp);
            my_pt[d * RSK] = qp;  // the row loops read the own agent's S0 p cell here
          }
        }
      }
      rz = wave_incl_sum(rz);
      if (lane == 63) red[0][wave] = rz;  // (read after the row loop's barrier)
    }
    if constexpr (!TQ) __syncthreads();  // the own S0 p cells in Pt (TQ: in Qt since the MFMA barrier)
    PSTAMP(3);
    // ---- working rows: partner cells (polled until they carry this step's tag), eta . d(S0 p) ---------------------------
    {
      double sq = 0.0;
      unsigned spins = 0;
      bool bad = false;
      for (int e = threadIdx.x; e < ne; e += NT16) {
        const int code = e_code[e];
        const int ek = code & 63, al = (code >> 6) & 15, side = (code >> 10) & 1, par = code >> 11;
        const u64* pc = A.cells + ((size_t)((int64_t)ek * N + par) * D) * 2;
        u32x4 w[D];
        if (!wait_cell<D>(A, pc, tag, spins, w)) {
          bad = true;
          break;
        }
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) s += e_c[(size_t)e * D + d] * (Qt[(size_t)(al * D + d) * RSK + ek] - pair_value(w[d]));
        e_s[e] = s;              // (both copies of a row: the same bits, c and the difference change sign together)
        if (!side) sq += s * s;  // every row once
      }
      if (bad) raise_give_up(A, fail_s);
      sq = wave_incl_sum(sq);
      if (lane == 63) red[1][wave] = sq;
    }
    __syncthreads();
    if (fail_s) { ok = false; break; }
    PSTAMP(4);
    // ---- all-gather of the two partials of every workgroup -----------------------------------------------------------------
    // (A two-level form -- group leaders sum 16 partials, everybody polls 16 group sums: a sixteenth of the polls -- was
    // measured at 4096 x 50 and is SLOWER, 4.8 against 4.0 us: what this phase waits for is the slowest workgroup of the
    // step, not the fabric.)
    publish_partials(red, 2, 3u, gpart + (size_t)blockIdx.x * 4, tag);
    // what the fixed-row update needs and a does not change, formed while the partials are in flight: z = Pi(v)
    double zcl[D][4];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double lo[2], hi[2];
      bounds(d, lo, hi);
      zcl[d][0] = fmin(fmax(v[d][0], jlo), jhi);
      zcl[d][1] = fmin(fmax(v[d][1], alo), ahi);
      zcl[d][2] = fmin(fmax(v[d][2], lo[0]), hi[0]);
      zcl[d][3] = fmin(fmax(v[d][3], lo[1]), hi[1]);
      if (first) {  // z of a reset is A x0 itself (y = 0, v = z)
#pragma unroll
        for (int t = 0; t < 4; ++t) zcl[d][t] = v[d][t];
      }
    }
    gather_pairs<NT16>(A, gpart, 2 * nblk, tag, gp, fail_s);
    __syncthreads();
    if (fail_s) { ok = false; break; }
    PSTAMP(5);
    const double a = step_length(gp, nblk, rho_c);
    const double aa = alpha * a;
    PSTAMP(6);
    // ---- collision rows first (the certificate of the last step needs their delta-y before the lanes' chain) ----------------
    {
      const double irc = 1.0 / rho_c;
      for (int e = threadIdx.x; e < ne; e += NT16) {
        // row values at x + a p (z~) and x + alpha a p (the next x): c . (S0 x_own - S0 x_partner) + a c . (S0 p_own - ...)
        const double s = e_s[e], ax0 = e_ax[e];
        const double tc = fma(a, s, ax0), ax = fma(aa, s, ax0);
        e_ax[e] = ax;
        const double zo = e_z[e], yo = e_y[e];
        const double zh = alpha * tc + (1.0 - alpha) * zo;
        const double zn = fmax(zh + yo * irc, e_l[e]);
        const double yn = yo + rho_c * (zh - zn);
        e_z[e] = zn;
        e_y[e] = yn;
        e_g[e] = (rho_c * zn - yn) - rho_c * ax;
        if (last && with_dy) e_s[e] = fmin(yn - yo, 0.0);  // delta-y of the batch's last step (u = +inf: polar of the
                                                          // recession cone), parked until the check
      }
    }
    const bool cert = last && with_dy;
    if (cert) __syncthreads();  // (uniform: every lane of the grid takes it) the rows' delta-y are parked
    double m_ndy = 0.0, m_supp = 0.0, m_natdy = 0.0;  // delta-y of this step, reduced on the spot (certificate)
    // ---- fixed rows: z~ = F (x + a p) from the combined prefix sums, relaxation, projection, duals -----------------------
    {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double xt = fma(a, p[d], x[d]);
        const double t1 = fma(a, s1p[d], c1[d]), t2 = fma(a, s2p[d], c2[d]);
        const double xtn = lane_above(xt);
        // v' = v + alpha (F x~ - Pi(v)); the new z, y are Pi(v'), rho (v' - Pi(v'))
        const double cj = zcl[d][0], ca = zcl[d][1], cv = zcl[d][2], cp = zcl[d][3];
        const double nj = jok ? fma(alpha, (xtn - xt) * ih - cj, v[d][0]) : v[d][0];
        const double na = fma(alpha, xt - ca, v[d][1]);
        const double nv = fma(alpha, h * t1 - cv, v[d][2]);
        const double np = fma(alpha, hh * (t2 + 0.5 * t1) - cp, v[d][3]);
        if (cert) {
          // OSQP's certificate on delta-y = rho [(v' - Pi(v')) - (v - Pi(v))] of this step: |dy|, the support value
          // u.dy+ + l.dy-, and A^T dy by the r chain
          double lo[2], hi[2];
          bounds(d, lo, hi);
          const double dyj = rho * ((nj - fmin(fmax(nj, jlo), jhi)) - (v[d][0] - cj));
          const double dya = rho * ((na - fmin(fmax(na, alo), ahi)) - (v[d][1] - ca));
          const double dyv = rv * ((nv - fmin(fmax(nv, lo[0]), hi[0])) - (v[d][2] - cv));
          const double dyp = rv * ((np - fmin(fmax(np, lo[1]), hi[1])) - (v[d][3] - cp));
          m_ndy = fmax(m_ndy, fmax(fmax(fabs(dyj), fabs(dya)), fmax(fabs(dyv), fabs(dyp))));
          m_supp += (jhi * fmax(dyj, 0.0) + jlo * fmin(dyj, 0.0)) + (ahi * fmax(dya, 0.0) + alo * fmin(dya, 0.0)) +
                    (hi[0] * fmax(dyv, 0.0) + lo[0] * fmin(dyv, 0.0)) + (hi[1] * fmax(dyp, 0.0) + lo[1] * fmin(dyp, 0.0));
          double gd = 0.0;
          for (int e = c0; e < c1e; ++e) gd += e_c[(size_t)e * D + d] * e_s[e];
          const double u1 = h * dyv + 0.5 * hh * (dyp - gd);
          const double u2 = dyp + gd;
          const double d1 = wave_incl_rsum(u1);
          const double s1 = wave_incl_rsum(u2);
          const double d2 = lane_above(wave_incl_rsum(s1));
          const double vjm = lane_below(dyj);
          const double at = ((vjm - dyj) * ih + dya) + (d1 + 0.5 * hh * gd) + hh * d2;
          if (live) m_natdy = fmax(m_natdy, fabs(at));
        }
        v[d][0] = nj; v[d][1] = na; v[d][2] = nv; v[d][3] = np;
        x[d] = fma(aa, p[d], x[d]);
        c1[d] = fma(aa, s1p[d], c1[d]);
        c2[d] = fma(aa, s2p[d], c2[d]);
        __builtin_amdgcn_sched_barrier(0);  // one column at a time: interleaving both doubles the temporaries
      }
    }
    if (cert) {
      m_ndy = wave_max_nn(m_ndy);
      m_supp = wave_incl_sum(m_supp);
      m_natdy = wave_max_nn(m_natdy);
      if (lane == 63) { cert_s[0][wave] = m_ndy; cert_s[1][wave] = m_supp; cert_s[2][wave] = m_natdy; }
    }
    __syncthreads();
    PSTAMP(7);
  }

  if (!ok) break;
  it_done += nit;
  // ==== termination check (same quantities as the 8-agent kernel's; x's prefix sums are rebuilt exactly) =========================
  {
    const unsigned ctag = 0x80000000u | (A.epoch0 + steps);
    const double rv = lastk ? rho * A.rho_eq : rho;
    double m[NCHK];
#pragma unroll
    for (int j = 0; j < NCHK; ++j) m[j] = 0.0;
    {
      double gy[D];
#pragma unroll
      for (int d = 0; d < D; ++d) gy[d] = 0.0;
      for (int e = c0; e < c1e; ++e) {
        const double ye = e_y[e];
#pragma unroll
        for (int d = 0; d < D; ++d) gy[d] += e_c[(size_t)e * D + d] * ye;
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double s1 = wave_incl_sum(x[d]);
        const double s2 = lane_below(wave_incl_sum(s1));
        const double qx = hh * (s2 - 0.5 * lane_below(s1));
        c1[d] = live ? s1 : 0.0;
        c2[d] = live ? s2 : 0.0;
        if (has_rows) {
          st_granules(my_cell + 2 * d, ctag, qx);
          my_pt[d * RSK] = qx;
        }
        double lo[2], hi[2];
        bounds(d, lo, hi);
        const double xn = lane_above(x[d]);
        const double f[4] = {jok ? (xn - x[d]) * ih : 0.0, x[d], h * c1[d], hh * (c2[d] + 0.5 * c1[d])};
        const double zc[4] = {fmin(fmax(v[d][0], jlo), jhi), fmin(fmax(v[d][1], alo), ahi),
                              fmin(fmax(v[d][2], lo[0]), hi[0]), fmin(fmax(v[d][3], lo[1]), hi[1])};  // z = Pi(v)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t == 0 ? jok : live) {
            m[CK_RP] = fmax(m[CK_RP], fabs(f[t] - zc[t]));
            m[CK_NAX] = fmax(m[CK_NAX], fabs(f[t]));
            m[CK_NZ] = fmax(m[CK_NZ], fabs(zc[t]));
          }
        }
        // A^T y: the r chain with W' -> y = rho (v - Pi(v))
        const double vj = jok ? rho * (v[d][0] - zc[0]) : 0.0, va = rho * (v[d][1] - zc[1]);
        const double vv = rv * (v[d][2] - zc[2]), vp = rv * (v[d][3] - zc[3]);
        const double g = gy[d];
        const double u1 = h * vv + 0.5 * hh * (vp - g);
        const double u2 = vp + g;
        const double d1 = wave_incl_rsum(u1);
        const double r1 = wave_incl_rsum(u2);
        const double d2 = lane_above(wave_incl_rsum(r1));
        const double vjm = lane_below(vj);
        const double at = ((vjm - vj) * ih + va) + (d1 + 0.5 * hh * g) + hh * d2;
        if (live) {
          const double px = 2.0 * x[d];
          m[CK_RD] = fmax(m[CK_RD], fabs(px + at));
          m[CK_NPX] = fmax(m[CK_NPX], fabs(px));
          m[CK_NATY] = fmax(m[CK_NATY], fabs(at));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    {  // collision rows: exact S0 x cells of both agents (the carried row values are refreshed), residuals, delta-y
      unsigned spins = 0;
      bool bad = false;
      for (int e = threadIdx.x; e < ne; e += NT16) {
        const int code = e_code[e];
        const int ek = code & 63, al = (code >> 6) & 15, side = (code >> 10) & 1, par = code >> 11;
        const u64* pc = A.cells + ((size_t)((int64_t)ek * N + par) * D) * 2;
        u32x4 w[D];
        if (!wait_cell<D>(A, pc, ctag, spins, w)) {
          bad = true;
          break;
        }
        double ax = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double qq = pair_value(w[d]);
          const double qo = Pt[(size_t)(al * D + d) * RSK + ek];
          ax += e_c[(size_t)e * D + d] * (qo - qq);
        }
        e_ax[e] = ax;
        if (!side) {
          const double zc_ = e_z[e];
          m[CK_RP] = fmax(m[CK_RP], fabs(ax - zc_));
          m[CK_NAX] = fmax(m[CK_NAX], fabs(ax));
          m[CK_NZ] = fmax(m[CK_NZ], fabs(zc_));
          if (with_dy) {
            const double dd = e_s[e];
            m[CK_NDY] = fmax(m[CK_NDY], fabs(dd));
            m[CK_SUPP] += e_l[e] * dd;
          }
        }
      }
      if (bad) raise_give_up(A, fail_s);
    }
#pragma unroll
    for (int j = 0; j < NCHK; ++j) {
      double v = j == CK_SUPP ? wave_incl_sum(m[j]) : wave_max_nn(m[j]);
      if (lane == 63) {  // + the fixed rows' share of the certificate, reduced when the last step produced it
        if (j == CK_NDY) v = fmax(v, cert_s[0][wave]);
        if (j == CK_SUPP) v += cert_s[1][wave];
        if (j == CK_NATDY) v = fmax(v, cert_s[2][wave]);
        red[j][wave] = v;
      }
    }
    __syncthreads();
    if (fail_s) { ok = false; break; }
    publish_partials(red, NCHK, 1u << CK_SUPP, A.gcheck + (size_t)blockIdx.x * NCHK * 2, ctag);
    gather_pairs<NT16>(A, A.gcheck, NCHK * nblk, ctag, gck, fail_s);
    __syncthreads();
    if (fail_s) { ok = false; break; }
    double chk[NCHK];
    reduce_checks(gck, nblk, chk);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < NCHK; ++j) chk_s[j] = chk[j];
    }
    __syncthreads();  // gck may share its LDS with the r / p tiles of the next step
    if (L.gchk == L.rt) {  // ... which must be zero in the columns beyond the block again
      for (int i = threadIdx.x; i < NC16 * RSK; i += NT16) Rt[i] = 0.0;
      // (Pt: the cells of rows are rewritten by the next step before anybody reads them)
    }
    int slot;
    exit_code = check_decision(A, chk, it_done, rho, with_dy, cad, slot);
    if (exit_code) break;
    if (slot >= 0) {
      // ---- switch rho in place (what the host does between two launches: build_kkt hit + rows_value_kernel) -----------------
      const double nrs = A.tab[slot].rho;
      {  // y = rho (v - Pi(v)) must survive the switch.  EXACTLY the arithmetic of leaving (write-back: z = Pi(v), y = rho_old
         // (v - Pi(v))) and re-entering with the new rho (load: v = z + y / rho_new), so that a solver object whose cache
         // already holds the new rho's blocks (switch here) and a fresh one (exit, host builds the blocks, relaunch)
         // produce the same bits -- records of pooled and one-at-a-time solves stay identical
#pragma unroll
        for (int d = 0; d < D; ++d) {
          double lo[2], hi[2];
          bounds(d, lo, hi);
          const double zc[4] = {fmin(fmax(v[d][0], jlo), jhi), fmin(fmax(v[d][1], alo), ahi),
                                fmin(fmax(v[d][2], lo[0]), hi[0]), fmin(fmax(v[d][3], lo[1]), hi[1])};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const double rr_old = (t >= 2 && lastk) ? rho * A.rho_eq : rho, rr_new = (t >= 2 && lastk) ? nrs * A.rho_eq : nrs;
            const double yv = rr_old * (v[d][t] - zc[t]);
            v[d][t] = zc[t] + yv / rr_new;
          }
        }
      }
      rho = nrs;
      rho_c = rho * A.rho_col_scale;
      for (int i = threadIdx.x; i < tK * nks * 64; i += NT16) {
        Ml[i] = A.tab[slot].pMinv[i];
        if constexpr (TQ) Tl[i] = A.tab[slot].pT[i];
      }
      for (int e = threadIdx.x; e < ne; e += NT16)  // row values of the next right-hand side from the exact S0 x cells
        e_g[e] = (rho_c * e_z[e] - e_y[e]) - rho_c * e_ax[e];
      ++n_rho;
    }
    __syncthreads();  // Rt zeroed, operands / row values of a new rho in place
    PSTAMP(9);
  }
  }  // batches

  if (leave_if_gave_up(A, ok)) return;
  // ---- write the state back (F x and S0 x from the exact prefix sums the last check left) ------------------------------------
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double xn = lane_above(x[d]);
    const double c1b = lane_below(c1[d]);
    double lo[2], hi[2];
    bounds(d, lo, hi);
    const double f[4] = {(xn - x[d]) * ih, x[d], h * c1[d], hh * (c2[d] + 0.5 * c1[d])};
    const double zc[4] = {fmin(fmax(v[d][0], jlo), jhi), fmin(fmax(v[d][1], alo), ahi),
                          fmin(fmax(v[d][2], lo[0]), hi[0]), fmin(fmax(v[d][3], lo[1]), hi[1])};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t == 0 ? jok : live) {
        const int row = t == 0 ? k : t * K - 1 + k;
        const int64_t g = (int64_t)row * C + (int64_t)agent * D + d;
        A.zf[g] = zc[t];
        A.yf[g] = ((t >= 2 && lastk) ? rho * A.rho_eq : rho) * (v[d][t] - zc[t]);
        A.fx[g] = f[t];
      }
    }
    if (live) {
      const int64_t g = (int64_t)k * C + (int64_t)agent * D + d;
      A.x[g] = x[d];
      A.Qx[g] = hh * (c2[d] - 0.5 * c1b);
    }
  }
  const bool own_lists = A.own_lists != 0;
  const int ebase = own_lists ? 0 : A.cell_ptr[cell_of(0, a0, K)];
  for (int e = threadIdx.x; e < ne; e += NT16) {
    if (!own_lists) A.gval[ebase + e] = e_g[e];
    if (!((e_code[e] >> 10) & 1)) {
      const int n = (own_lists ? A.own_code[(size_t)blockIdx.x * cap + e] : A.ent_code[ebase + e]) >> 1;
      A.zc[n] = e_z[e];
      A.yc[n] = e_y[e];
      if (own_lists) A.grow[n] = e_g[e];  // both entries of a row hold the same bits
    }
  }
  PSTAMP(8);
#ifdef SCP_PHASE_PROFILE
  if (prof_t)
    for (int i = 0; i < 16; ++i) scp_persist16_clk[i] = i == 15 ? (unsigned long long)steps : pacc_s[i];
#endif
  publish_exit(A, chk_s, it_done, n_rho, rho, exit_code);
}

}  // namespace

#ifdef SCP_PHASE_PROFILE
// developer hook of the profiling build only (not declared in include/scp_hip.h)
extern "C" int scp_debug_persist16_clocks(unsigned long long* out, int n) {
  if (n > 16) n = 16;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(scp_persist16_clk), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif

size_t scp_persist16_entry_bytes(int D) { return (size_t)ent_doubles(D) * sizeof(double) + sizeof(int); }

size_t scp_persist16_lds_bytes(int K, int cap, int nblk, int D, int apb) {
  const Lds16 L(K, cap, nblk, D, apb);
  const size_t ints = (size_t)cap + (size_t)apb * K + 1;
  return L.n_dbl * sizeof(double) + ((ints + 1) / 2 * 2) * sizeof(int);
}

KernelFn scp_persist16_kernel(int D, int apb) {
  if (D == 2 && apb == 16) return cg1_persist16_kernel<2, 16>;
  if (D == 2 && apb == 8) return cg1_persist16_kernel<2, 8>;
  if (D == 3 && apb == 8) return cg1_persist16_kernel<3, 8>;
  return nullptr;
}
