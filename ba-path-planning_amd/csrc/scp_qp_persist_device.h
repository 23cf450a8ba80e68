// Shared by the persistent ADMM kernels (scp_qp_persist.hip: one wave per agent, 8 / 4 agents per workgroup;
// scp_qp_persist16.hip: the lean 16-agent form): launch arguments, exit codes, the tagged-granule primitives of the two
// cross-workgroup exchanges, and the protocol both kernels run on them -- bounded polls, all-gathers, the collective give-up,
// the decision after a check and what the host reads at the exit.  gfx950 only.
#pragma once
#include "scp_qp_device.h"

// The hand-offs rely on gfx9 memory semantics: sc1 stores write through to the agent-coherent level, and the asm loads wait
// for their own data with s_waitcnt vmcnt(0).  Neither is checked for another target.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "scp_qp_persist_device.h: the persistent ADMM kernels' hand-offs are written for gfx950 only"
#endif

namespace scp_persist {
using namespace scpdev;

typedef unsigned long long u64;
constexpr unsigned SPIN_LIMIT = 1u << 20;

struct PersistArgs {
  int K, N, nblk, ent_cap;
  int it0, max_iter, check_every, rho_interval;  // iterations done so far in this solve; limits; termination / rho periods
  int cad0, check_fine;    // adaptive check cadence (scp_qp_settings.check_fine): steps between checks when this launch starts
  double fine_ratio;       // (the host's decision after the previous check), the fine period, and "close" = residuals < ratio x tolerance
  int64_t C;
  double rho, rho_c, rho_eq, alpha, h;
  double eps_abs, eps_rel, eps_prim_inf, rho_tol;  // termination tests (eps_prim_inf <= 0: no certificate; rho_tol <= 0: fixed rho)
  // lean kernel: the bounds of the jerk / acceleration rows (the same for every row), and what the velocity / position
  // bounds are made of (scp_qp_set_problem keeps a copy of the four state arrays: [4][N][D] = p0, v0, pf, vf)
  double jerk_lo, jerk_hi, acc_lo, acc_hi, vel_lo, vel_hi, pmin[3], pmax[3];
  const double* states;
  int first_step;  // lean kernels: this launch starts with the first ADMM step after scp_qp_reset (z = A x0 unprojected, y = 0)
  int spin_sleep;  // naps (64 clocks each) between two polls of a granule that has not arrived (1; more when many persistent
                   // launches share the chip: their polls load the fabric the hand-offs travel on)
  const double* pMinv;
  const double* pT;      // packed T = S0 H_f^{-1}
  const double *lf, *uf;
  double *zf, *yf, *fx, *x, *Qx, *dyf;
  u64* cells;       // [K][N][D][2] granules: S0 p of (time step, agent), low / high word, each tagged with the step
  u64* gpart;       // [2 parities][nblk][4] granules: r.p and sum (eta . d S0 p)^2 of one workgroup
  u64* gcheck;      // [nblk][18] granules: the nine partial results of a termination check of one workgroup
  unsigned* give_up;
  const int *cell_ptr, *ent_code, *w_k, *w_i, *w_j;
  const double *w_eta, *w_l;
  double *zc, *yc, *dyc, *gval;
  // Where the entry tables come from.  own_lists = 0: the host built the incidence lists and the row values (cell_ptr,
  // ent_code, gval: the small install's single launch, or the "persist_host_lists" hook) and the kernel copies its slice.
  // own_lists = 1: every workgroup derives its slice from the nW raw rows (build_entry_tables) and forms the row values
  // from the S0 x cells it loads anyway -- or, vals_carried, takes the values an earlier launch of this solve left per
  // row in `grow` -- and cell_ptr / ent_code / gval are neither read nor written.
  int nW, own_lists, vals_carried;
  int* own_code;  // [SCP_PERSIST_MAX_WG + 1][ent_cap]: the sorted codes 2 n + side of each workgroup, written at entry and read
                  // again by the same workgroup at the exit (the lean kernels keep no row index in LDS)
  double* grow;   // [nW] the row values at the exit, per row (from the side-0 entry)
  unsigned* host_status;  // mapped host words: [0] exit code (EXIT_*), [1] ADMM iterations done when the kernel left
  double* host_scal;      // mapped host array: the nine check results in the SL_* slots of scp_qp::h_scal
  u64* host_flag;         // mapped completion word, set to `seq` last
  u64 seq;
  unsigned epoch0;        // steps completed by earlier launches (tags never repeat; the buffers start zeroed)
  // adaptive rho inside the kernel: the rho values whose blocks the host has cached (scp_qp::kkt).  When a check asks for a
  // new rho that is in this table the kernel switches by itself (operands reloaded, row values recomputed) and goes on;
  // otherwise it returns EXIT_RHO and the host builds the blocks.  host_status[2] = switches made, *host_rho = rho at exit.
  double rho_col_scale;
  double* host_rho;
  int n_tab;
  struct RhoSlot {
    double rho;
    const double* pMinv;
    const double* pT;
  } tab[SCP_KKT_SLOTS_MAX];
};

typedef void (*KernelFn)(PersistArgs);  // a persistent kernel, launched one workgroup per CU

// why the kernel returned (host_status[0]); the host re-derives every decision from the nine check results
enum { EXIT_SOLVED = 1, EXIT_GAVE_UP = 2, EXIT_MAX_ITER = 3, EXIT_INFEASIBLE = 4, EXIT_RHO = 5, EXIT_OVERFLOW = 6 };
constexpr int NCHK = 9;  // rp, |Ax|, |z|, rd, |Px|, |A^T y|, |dy|, supp (a sum), |A^T dy|  (maxima of non-negative values)
constexpr int CK_RP = 0, CK_NAX = 1, CK_NZ = 2, CK_RD = 3, CK_NPX = 4, CK_NATY = 5, CK_NDY = 6, CK_SUPP = 7, CK_NATDY = 8;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// One double = one 16-byte pair of granules {low word, tag, high word, tag}: ONE write-through store, ONE load (a scalar
// sc1 store is one fabric write whatever its width: 8-byte stores doubled the hand-off's fabric traffic).  Each 8-byte
// half carries its own tag, so a torn pair is detected like a late one.  Inline asm because the builtins offer no 16-byte
// agent-scope access; the asm loads wait for their own data (the compiler does not count them).  The store ends with the
// wait state a 16-byte store needs before a VALU may overwrite its data registers: the compiler pads its own stores, not
// an asm one, and without it the next instruction can change the low word before the store has read it.
__device__ inline void st_granules(u64* g, unsigned tag, double v) {
  const u32x4 w = {(unsigned)__double2loint(v), tag, (unsigned)__double2hiint(v), tag};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(g), "v"(w) : "memory");
}
__device__ inline u32x4 ld_pair(const u64* g) {
  u32x4 w;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(w) : "v"(g) : "memory");
  return w;
}
template <int D>
__device__ inline void ld_cell(const u64* g, u32x4 (&w)[D]) {  // the D doubles of one cell: D loads in flight, one wait
  if (D == 2) {
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1])
                 : "v"(g)
                 : "memory");
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) w[d] = ld_pair(g + 2 * d);
  }
}
__device__ inline void spin_nap(int n) {
  for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1);
}
__device__ inline bool pair_ok(const u32x4& w, unsigned tag) { return w[1] == tag && w[3] == tag; }
__device__ inline double pair_value(const u32x4& w) { return __hiloint2double((int)w[2], (int)w[0]); }

// ---- the exchange protocol of both kernels --------------------------------------------------------------------------------
// Every spin is bounded: a workgroup that times out raises the give-up word, every workgroup then leaves WITHOUT writing
// state back (leave_if_gave_up), and the host repeats the iterations on the three-launch pipeline.

// Bounded wait for the D granule pairs of one cell (D = 1: one pair) to carry `tag`.  `spins` counts on across the calls
// of one exchange.  False: the spin budget is spent, or another workgroup has given up (its word is read every 256
// spins) -- the caller stops polling and raises the word itself (raise_give_up).
template <int D>
__device__ __forceinline__ bool wait_cell(const PersistArgs& A, const u64* g, unsigned tag, unsigned& spins, u32x4 (&w)[D]) {
  for (;;) {
    ld_cell<D>(g, w);
    bool here = true;
#pragma unroll
    for (int d = 0; d < D; ++d) here = here && pair_ok(w[d], tag);
    if (here) return true;
    if (++spins > SPIN_LIMIT ||
        ((spins & 255u) == 0u && __hip_atomic_load(A.give_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u))
      return false;
    spin_nap(A.spin_sleep);
  }
}

// after a wait that failed: tell every other workgroup, and this one (fail_s, read after the next barrier)
__device__ __forceinline__ void raise_give_up(const PersistArgs& A, int& fail_s) {
  __hip_atomic_store(A.give_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  fail_s = 1;
}

// Thread j < n publishes this workgroup's partial j, reduced over its APB waves (red[j][wave]) in a fixed order: a sum where
// bit j of sum_mask is set, else a maximum of non-negative values.  Partial j goes to the granule pair at dst + 2 j.
template <int APB>
__device__ __forceinline__ void publish_partials(const double (&red)[NCHK][APB], int n, unsigned sum_mask, u64* dst,
                                                 unsigned tag) {
  if (threadIdx.x < n) {
    const int j = threadIdx.x;
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < APB; ++w) t = (sum_mask >> j) & 1u ? t + red[j][w] : fmax(t, red[j][w]);
    st_granules(dst + 2 * j, tag, t);
  }
}

// All-gather: the n doubles at buf (n granule pairs, every workgroup's partials) into out[0, n), one double per thread
// and pass.  A wait that fails raises the give-up word; the caller reads fail_s after its barrier.
template <int NT>
__device__ __forceinline__ void gather_pairs(const PersistArgs& A, const u64* buf, int n, unsigned tag, double* out,
                                             int& fail_s) {
  unsigned spins = 0;
  bool bad = false;
  for (int q = threadIdx.x; q < n; q += NT) {
    u32x4 w[1];
    if (!wait_cell<1>(A, buf + 2 * q, tag, spins, w)) {
      bad = true;
      break;
    }
    out[q] = pair_value(w[0]);
  }
  if (bad) raise_give_up(A, fail_s);
}

// The step length of the exact line search, a = r.p / (r.p + rho_c sum (eta . d S0 p)^2), from the gathered partials
// (gp: [nblk][2]).  Every wave sums them in the same order: the same bits everywhere, no further barrier.
__device__ __forceinline__ double step_length(const double* gp, int nblk, double rho_c) {
  double vr = 0.0, vs = 0.0;
  for (int b = threadIdx.x & 63; b < nblk; b += 64) {
    vr += gp[2 * b];
    vs += gp[2 * b + 1];
  }
  const double rzt = read_lane(wave_incl_sum(vr), 63);
  const double sqt = read_lane(wave_incl_sum(vs), 63);
  const double pHp = rzt + rho_c * sqt;
  return (pHp > 0.0 && rzt != 0.0) ? rzt / pHp : 0.0;
}

// The nine results of a termination check from the gathered partials (gck: [nblk][NCHK]), in the same reduction order in
// every wave of every workgroup: identical decisions everywhere.
__device__ __forceinline__ void reduce_checks(const double* gck, int nblk, double (&chk)[NCHK]) {
#pragma unroll
  for (int j = 0; j < NCHK; ++j) {
    double v = 0.0;
    for (int b = threadIdx.x & 63; b < nblk; b += 64) v = j == CK_SUPP ? v + gck[b * NCHK + j] : fmax(v, gck[b * NCHK + j]);
    chk[j] = read_lane(j == CK_SUPP ? wave_incl_sum(v) : wave_max_nn(v), 63);
  }
}

// The decision after a check (the host repeats these tests on the same nine numbers, scp_qp_solve): the exit code, or 0 to
// go on.  Sets the cadence of the next batch and `slot`: the entry of A.tab whose rho the kernel switches to in place
// before it goes on, or -1.
__device__ __forceinline__ unsigned check_decision(const PersistArgs& A, const double (&chk)[NCHK], int it_done, double rho,
                                                   bool with_dy, int& cad, int& slot) {
  slot = -1;
  const double np_ = fmax(chk[CK_NAX], chk[CK_NZ]), nd_ = fmax(chk[CK_NPX], chk[CK_NATY]);
  const double tol_p = A.eps_abs + A.eps_rel * np_, tol_d = A.eps_abs + A.eps_rel * nd_;
  if (chk[CK_RP] <= tol_p && chk[CK_RD] <= tol_d) return EXIT_SOLVED;
  if (A.check_fine > 0)  // (the same decision as scp_qp_solve's, from the same nine numbers)
    cad = (chk[CK_RP] < A.fine_ratio * tol_p && chk[CK_RD] < A.fine_ratio * tol_d) ? A.check_fine : A.check_every;
  if (it_done >= A.max_iter) return EXIT_MAX_ITER;
  if (with_dy && chk[CK_NDY] > A.eps_prim_inf && chk[CK_SUPP] < -A.eps_prim_inf * chk[CK_NDY] &&
      chk[CK_NATDY] < A.eps_prim_inf * chk[CK_NDY])
    return EXIT_INFEASIBLE;
  if (A.rho_tol > 0.0 && it_done % A.rho_interval == 0) {
    // OSQP's rho estimate, snapped to the 2^(1/4) grid as the host does it (scp_qp_solve).  Device log2 / exp2 may differ
    // from the host's in the last bit, so the candidate only SELECTS: the value that counts is the host-computed double
    // in the table of cached rho, and the threshold test is repeated on it exactly as the host would.
    const double prim = chk[CK_RP] / fmax(np_, 1e-10), dual = chk[CK_RD] / fmax(nd_, 1e-10);
    const double nr = fmin(fmax(rho * sqrt(prim / fmax(dual, 1e-10)), 1e-6), 1e6);
    const double cand = exp2(round(4.0 * log2(nr)) * 0.25);
    if (cand > rho * A.rho_tol * (1.0 - 1e-9) || cand < rho / A.rho_tol * (1.0 + 1e-9)) {  // (else: clearly no update)
      int s = -1;
      for (int i = 0; i < A.n_tab; ++i)
        if (fabs(A.tab[i].rho - cand) <= 1e-12 * cand) s = i;
      if (s < 0) return EXIT_RHO;  // not cached yet: the host builds the blocks and relaunches
      const double nrs = A.tab[s].rho;
      if (nrs > rho * A.rho_tol || nrs < rho / A.rho_tol) {
        slot = s;
        if (A.check_fine > 0) cad = A.check_fine;
      }
    }
  }
  return 0;
}

// More incident rows around some block of APB agents than the LDS tables hold: EVERY workgroup finds that out by itself
// (the largest block's count) and leaves before anything is published -- nobody spins on anybody.  `over`: this thread
// saw a block beyond the capacity.  True: the caller returns at once.
__device__ __forceinline__ bool leave_on_overflow(const PersistArgs& A, bool over) {
  if (!__syncthreads_or(over)) return false;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(A.host_status, (unsigned)EXIT_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_flag, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  return true;
}
// ... from the host-built lists: a few loads of cell_ptr
template <int APB>
__device__ __forceinline__ bool entries_overflow(const PersistArgs& A) {
  int worst = 0;
  for (int b = threadIdx.x; b < (A.N + APB - 1) / APB; b += 64 * APB) {
    const int b0 = b * APB, b1 = min(b0 + APB, A.N);
    worst = max(worst, A.cell_ptr[cell_of(0, b1, A.K)] - A.cell_ptr[cell_of(0, b0, A.K)]);
  }
  return leave_on_overflow(A, worst > A.ent_cap);
}

// The entry tables of the block of agents [a0, a1) straight from the raw working rows (PersistArgs::own_lists), with no
// word exchanged between workgroups: the same block-relative cell offsets (cptr[(a1 - a0) K + 1]) and the same codes
// 2 n + side in the same order as the slice of the global build (scp_qp_csr_ensure: cells in cell_of order, ascending
// code inside a cell), and the entry count of EVERY block of the grid, so that the overflow decision is the one every
// other workgroup takes.  One pass over the nW rows (four rows in flight per thread): LDS atomic counts per block of the
// grid and per own cell, the own hits appended unsorted; then, in LDS only, a scan of the cell counts (one wave), the
// scatter into cell order and an insertion sort per cell.  Integer counts do not depend on the order of the atomics, and
// the sort fixes the order inside a cell.  Temporaries, all free until the column state is loaded: hits [2 cap] (code,
// cell), cur [(a1 - a0) K] fill cursors, blk_cnt [blocks of the grid].  Every loop is bounded by nW, the cell count or the
// block's entry count.  Returns the block's entry count, or -1: some block overflows the tables, the caller returns.
template <int APB, int NT>
__device__ __forceinline__ int build_entry_tables(const PersistArgs& A, int a0, int a1, int* cptr, int* codes, int* hits,
                                                  int* cur, int* blk_cnt) {
  static_assert(APB <= 16 && (APB & (APB - 1)) == 0, "one wave scans 64 x 16 cells; blocks by shift");
  const int K = A.K, nW = A.nW, cap = A.ent_cap, tid = threadIdx.x, me = blockIdx.x;
  const int nb = (A.N + APB - 1) / APB, ncell = (a1 - a0) * K;
  for (int i = tid; i <= ncell; i += NT) cptr[i] = 0;  // entry counts of the own cells first, offsets after the scan
  for (int i = tid; i < ncell; i += NT) cur[i] = 0;
  for (int i = tid; i < nb; i += NT) blk_cnt[i] = 0;
  __syncthreads();
  constexpr int U = 4;
  for (int n0 = tid; n0 < nW; n0 += U * NT) {
    int w[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = n0 + u * NT;
      w[u][0] = n < nW ? A.w_i[n] : -1;
      w[u][1] = n < nW ? A.w_j[n] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = n0 + u * NT;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int ag = w[u][side];
        if (ag < 0) continue;
        if (ag / APB != me) {
          atomicAdd(&blk_cnt[ag / APB], 1);
        } else {
          const int at = atomicAdd(&blk_cnt[me], 1);
          const int cell = (ag - a0) * K + A.w_k[n];
          atomicAdd(&cptr[cell], 1);
          if (at < cap) {  // (beyond: every workgroup leaves below)
            hits[2 * at] = 2 * n + side;
            hits[2 * at + 1] = cell;
          }
        }
      }
    }
  }
  __syncthreads();
  int worst = 0;
  for (int b = tid; b < nb; b += NT) worst = max(worst, blk_cnt[b]);
  if (leave_on_overflow(A, worst > cap)) return -1;
  const int ne = blk_cnt[me];
  if (tid < 64) {  // exclusive scan of the cell counts: 16 consecutive cells per lane (at most 16 agents x 64 time steps)
    constexpr int SC = 16;
    int v[SC], tot = 0;
#pragma unroll
    for (int e = 0; e < SC; ++e) {
      v[e] = SC * tid + e < ncell ? cptr[SC * tid + e] : 0;
      tot += v[e];
    }
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (tid >= o) incl += t;
    }
    int run = incl - tot;
#pragma unroll
    for (int e = 0; e < SC; ++e) {
      if (SC * tid + e < ncell) cptr[SC * tid + e] = run;
      run += v[e];
    }
    if (tid == 63) cptr[ncell] = run;
  }
  __syncthreads();
  for (int t = tid; t < ne; t += NT) {
    const int cell = hits[2 * t + 1];
    codes[cptr[cell] + atomicAdd(&cur[cell], 1)] = hits[2 * t];
  }
  __syncthreads();
  for (int c = tid; c < ncell; c += NT) {  // ascending code inside every cell, as csr_sort_kernel leaves it
    const int b = cptr[c], e = cptr[c + 1];
    for (int i = b + 1; i < e; ++i) {
      const int v = codes[i];
      int j = i - 1;
      while (j >= b && codes[j] > v) {
        codes[j + 1] = codes[j];
        --j;
      }
      codes[j + 1] = v;
    }
  }
  __syncthreads();
  return ne;
}

// The first row value of the single-step pipeline, g = (rho_c z_c - y_c) - rho_c ax with ax = c . (S0 x_own - S0 x_partner)
// summed from 0 in axis order: the two fused multiply-adds rows_value_kernel<D, true> compiles to, spelled out so that the
// bits do not hang on how this translation unit is contracted.
__device__ __forceinline__ double first_row_value(double rho_c, double zc, double yc, double ax) {
  return __builtin_fma(-rho_c, ax, __builtin_fma(rho_c, zc, -yc));
}

// The exit decision is collective: a workgroup that timed out has raised the give-up word BEFORE the cell or partial it
// was waiting for appeared, so every workgroup that got past that exchange afterwards sees the word here and leaves
// without writing back as well (the host additionally drops its carried-state flags on a give-up).  True: the caller
// returns at once -- nothing was written back, the state in global memory is the state before this launch.
__device__ __forceinline__ bool leave_if_gave_up(const PersistArgs& A, bool ok) {
  if (ok && __syncthreads_or(threadIdx.x == 0 &&
                             __hip_atomic_load(A.give_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u))
    ok = false;
  if (ok) return false;
  if (threadIdx.x == 0) {
    __hip_atomic_store(A.host_status, (unsigned)EXIT_GAVE_UP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_flag, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  return true;
}

// After the write-back: the nine check results in the slots the host reads (scp_qp::h_scal), the iteration count, the
// rho switches and rho, then the exit code and, last, the completion word.
__device__ __forceinline__ void publish_exit(const PersistArgs& A, const double* chk, int it_done, unsigned n_rho, double rho,
                                             unsigned exit_code) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int slot[NCHK] = {SL_RP, SL_NAX, SL_NZ, SL_RD, SL_NPX, SL_NATY, SL_NDY, SL_SUPP, SL_NATDY};
#pragma unroll
    for (int j = 0; j < NCHK; ++j)
      __hip_atomic_store((u64*)(A.host_scal + slot[j]), (u64)__double_as_longlong(chk[j]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_status + 1, (unsigned)it_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_status + 2, n_rho, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((u64*)A.host_rho, (u64)__double_as_longlong(rho), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_status, exit_code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.host_flag, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace scp_persist

// host side of the lean kernel (scp_qp_persist16.hip), called by scp_qp_cg1_persist
size_t scp_persist16_lds_bytes(int K, int cap, int nblk, int D, int apb);
size_t scp_persist16_entry_bytes(int D);  // LDS per incident row (entry tables + its code)
scp_persist::KernelFn scp_persist16_kernel(int D, int apb);  // cg1_persist16_kernel<D, apb>, or null: no such instantiation
