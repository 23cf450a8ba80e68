// Holds: fixed separating half-planes that repair between-sample conflicts (scp_update_holds, scp_apply_holds;
// include/scp_hip.h has the rule, DESIGN.md section 3.7 why it is sufficient).
//
// A hold (row r = (k', q), unit vector e, margin c) replaces collision row r of the linearisation by e.(p_i[k'] - p_j[k']) >= R + c.
// The table of holds is sorted by row and has unique rows.
//
// scp_update_holds   every record of scp_list_conflicts proposes ONE (e, s) for its own row (candidate A) and for the row one
//                    time step later (candidate B).  The conflict list is sorted by row, so both candidate lists are sorted
//                    and a row has at most one candidate of each kind.  The new table is the union of three sorted lists
//                    without duplicates (old table T, A, B); an element OWNS its row if no list before it in the order T, A, B
//                    has the row, and the place of a row in the union is the number of owners below it: a binary search in T
//                    plus two prefix sums of owner flags.  Four kinds of launches: candidates + flags, the two scans (one
//                    workgroup each), the merge into a scratch table, the commit (copy + count) -- the table is read by the merge
//                    and written by the commit only, so a result that does not fit leaves it as it was.
// scp_apply_holds    flags (hold in range and its bitmap bit clear), one scan, then the writes: eta planes, l, the bit (an
//                    integer atomic: holds may share a bitmap word) and the ascending list of rows whose bit was clear.
// Everything is a function of the sorted inputs alone: no floating-point atomics, no dependence on scheduling.
#include <algorithm>

#include "scp_common.h"
#include "scp_compact_device.h"
#include "scp_pair_device.h"

namespace {

constexpr int HOLD_THREADS = CMP_THREADS;  // block_exclusive_scan's workgroup
constexpr int64_t HOLD_MAX = SCP_HOLD_MAX_TABLE;

struct HoldCand {  // what a conflict proposes for its two rows
  double eta[3];
  double s;
};

// number of conflict records with row < r (the list is sorted by row)
__device__ inline int64_t conflicts_below(const scp_conflict* __restrict__ c, int64_t n, unsigned long long r) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid].row < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ inline int64_t holds_below(const scp_hold* __restrict__ t, int64_t n, unsigned long long r) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (t[mid].row < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct HoldShape {
  int N, K, D;
  int64_t pairs, q_begin, q_end;
  // a row of the K * pairs rows whose pair lies in the range
  __device__ bool in_range(unsigned long long row) const {
    if (row >= (unsigned long long)K * (unsigned long long)pairs) return false;
    const int64_t q = (int64_t)(row % (unsigned long long)pairs);
    return q >= q_begin && q < q_end;
  }
};

// Index of the conflict that proposes candidate A / B for row r, or -1.  A: the conflict OF row r; B: the conflict of the row
// one time step earlier.  Both must pass the range filter (the same pair, so the same answer for both).
__device__ inline int64_t cand_a_of(const HoldShape& s, const scp_conflict* __restrict__ c, int64_t n, unsigned long long r) {
  if (!s.in_range(r)) return -1;
  const int64_t e = conflicts_below(c, n, r);
  return e < n && c[e].row == r ? e : -1;
}

__device__ inline int64_t cand_b_of(const HoldShape& s, const scp_conflict* __restrict__ c, int64_t n, unsigned long long r) {
  if (!s.in_range(r) || r < (unsigned long long)s.pairs) return -1;
  return cand_a_of(s, c, n, r - (unsigned long long)s.pairs);
}

// The winner of the candidates for row r: the larger shortfall, ties to the smaller conflict row (B's).  -1: no candidate
__device__ inline int64_t winner_of(const HoldCand* __restrict__ cand, int64_t ea, int64_t eb) {
  if (ea < 0) return eb;
  if (eb < 0) return ea;
  return cand[ea].s > cand[eb].s ? ea : eb;
}

// ---- update ----------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
  HoldShape s;
  double R, pad;
  const double *pos, *vel, *acc;
  const scp_conflict* conflicts;
  int64_t n_c, n_t, capacity;
  scp_hold* table;
  HoldCand* cand;        // [n_c]
  int *flag_a, *flag_b;  // [n_c] owner flags of the two candidates of a conflict ...
  int *pre_a, *pre_b;    // [n_c] ... and the owners before them (exclusive scans)
  int* totals;           // [2] owners among A, among B
  scp_hold* merged;      // [n_t + 2 n_c]
  unsigned long long* n_holds;
};

// one thread per conflict: its proposal (the rule of include/scp_hip.h, every product and sum rounded on its own) and whether
// its two candidates own their rows
__global__ __launch_bounds__(HOLD_THREADS) void hold_candidates_kernel(UpdateArgs a) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * HOLD_THREADS + threadIdx.x;
  if (e >= a.n_c) return;
  const scp_conflict c = a.conflicts[e];
  HoldCand out{{0.0, 0.0, 0.0}, 0.0};
  int fa = 0, fb = 0;
  if (a.s.in_range(c.row)) {
    const int D = a.s.D, K = a.s.K;
    const int k = (int)(c.row / (unsigned long long)a.s.pairs);
    int i, j;
    decode_pair((int64_t)(c.row % (unsigned long long)a.s.pairs), a.s.N, i, j);
    const int64_t oi = ((int64_t)i * K + k) * D, oj = ((int64_t)j * K + k) * D;
    const double t = c.t_min, ht = 0.5 * t;
    double dm[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    double nn = 0.0, ww = 0.0;
    for (int d = 0; d < D; ++d) {
      const double dp = a.pos[oi + d] - a.pos[oj + d], dv = a.vel[oi + d] - a.vel[oj + d], da = a.acc[oi + d] - a.acc[oj + d];
      const double tv = t * dv, ta = (ht * t) * da;
      dm[d] = dp + (tv + ta);
      w[d] = dv + t * da;
      nn = nn + dm[d] * dm[d];
      ww = ww + w[d] * w[d];
    }
    const double n = sqrt(nn), wn = sqrt(ww);
    if (n >= 1e-6) {
      for (int d = 0; d < D; ++d) out.eta[d] = dm[d] / n;
    } else if (wn < 1e-12) {
      out.eta[0] = 1.0;
    } else if (D == 2) {
      out.eta[0] = -w[1] / wn;
      out.eta[1] = w[0] / wn;
    } else {
      int m = 0;
      if (fabs(w[1]) < fabs(w[m])) m = 1;
      if (fabs(w[2]) < fabs(w[m])) m = 2;
      // w x e_m
      double x[3];
      x[0] = m == 0 ? 0.0 : (m == 1 ? -w[2] : w[1]);
      x[1] = m == 0 ? w[2] : (m == 1 ? 0.0 : -w[0]);
      x[2] = m == 0 ? -w[1] : (m == 1 ? w[0] : 0.0);
      double xx = 0.0;
      for (int d = 0; d < 3; ++d) xx = xx + x[d] * x[d];
      const double xn = sqrt(xx);
      for (int d = 0; d < 3; ++d) out.eta[d] = x[d] / xn;
    }
    out.s = (a.R - c.min_dist) + a.pad;
    // A owns its row unless the table has it; B (one step later, if there is such a row) unless the table or A has it
    const int64_t ta_ = holds_below(a.table, a.n_t, c.row);
    fa = !(ta_ < a.n_t && a.table[ta_].row == c.row);
    if (k + 1 < K) {
      const unsigned long long rb = c.row + (unsigned long long)a.s.pairs;
      const int64_t tb = holds_below(a.table, a.n_t, rb);
      fb = !(tb < a.n_t && a.table[tb].row == rb) && cand_a_of(a.s, a.conflicts, a.n_c, rb) < 0;
    }
  }
  a.cand[e] = out;
  a.flag_a[e] = fa;
  a.flag_b[e] = fb;
}

// ONE workgroup: out[e] = flags[0] + .. + flags[e - 1], *total = their sum (out may be flags)
__global__ __launch_bounds__(HOLD_THREADS) void hold_scan_kernel(const int* flags, int* out, int64_t n, int* total) {
  int carry = 0;
  for (int64_t base = 0; base < n; base += HOLD_THREADS) {  // uniform trip count: every thread scans every chunk
    const int64_t e = base + threadIdx.x;
    const int v = e < n ? flags[e] : 0;
    int tot;
    const int ex = block_exclusive_scan(v, &tot);
    if (e < n) out[e] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

__device__ inline scp_hold hold_from(unsigned long long row, const HoldCand& c, double margin) {
  return scp_hold{row, {c.eta[0], c.eta[1], c.eta[2]}, margin, 0ULL};
}

// one thread per element of T, A, B: an owner writes its row's record to its place in the union
__global__ __launch_bounds__(HOLD_THREADS) void hold_merge_kernel(UpdateArgs a) {
  const int64_t x = (int64_t)blockIdx.x * HOLD_THREADS + threadIdx.x;
  if (x >= a.n_t + 2 * a.n_c) return;
  if (a.n_t + a.totals[0] + a.totals[1] > a.capacity) return;  // does not fit: nothing changes
  const unsigned long long pairs = (unsigned long long)a.s.pairs;
  // owners below row r among A (conflict rows < r) and among B (conflict rows + pairs < r)
  auto a_below = [&](unsigned long long r) {
    const int64_t e = conflicts_below(a.conflicts, a.n_c, r);
    return e < a.n_c ? a.pre_a[e] : a.totals[0];
  };
  auto b_below = [&](unsigned long long r) {
    const int64_t e = r < pairs ? 0 : conflicts_below(a.conflicts, a.n_c, r - pairs);
    return e < a.n_c ? a.pre_b[e] : a.totals[1];
  };
  if (x < a.n_t) {  // an old hold: takes the winner's direction, margin old + s
    scp_hold hd = a.table[x];
    const int64_t w = winner_of(a.cand, cand_a_of(a.s, a.conflicts, a.n_c, hd.row), cand_b_of(a.s, a.conflicts, a.n_c, hd.row));
    if (w >= 0) hd = hold_from(hd.row, a.cand[w], hd.margin + a.cand[w].s);
    a.merged[x + a_below(hd.row) + b_below(hd.row)] = hd;
  } else if (x < a.n_t + a.n_c) {  // candidate A of conflict e: a new row, the winner of A and a B for the same row
    const int64_t e = x - a.n_t;
    if (!a.flag_a[e]) return;
    const unsigned long long r = a.conflicts[e].row;
    const int64_t w = winner_of(a.cand, e, cand_b_of(a.s, a.conflicts, a.n_c, r));
    a.merged[holds_below(a.table, a.n_t, r) + a.pre_a[e] + b_below(r)] = hold_from(r, a.cand[w], a.cand[w].s);
  } else {  // candidate B of conflict e: a new row nobody else proposes for
    const int64_t e = x - a.n_t - a.n_c;
    if (!a.flag_b[e]) return;
    const unsigned long long r = a.conflicts[e].row + pairs;
    a.merged[holds_below(a.table, a.n_t, r) + a_below(r) + a.pre_b[e]] = hold_from(r, a.cand[e], a.cand[e].s);
  }
}

// the merged table -> the caller's, and the count (the size needed if it does not fit)
__global__ __launch_bounds__(HOLD_THREADS) void hold_commit_kernel(UpdateArgs a) {
  const int64_t n_new = a.n_t + a.totals[0] + a.totals[1];
  const int64_t x = (int64_t)blockIdx.x * HOLD_THREADS + threadIdx.x;
  if (x == 0) *a.n_holds = (unsigned long long)n_new;
  if (n_new <= a.capacity && x < n_new) a.table[x] = a.merged[x];
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
struct ApplyArgs {
  HoldShape s;
  double h, R;
  const scp_hold* table;
  int64_t n_t, new_cap;
  const double *p0, *v0;
  double *eta, *l;
  int64_t stride;  // of an eta plane
  uint32_t* bitmap;
  int64_t* new_rows;
  int *flag, *pre;  // [n_t] hold in range with its bit clear; such holds before it
  int* total;       // their number
  unsigned long long* n_new;
};

__device__ inline int64_t hold_local_row(const HoldShape& s, unsigned long long row) {
  const int64_t k = (int64_t)(row / (unsigned long long)s.pairs), q = (int64_t)(row % (unsigned long long)s.pairs);
  return k * (s.q_end - s.q_begin) + (q - s.q_begin);
}

__global__ __launch_bounds__(HOLD_THREADS) void hold_apply_flags_kernel(ApplyArgs a) {
  const int64_t x = (int64_t)blockIdx.x * HOLD_THREADS + threadIdx.x;
  if (x >= a.n_t) return;
  const unsigned long long row = a.table[x].row;
  int f = 0;
  if (a.s.in_range(row)) {
    const int64_t lr = hold_local_row(a.s, row);
    f = !((a.bitmap[lr >> 5] >> (lr & 31)) & 1u);
  }
  a.flag[x] = f;
}

// the count for the caller (after the scan)
__global__ void hold_apply_count_kernel(ApplyArgs a) { *a.n_new = (unsigned long long)*a.total; }

// l_r = (R + c) - e.((p0_i - p0_j) + (k h)(v0_i - v0_j)): every product and every sum rounded on its own, coordinates ascending
__global__ __launch_bounds__(HOLD_THREADS) void hold_apply_write_kernel(ApplyArgs a) {
#pragma clang fp contract(off)
  const int64_t x = (int64_t)blockIdx.x * HOLD_THREADS + threadIdx.x;
  if (x >= a.n_t || (int64_t)*a.total > a.new_cap) return;  // the list does not fit: nothing is written at all
  const scp_hold hd = a.table[x];
  if (!a.s.in_range(hd.row)) return;
  const int D = a.s.D;
  const int k = (int)(hd.row / (unsigned long long)a.s.pairs);
  int i, j;
  decode_pair((int64_t)(hd.row % (unsigned long long)a.s.pairs), a.s.N, i, j);
  const double kh = (double)k * a.h;
  double dot = 0.0;
  for (int d = 0; d < D; ++d) {
    const double dp = a.p0[(int64_t)i * D + d] - a.p0[(int64_t)j * D + d], dv = a.v0[(int64_t)i * D + d] - a.v0[(int64_t)j * D + d];
    const double c = dp + kh * dv;
    dot = dot + hd.eta[d] * c;
  }
  const int64_t lr = hold_local_row(a.s, hd.row);
  for (int d = 0; d < D; ++d) a.eta[d * a.stride + lr] = hd.eta[d];
  a.l[lr] = (a.R + hd.margin) - dot;
  atomicOr(a.bitmap + (lr >> 5), 1u << (lr & 31));
  if (a.flag[x]) a.new_rows[a.pre[x]] = (int64_t)hd.row;
}

// a device count to the host (drains the ctx stream)
int hold_read_count(scp_ctx* ctx, const uint64_t* dev, uint64_t* out) {
  SCP_HIP_CHECK(ctx, hipMemcpyAsync(out, dev, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return SCP_OK;
}

int hold_end(scp_ctx* ctx) {  // after the call's last launch: launch errors, the end of the timing bracket
  SCP_HIP_CHECK(ctx, hipGetLastError());
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev1, ctx->stream));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  return SCP_OK;
}

inline size_t hold_align(size_t b) { return (b + 63) & ~(size_t)63; }

}  // namespace

extern "C" int scp_update_holds(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                                const double* pos, const double* vel, const double* acc, const scp_conflict* conflicts,
                                const uint64_t* n_conflicts, double pad, scp_hold* table, int64_t capacity, uint64_t* n_holds) {
  if (!ctx) return SCP_ERR_INVALID;
  int rc = scp_check_pair_range(ctx, N, K, D, q_begin, q_end);
  if (rc) return rc;
  SCP_REQUIRE(ctx, pos && vel && acc && n_conflicts && n_holds, "update_holds: null pointer");
  SCP_REQUIRE(ctx, h > 0.0 && h < __builtin_huge_val(), "update_holds: bad time step h=%g", h);
  SCP_REQUIRE(ctx, pad >= 0.0 && pad < __builtin_huge_val(), "update_holds: bad pad %g", pad);
  SCP_REQUIRE(ctx, capacity >= 0, "update_holds: bad capacity %lld", (long long)capacity);
  SCP_REQUIRE(ctx, table || capacity == 0, "update_holds: null table of capacity %lld", (long long)capacity);
  if (capacity > HOLD_MAX) return scp_fail(ctx, SCP_ERR_CAPACITY, "update_holds: capacity %lld exceeds the largest table %lld",
                                           (long long)capacity, (long long)HOLD_MAX);
  uint64_t n_c = 0, n_t = 0;
  if ((rc = hold_read_count(ctx, n_conflicts, &n_c)) || (rc = hold_read_count(ctx, n_holds, &n_t))) return rc;
  SCP_REQUIRE(ctx, n_t <= (uint64_t)capacity, "update_holds: %llu holds in a table of capacity %lld", (unsigned long long)n_t,
              (long long)capacity);
  SCP_REQUIRE(ctx, conflicts || n_c == 0, "update_holds: null conflict list");
  if (n_c > (uint64_t)HOLD_MAX) return scp_fail(ctx, SCP_ERR_CAPACITY, "update_holds: %llu conflicts exceed the largest table %lld",
                                                (unsigned long long)n_c, (long long)HOLD_MAX);
  const size_t b_cand = hold_align(n_c * sizeof(HoldCand)), b_int = hold_align(n_c * sizeof(int));
  const size_t b_merged = hold_align((n_t + 2 * n_c) * sizeof(scp_hold));
  rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, b_cand + 4 * b_int + 64 + b_merged);
  if (rc) return rc;
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  if (n_c > 0 && scp_pairs(N) > 0) {
    char* w = (char*)ctx->sep_ws;
    UpdateArgs a{};
    a.s = HoldShape{N, K, D, scp_pairs(N), q_begin, q_end};
    a.R = R; a.pad = pad;
    a.pos = pos; a.vel = vel; a.acc = acc;
    a.conflicts = conflicts;
    a.n_c = (int64_t)n_c; a.n_t = (int64_t)n_t; a.capacity = capacity;
    a.table = table;
    a.cand = (HoldCand*)w; w += b_cand;
    a.flag_a = (int*)w; w += b_int;
    a.flag_b = (int*)w; w += b_int;
    a.pre_a = (int*)w; w += b_int;
    a.pre_b = (int*)w; w += b_int;
    a.totals = (int*)w; w += 64;
    a.merged = (scp_hold*)w;
    a.n_holds = (unsigned long long*)n_holds;
    const dim3 block(HOLD_THREADS), per_conflict((unsigned)scp_cdiv(a.n_c, HOLD_THREADS)),
        per_element((unsigned)scp_cdiv(a.n_t + 2 * a.n_c, HOLD_THREADS));
    hipLaunchKernelGGL(hold_candidates_kernel, per_conflict, block, 0, ctx->stream, a);
    hipLaunchKernelGGL(hold_scan_kernel, dim3(1), block, 0, ctx->stream, a.flag_a, a.pre_a, a.n_c, a.totals);
    hipLaunchKernelGGL(hold_scan_kernel, dim3(1), block, 0, ctx->stream, a.flag_b, a.pre_b, a.n_c, a.totals + 1);
    hipLaunchKernelGGL(hold_merge_kernel, per_element, block, 0, ctx->stream, a);
    hipLaunchKernelGGL(hold_commit_kernel, per_element, block, 0, ctx->stream, a);
  }
  return hold_end(ctx);
}

extern "C" int scp_apply_holds(scp_ctx* ctx, int N, int K, int D, double h, double R, int64_t q_begin, int64_t q_end,
                               const scp_hold* table, const uint64_t* n_holds, const double* p0, const double* v0, double* eta,
                               double* l, uint32_t* sel_bitmap, int64_t* new_rows, int64_t new_cap, uint64_t* n_new) {
  if (!ctx) return SCP_ERR_INVALID;
  int rc = scp_check_pair_range(ctx, N, K, D, q_begin, q_end);
  if (rc) return rc;
  SCP_REQUIRE(ctx, n_holds && p0 && v0 && eta && l && sel_bitmap && n_new, "apply_holds: null pointer");
  SCP_REQUIRE(ctx, h > 0.0 && h < __builtin_huge_val(), "apply_holds: bad time step h=%g", h);
  SCP_REQUIRE(ctx, new_cap >= 0 && (new_rows || new_cap == 0), "apply_holds: bad row list (capacity %lld)", (long long)new_cap);
  uint64_t n_t = 0;
  if ((rc = hold_read_count(ctx, n_holds, &n_t))) return rc;
  SCP_REQUIRE(ctx, table || n_t == 0, "apply_holds: null table");
  if (n_t > (uint64_t)HOLD_MAX) return scp_fail(ctx, SCP_ERR_CAPACITY, "apply_holds: %llu holds exceed the largest table %lld",
                                                (unsigned long long)n_t, (long long)HOLD_MAX);
  const size_t b_int = hold_align(n_t * sizeof(int));
  rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, 2 * b_int + 64);
  if (rc) return rc;
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  char* w = (char*)ctx->sep_ws;
  ApplyArgs a{};
  a.s = HoldShape{N, K, D, scp_pairs(N), q_begin, q_end};
  a.h = h; a.R = R;
  a.table = table;
  a.n_t = scp_pairs(N) > 0 ? (int64_t)n_t : 0;
  a.new_cap = new_cap;
  a.p0 = p0; a.v0 = v0; a.eta = eta; a.l = l;
  a.stride = scp_eta_stride(K, q_end - q_begin);
  a.bitmap = sel_bitmap;
  a.new_rows = new_rows;
  a.flag = (int*)w; w += b_int;
  a.pre = (int*)w; w += b_int;
  a.total = (int*)w;
  a.n_new = (unsigned long long*)n_new;
  const dim3 block(HOLD_THREADS), per_hold((unsigned)std::max(scp_cdiv(a.n_t, HOLD_THREADS), 1));
  hipLaunchKernelGGL(hold_apply_flags_kernel, per_hold, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(hold_scan_kernel, dim3(1), block, 0, ctx->stream, a.flag, a.pre, a.n_t, a.total);
  hipLaunchKernelGGL(hold_apply_count_kernel, dim3(1), dim3(1), 0, ctx->stream, a);
  hipLaunchKernelGGL(hold_apply_write_kernel, per_hold, block, 0, ctx->stream, a);
  return hold_end(ctx);
}
