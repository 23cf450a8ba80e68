// Static obstacles on gfx950: the summed table of an occupancy grid, safe-flight-corridor boxes around a reference path,
// the boxes of the states in metres, their way into the bounds of the joint QP, and the continuous-time check that every
// segment stays inside its box.  The rules are stated in include/scp_hip.h ("static obstacles"); tests/corridor_ref.py is
// their numpy restatement (integers exactly, doubles bit for bit: no contraction anywhere in this file).
#include "scp_common.h"
#include "scp_corridor_device.h"

#include <cmath>

namespace {

constexpr int64_t CORRIDOR_MAX_CELLS = (int64_t)1 << 24;
constexpr int CORRIDOR_MAX_GROW = 1024;

// ----------------------------------------------------------------------------------------------------
// the summed table: one launch per dimension, in place after the first
// ----------------------------------------------------------------------------------------------------
// along x: one wave per row (y, z), 64 cells per trip, the running count carried from trip to trip
__global__ __launch_bounds__(256) void sat_rows_kernel(int nx, int64_t rows, const uint8_t* __restrict__ occ,
                                                        int32_t* __restrict__ sat) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  const uint8_t* src = occ + row * nx;
  int32_t* dst = sat + row * nx;
  int carry = 0;
  for (int base = 0; base < nx; base += 64) {
    const int x = base + lane;
    int v = (x < nx && src[x] != 0) ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(v, o);
      if (lane >= o) v += up;
    }
    if (x < nx) dst[x] = carry + v;
    carry += __shfl(v, 63);
  }
}

// along y (stride = nx, count = ny, lines = (x, z)) and along z (stride = nx ny, count = nz, lines = (x, y)): one thread
// walks a line, neighbouring threads neighbouring x
__global__ __launch_bounds__(256) void sat_lines_kernel(int64_t lines, int inner, int64_t outer_stride, int count,
                                                         int64_t stride, int32_t* __restrict__ sat) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= lines) return;
  int32_t* p = sat + (t / inner) * outer_stride + (t % inner);
  int run = 0;
  for (int n = 0; n < count; ++n) {
    run += p[(int64_t)n * stride];
    p[(int64_t)n * stride] = run;
  }
}

// ----------------------------------------------------------------------------------------------------
// corridor boxes: one thread per (vehicle, segment)
// ----------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void corridor_boxes_kernel(int64_t n_seg, int K, CorridorGrid g,
                                                              const int32_t* __restrict__ sat,
                                                              const double* __restrict__ ref, int max_grow,
                                                              int32_t* __restrict__ cells,
                                                              unsigned long long* __restrict__ n_blocked) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool blocked = false;
  if (t < n_seg) {
    const int64_t i = t / K;
    const int gseg = (int)(t % K);
    const double* r0 = ref + (i * (K + 1) + gseg) * D;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < D; ++d) {
      int c0 = 0, c1 = 0;
      const bool in0 = cell_of(g, d, r0[d], c0), in1 = cell_of(g, d, r0[D + d], c1);
      if (!(in0 && in1)) blocked = true;
      lo[d] = c0 < c1 ? c0 : c1;
      hi[d] = c0 < c1 ? c1 : c0;
    }
    if (!blocked && occupied_in<D>(sat, g, lo, hi) != 0) blocked = true;
    if (!blocked) {
      int seed_lo[3], seed_hi[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        seed_lo[d] = lo[d];
        seed_hi[d] = hi[d];
      }
      const int max_sweeps = 2 * D * max_grow + 1;
      for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        bool grew = false;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          if (seed_lo[d] - lo[d] < max_grow && lo[d] - 1 >= 0) {  // direction -d
            int a[3] = {lo[0], lo[1], lo[2]}, b[3] = {hi[0], hi[1], hi[2]};
            a[d] = b[d] = lo[d] - 1;
            if (occupied_in<D>(sat, g, a, b) == 0) {
              lo[d] -= 1;
              grew = true;
            }
          }
          if (hi[d] - seed_hi[d] < max_grow && hi[d] + 1 < g.dims[d]) {  // direction +d
            int a[3] = {lo[0], lo[1], lo[2]}, b[3] = {hi[0], hi[1], hi[2]};
            a[d] = b[d] = hi[d] + 1;
            if (occupied_in<D>(sat, g, a, b) == 0) {
              hi[d] += 1;
              grew = true;
            }
          }
        }
        if (!grew) break;
      }
    }
    int32_t* out = cells + t * 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      out[d] = blocked ? 0 : lo[d];
      out[3 + d] = blocked ? -1 : hi[d];
    }
  }
  const unsigned long long m = __ballot(blocked);
  if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(n_blocked, (unsigned long long)__popcll(m));
}

// ----------------------------------------------------------------------------------------------------
// the boxes of the states in metres: one thread per (vehicle, state)
// ----------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void state_boxes_kernel(int64_t n_state, int K, CorridorGrid g,
                                                           const int32_t* __restrict__ cells, double shrink,
                                                           double* __restrict__ lo, double* __restrict__ hi,
                                                           unsigned long long* __restrict__ n_open) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool open = false;
  if (t < n_state) {
    const int j = (int)(t % K);
    double l[3], u[3];
    bool given = j > 0;
    if (j > 0) {
      const CorridorCells a = corridor_load_cells(cells, t - 1), b = corridor_load_cells(cells, t);
      if (corridor_blocked(a) || corridor_blocked(b)) {
        given = false;
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          double La, Ha, Lb, Hb;
          corridor_metres(g, a, d, La, Ha);
          corridor_metres(g, b, d, Lb, Hb);
          l[d] = corridor_max(La, Lb) + shrink;
          u[d] = corridor_min(Ha, Hb) - shrink;
          if (l[d] > u[d]) given = false;
        }
      }
      open = !given;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      lo[t * D + d] = given ? l[d] : -INFINITY;
      hi[t * D + d] = given ? u[d] : INFINITY;
    }
  }
  const unsigned long long m = __ballot(open);
  if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(n_open, (unsigned long long)__popcll(m));
}

// ----------------------------------------------------------------------------------------------------
// the boxes into the bounds of the QP: one thread per (state j = 1 .. K-1, column)
// ----------------------------------------------------------------------------------------------------
struct SpaceBox {
  double pmin[3], pmax[3];
};

__global__ __launch_bounds__(256) void position_boxes_kernel(int N, int K, int D, double h, SpaceBox sp,
                                                              const double* __restrict__ states,
                                                              const double* __restrict__ lo, const double* __restrict__ hi,
                                                              double* __restrict__ lf, double* __restrict__ uf) {
#pragma clang fp contract(off)
  const int64_t C = (int64_t)N * D;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= C * (K - 1)) return;
  const int k = (int)(t / C);  // row of the position block: state j = k + 1
  const int64_t c = t % C;
  const int64_t i = c / D;
  const int d = (int)(c % D);
  const double hk = h * (double)(k + 1);
  const double hkv = hk * states[C + c];
  const double off = states[c] + hkv;  // (bound_of of scp_traj.hip)
  const int64_t e = (i * K + (k + 1)) * D + d;
  const int64_t row = ((int64_t)(3 * K - 1) + k) * C + c;
  lf[row] = corridor_max(sp.pmin[d], lo[e]) - off;
  uf[row] = corridor_min(sp.pmax[d], hi[e]) - off;
}

// ----------------------------------------------------------------------------------------------------
// the check: one wave per vehicle, lanes over its segments
// ----------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void check_corridor_kernel(int N, int K, double h, CorridorGrid g,
                                                              const int32_t* __restrict__ cells,
                                                              const double* __restrict__ pos, const double* __restrict__ vel,
                                                              const double* __restrict__ acc, double tol,
                                                              scp_corridor_stats* __restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;  // (the whole wave)
  double best = -INFINITY;
  unsigned best_g = 0xffffffffu;
  unsigned n_blocked = 0;
  unsigned long long n_outside = 0;
  for (int gseg = lane; gseg < K; gseg += 64) {
    const int64_t s = i * K + gseg;
    const CorridorCells c = corridor_load_cells(cells, s);
    if (corridor_blocked(c)) {
      ++n_blocked;
      continue;
    }
    double excess = -INFINITY;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double p = pos[s * D + d], v = vel[s * D + d], a = acc[s * D + d];
      double lo_v, hi_v;
      corridor_extremes(p, v, a, 0.0, h, lo_v, hi_v);
      double L, H;
      corridor_metres(g, c, d, L, H);
      excess = corridor_max(excess, corridor_max(L - lo_v, hi_v - H));
    }
    if (excess > tol) ++n_outside;
    if (excess > best || best_g == 0xffffffffu) {  // (ascending g within a lane: a tie keeps the lower g)
      best = excess;
      best_g = (unsigned)gseg;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const unsigned og = __shfl_xor(best_g, o);
    n_blocked += __shfl_xor(n_blocked, o);
    n_outside += __shfl_xor(n_outside, o);
    const bool take = og != 0xffffffffu && (best_g == 0xffffffffu || ob > best || (ob == best && og < best_g));
    if (take) {
      best = ob;
      best_g = og;
    }
  }
  if (lane == 0) {
    scp_corridor_stats r;
    r.max_excess = best;
    r.segment = best_g;
    r.n_blocked = n_blocked;
    r.n_outside = n_outside;
    r.reserved = 0;
    out[i] = r;
  }
}

}  // namespace

// ----------------------------------------------------------------------------------------------------
// host side (the first three are shared with the lattice calls: scp_corridor_device.h)
// ----------------------------------------------------------------------------------------------------
int corridor_grid(scp_ctx* ctx, const char* who, int D, const scp_occupancy_grid* grid, CorridorGrid& g) {
  SCP_REQUIRE(ctx, D == 2 || D == 3, "%s: D=%d (2 or 3)", who, D);
  SCP_REQUIRE(ctx, grid, "%s: null grid", who);
  SCP_REQUIRE(ctx, grid->cell > 0.0 && grid->cell < __builtin_huge_val(), "%s: bad cell size %g", who, grid->cell);
  int64_t n = 1;
  for (int d = 0; d < 3; ++d) {
    SCP_REQUIRE(ctx, grid->dims[d] >= 1, "%s: grid dimension %d is %d (>= 1)", who, d, grid->dims[d]);
    n *= grid->dims[d];
    SCP_REQUIRE(ctx, n <= CORRIDOR_MAX_CELLS, "%s: the grid has more than 2^24 cells", who);
    const double o = d < D ? grid->origin[d] : 0.0;
    SCP_REQUIRE(ctx, std::isfinite(o), "%s: origin[%d] is not finite", who, d);
    g.origin[d] = o;
    g.dims[d] = grid->dims[d];
  }
  SCP_REQUIRE(ctx, D == 3 || grid->dims[2] == 1, "%s: a 2-D grid has nz = 1, not %d", who, grid->dims[2]);
  g.cell = grid->cell;
  return SCP_OK;
}

int corridor_begin(scp_ctx* ctx) {
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev0, ctx->stream));
  return SCP_OK;
}

int corridor_end(scp_ctx* ctx) {  // after the call's last launch: launch errors, the end of the timing bracket
  SCP_HIP_CHECK(ctx, hipGetLastError());
  if (ctx->timing) SCP_HIP_CHECK(ctx, hipEventRecord(ctx->pair_ev1, ctx->stream));
  ctx->pair_timed = ctx->timing != 0;
  ctx->pair_ran = true;
  return SCP_OK;
}

extern "C" int scp_occupancy_prepare(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const uint8_t* occ, int32_t* sat) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = corridor_grid(ctx, "occupancy_prepare", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, occ && sat, "occupancy_prepare: null pointer");
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const int64_t rows = (int64_t)ny * nz;
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(sat_rows_kernel, dim3(scp_cdiv(rows, 4)), dim3(256), 0, ctx->stream, nx, rows, occ, sat);
  if (ny > 1)  // lines (x, z): t = z nx + x -> offset z (nx ny) + x
    hipLaunchKernelGGL(sat_lines_kernel, dim3(scp_cdiv((int64_t)nx * nz, 256)), dim3(256), 0, ctx->stream, (int64_t)nx * nz, nx,
                       (int64_t)nx * ny, ny, (int64_t)nx, sat);
  if (nz > 1)  // lines (x, y): t = y nx + x -> offset t
    hipLaunchKernelGGL(sat_lines_kernel, dim3(scp_cdiv((int64_t)nx * ny, 256)), dim3(256), 0, ctx->stream, (int64_t)nx * ny, nx,
                       (int64_t)nx, nz, (int64_t)nx * ny, sat);
  return corridor_end(ctx);
}

extern "C" int scp_corridor_boxes(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* sat,
                                  const double* ref, int max_grow, int32_t* cells, uint64_t* n_blocked) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = corridor_grid(ctx, "corridor_boxes", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "corridor_boxes: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, max_grow >= 0 && max_grow <= CORRIDOR_MAX_GROW, "corridor_boxes: max_grow=%d (0 .. %d)", max_grow,
              CORRIDOR_MAX_GROW);
  SCP_REQUIRE(ctx, sat && ref && cells && n_blocked, "corridor_boxes: null pointer");
  const int64_t n_seg = (int64_t)N * K;
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_blocked, 0, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(D == 2 ? corridor_boxes_kernel<2> : corridor_boxes_kernel<3>, dim3(scp_cdiv(n_seg, 256)), dim3(256), 0,
                     ctx->stream, n_seg, K, g, sat, ref, max_grow, cells, (unsigned long long*)n_blocked);
  return corridor_end(ctx);
}

extern "C" int scp_corridor_state_boxes(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* cells,
                                        double shrink, double* lo, double* hi, uint64_t* n_open) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = corridor_grid(ctx, "corridor_state_boxes", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "corridor_state_boxes: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, shrink >= 0.0 && shrink < __builtin_huge_val(), "corridor_state_boxes: bad shrink %g", shrink);
  SCP_REQUIRE(ctx, cells && lo && hi && n_open, "corridor_state_boxes: null pointer");
  const int64_t n_state = (int64_t)N * K;
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(n_open, 0, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(D == 2 ? state_boxes_kernel<2> : state_boxes_kernel<3>, dim3(scp_cdiv(n_state, 256)), dim3(256), 0,
                     ctx->stream, n_state, K, g, cells, shrink, lo, hi, (unsigned long long*)n_open);
  return corridor_end(ctx);
}

// the launch of scp_qp_set_position_boxes (scp_qp.hip): space = {min_0.., max_0..} as scp_qp keeps it (3 + 3 entries),
// states = the QP's [p0 | v0 | pf | vf]
int scp_launch_position_boxes(scp_ctx* ctx, int N, int K, int D, double h, const double* space6, const double* states,
                              const double* lo, const double* hi, double* lf, double* uf) {
  SpaceBox sp;
  for (int d = 0; d < 3; ++d) {
    sp.pmin[d] = space6[d];
    sp.pmax[d] = space6[3 + d];
  }
  const int64_t n = (int64_t)N * D * (K - 1);
  if (n <= 0) return SCP_OK;
  hipLaunchKernelGGL(position_boxes_kernel, dim3(scp_cdiv(n, 256)), dim3(256), 0, ctx->stream, N, K, D, h, sp, states, lo, hi,
                     lf, uf);
  SCP_HIP_CHECK(ctx, hipGetLastError());
  return SCP_OK;
}

extern "C" int scp_check_corridor(scp_ctx* ctx, int N, int K, int D, double h, const scp_occupancy_grid* grid,
                                  const int32_t* cells, const double* pos, const double* vel, const double* acc, double tol,
                                  scp_corridor_stats* out) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = corridor_grid(ctx, "check_corridor", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "check_corridor: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, h > 0.0 && h < __builtin_huge_val(), "check_corridor: bad time step h=%g", h);
  SCP_REQUIRE(ctx, !std::isnan(tol), "check_corridor: tol is NaN");
  SCP_REQUIRE(ctx, cells && pos && vel && acc && out, "check_corridor: null pointer");
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(D == 2 ? check_corridor_kernel<2> : check_corridor_kernel<3>, dim3(scp_cdiv(N, 4)), dim3(256), 0,
                     ctx->stream, N, K, h, g, cells, pos, vel, acc, tol, out);
  return corridor_end(ctx);
}
