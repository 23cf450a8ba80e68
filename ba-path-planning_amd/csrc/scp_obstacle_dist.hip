// Static obstacles on gfx950: the exact squared distance field of an occupancy grid (a separable transform: one scan along x,
// one lower-envelope pass along y and along z) and the clearance pass that judges a plan against the map: per vehicle the
// minimum of the field over the exact cell ranges of its trajectory's pieces, where and when, and the fleet's curve per time
// step.  The rules are stated in include/scp_hip.h ("distance field and clearance"); tests/obstacle_distance_ref.py is their
// restatement (integers exactly; the doubles of the clearance pass operation by operation: no contraction).
#include "scp_common.h"
#include "scp_corridor_device.h"

#include <cmath>

namespace {

constexpr uint32_t DIST_NONE = 0xffffffffu;  // no occupied cell (UINT32_MAX)
constexpr int DIST_MAX_DIM = 32768;          // (dim - 1)^2 < 2^30 per coordinate: three of them fit 32 bits

__device__ inline uint32_t gap_square(int delta, int gap) {  // max(delta - gap, 0)^2, delta < 2^15
  const uint32_t e = delta > gap ? (uint32_t)(delta - gap) : 0u;
  return e * e;
}

// ----------------------------------------------------------------------------------------------------
// along x: one wave per row (y, z), 64 cells per trip.  The first sweep carries the nearest occupied cell at or below x from
// trip to trip and leaves x - x' in the row; the second runs from the row's end with the nearest one at or above x and
// writes max(min(x - x', x'' - x) - gap, 0)^2.  A lane owns the same cells in both sweeps, so it reads back its own stores.
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dist_rows_kernel(int nx, int64_t rows, int gap, const uint8_t* __restrict__ occ,
                                                         uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  const uint8_t* src = occ + row * nx;
  uint32_t* dst = out + row * nx;
  int carry = -1;
  for (int base = 0; base < nx; base += 64) {
    const int x = base + lane;
    int v = (x < nx && src[x] != 0) ? x : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(v, o);
      if (lane >= o && up > v) v = up;
    }
    if (carry > v) v = carry;
    if (x < nx) dst[x] = v < 0 ? DIST_NONE : (uint32_t)(x - v);
    carry = __shfl(v, 63);
  }
  constexpr int FAR = 0x7fffffff;
  carry = FAR;
  for (int base = ((nx - 1) / 64) * 64; base >= 0; base -= 64) {
    const int x = base + lane;
    int v = (x < nx && src[x] != 0) ? x : FAR;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int down = __shfl_down(v, o);
      if (lane + o < 64 && down < v) v = down;
    }
    if (carry < v) v = carry;
    if (x < nx) {
      uint32_t d = dst[x];
      if (v != FAR && (uint32_t)(v - x) < d) d = (uint32_t)(v - x);
      dst[x] = d == DIST_NONE ? DIST_NONE : gap_square((int)d, gap);
    }
    carry = __shfl(v, 0);
  }
}

// ----------------------------------------------------------------------------------------------------
// along y (stride = nx, count = ny) and along z (stride = nx ny, count = nz): out[c] = min over the cells c' of c's line of
// in[c'] + max(|n - n'| - gap, 0)^2.  One thread per cell, x fastest, so the reads of a step coalesce.  A cell starts from
// its own value and looks delta = 1, 2, .. cells to both sides; it stops as soon as the penalty alone reaches the best so
// far, at the latest at the line's end.  in != out.  AXIS 1 is y, 2 is z (the slowest coordinate: no wrap of t / stride); the
// two instances also keep the passes apart in a kernel trace.
// ----------------------------------------------------------------------------------------------------
template <int AXIS>
__global__ __launch_bounds__(256) void dist_envelope_kernel(int64_t cells, int64_t stride, int count, int gap,
                                                             const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cells) return;
  const int n = AXIS == 1 ? (int)((t / stride) % count) : (int)(t / stride);
  uint32_t best = in[t];
  const int reach = n > count - 1 - n ? n : count - 1 - n;
  for (int delta = 1; delta <= reach; ++delta) {
    const uint32_t pen = gap_square(delta, gap);
    if (pen >= best) break;
    if (n - delta >= 0) {
      const uint32_t v = in[t - (int64_t)delta * stride];
      if (v != DIST_NONE && v + pen < best) best = v + pen;  // (v < 2^31, pen < 2^30: no wrap)
    }
    if (n + delta < count) {
      const uint32_t v = in[t + (int64_t)delta * stride];
      if (v != DIST_NONE && v + pen < best) best = v + pen;
    }
  }
  out[t] = best;
}

// ----------------------------------------------------------------------------------------------------
// the clearance pass: one wave per vehicle, a lane owns the segments lane, lane + 64, .. and walks their pieces
// ----------------------------------------------------------------------------------------------------
// (value, segment, piece, cell) ordered lexicographically as two words; "none" is all ones (cell -1)
struct ObstacleKey {
  unsigned long long hi, lo;
};

template <int D>
__global__ __launch_bounds__(256) void obstacle_clearance_kernel(int N, int K, double h, CorridorGrid g,
                                                                  const int32_t* __restrict__ sat,
                                                                  const uint32_t* __restrict__ field, int pieces,
                                                                  const double* __restrict__ pos, const double* __restrict__ vel,
                                                                  const double* __restrict__ acc,
                                                                  scp_obstacle_stats* __restrict__ out,
                                                                  unsigned long long* __restrict__ step_min) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;  // (the whole wave)
  ObstacleKey best = {~0ull, ~0ull};
  uint32_t best_v = DIST_NONE;
  unsigned n_touch = 0, n_off = 0, n_wide = 0;
  for (int gseg = lane; gseg < K; gseg += 64) {
    const int64_t s = i * K + gseg;
    double p[D], v[D], a[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      p[d] = pos[s * D + d];
      v[d] = vel[s * D + d];
      a[d] = acc[s * D + d];
    }
    uint32_t seg_v = DIST_NONE;
    bool seg_judged = false;
    for (int piece = 0; piece < pieces; ++piece) {
      const double t0 = h * ((double)piece / (double)pieces);
      const double t1 = h * ((double)(piece + 1) / (double)pieces);
      int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
      bool off = false;
      int64_t count = 1;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        double lo_v, hi_v;
        corridor_extremes(p[d], v[d], a[d], t0, t1, lo_v, hi_v);
        const double flo = floor((lo_v - g.origin[d]) / g.cell);
        const double fhi = floor((hi_v - g.origin[d]) / g.cell);
        const double top = (double)(g.dims[d] - 1);
        // (a NaN fails the first two; then flo <= fhi, both finite, and the clipped values lie in [0, dims_d - 1])
        if (!(fabs(flo) < INFINITY) || !(fabs(fhi) < INFINITY) || fhi < 0.0 || flo >= (double)g.dims[d]) {
          off = true;
        } else {
          lo[d] = (int)(flo > 0.0 ? flo : 0.0);
          hi[d] = (int)(fhi < top ? fhi : top);
          count *= hi[d] - lo[d] + 1;
        }
      }
      if (off) {
        ++n_off;
        continue;
      }
      if (count > SCP_OBSTACLE_MAX_RANGE) {
        ++n_wide;
        continue;
      }
      seg_judged = true;
      if (occupied_in<D>(sat, g, lo, hi) != 0) ++n_touch;
      uint32_t pv = DIST_NONE;
      int pc = -1;
      for (int z = lo[2]; z <= hi[2]; ++z)  // (ascending linear index: a tie keeps the lowest cell; <= 4096 cells in all)
        for (int y = lo[1]; y <= hi[1]; ++y) {
          const int base = (z * g.dims[1] + y) * g.dims[0];
          for (int x = lo[0]; x <= hi[0]; ++x) {
            const uint32_t f = field[base + x];
            if (f < pv) {
              pv = f;
              pc = base + x;
            }
          }
        }
      if (pv < seg_v) seg_v = pv;
      if (pv < best_v) {  // (ascending (segment, piece) within a lane: a tie keeps the lower)
        best_v = pv;
        best.hi = ((unsigned long long)pv << 32) | (unsigned)gseg;
        best.lo = ((unsigned long long)(unsigned)piece << 32) | (unsigned)pc;
      }
    }
    if (seg_judged) atomicMin(step_min + gseg, ((unsigned long long)seg_v << 32) | (unsigned long long)i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ObstacleKey other;
    other.hi = __shfl_xor(best.hi, o);
    other.lo = __shfl_xor(best.lo, o);
    n_touch += __shfl_xor(n_touch, o);
    n_off += __shfl_xor(n_off, o);
    n_wide += __shfl_xor(n_wide, o);
    if (other.hi < best.hi || (other.hi == best.hi && other.lo < best.lo)) best = other;
  }
  if (lane == 0) {
    scp_obstacle_stats r;
    r.min_sq = (uint32_t)(best.hi >> 32);
    r.segment = (uint32_t)best.hi;
    r.piece = (uint32_t)(best.lo >> 32);
    r.cell = (int32_t)(uint32_t)best.lo;
    r.n_touch = n_touch;
    r.n_off = n_off;
    r.n_wide = n_wide;
    r.reserved = 0;
    out[i] = r;
  }
}

int distance_grid(scp_ctx* ctx, const char* who, int D, const scp_occupancy_grid* grid, CorridorGrid& g) {
  const int rc = corridor_grid(ctx, who, D, grid, g);
  if (rc) return rc;
  for (int d = 0; d < 3; ++d)
    SCP_REQUIRE(ctx, g.dims[d] <= DIST_MAX_DIM, "%s: grid dimension %d is %d (the squared distances fit 32 bits up to %d)", who,
                d, g.dims[d], DIST_MAX_DIM);
  return SCP_OK;
}

}  // namespace

extern "C" int scp_obstacle_distance(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, const uint8_t* occ, int gap,
                                     uint32_t* field) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = distance_grid(ctx, "obstacle_distance", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, gap == 0 || gap == 1, "obstacle_distance: gap=%d (0 or 1)", gap);
  SCP_REQUIRE(ctx, occ && field, "obstacle_distance: null pointer");
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const int64_t rows = (int64_t)ny * nz, cells = rows * nx;
  // every envelope pass writes the buffer it does not read; the last pass writes `field`
  const int n_env = (ny > 1 ? 1 : 0) + (nz > 1 ? 1 : 0);
  uint32_t* other = nullptr;
  if (n_env) {
    rc = scp_ctx_ensure_bytes(ctx, &ctx->sep_ws, &ctx->sep_ws_bytes, (size_t)cells * sizeof(uint32_t));
    if (rc) return rc;
    other = (uint32_t*)ctx->sep_ws;
  }
  uint32_t* cur = n_env == 1 ? other : field;
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(dist_rows_kernel, dim3(scp_cdiv(rows, 4)), dim3(256), 0, ctx->stream, nx, rows, gap, occ, cur);
  if (ny > 1) {
    uint32_t* next = cur == field ? other : field;
    hipLaunchKernelGGL(dist_envelope_kernel<1>, dim3(scp_cdiv(cells, 256)), dim3(256), 0, ctx->stream, cells, (int64_t)nx, ny, gap,
                       cur, next);
    cur = next;
  }
  if (nz > 1) {
    uint32_t* next = cur == field ? other : field;
    hipLaunchKernelGGL(dist_envelope_kernel<2>, dim3(scp_cdiv(cells, 256)), dim3(256), 0, ctx->stream, cells, (int64_t)nx * ny, nz,
                       gap, cur, next);
    cur = next;
  }
  return corridor_end(ctx);
}

extern "C" int scp_obstacle_clearance(scp_ctx* ctx, int N, int K, int D, double h, const scp_occupancy_grid* grid,
                                      const int32_t* sat, const uint32_t* field, int pieces, const double* pos, const double* vel,
                                      const double* acc, scp_obstacle_stats* out, uint64_t* step_min) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = distance_grid(ctx, "obstacle_clearance", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "obstacle_clearance: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, h > 0.0 && h < __builtin_huge_val(), "obstacle_clearance: bad time step h=%g", h);
  SCP_REQUIRE(ctx, pieces >= 1 && pieces <= SCP_OBSTACLE_MAX_PIECES, "obstacle_clearance: pieces=%d (1 .. %d)", pieces,
              SCP_OBSTACLE_MAX_PIECES);
  SCP_REQUIRE(ctx, sat && field && pos && vel && acc && out && step_min, "obstacle_clearance: null pointer");
  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(step_min, 0xff, (size_t)K * sizeof(uint64_t), ctx->stream));  // UINT64_MAX
  hipLaunchKernelGGL(D == 2 ? obstacle_clearance_kernel<2> : obstacle_clearance_kernel<3>, dim3(scp_cdiv(N, 4)), dim3(256), 0,
                     ctx->stream, N, K, h, g, sat, field, pieces, pos, vel, acc, out, (unsigned long long*)step_min);
  return corridor_end(ctx);
}
