// Static obstacles on gfx950: spheres / discs, boxes, capsules and polygons / prisms into the occupancy grid that
// scp_occupancy_prepare and everything after it consume.  The rules are stated in include/scp_hip.h ("shapes into an
// occupancy grid"); tests/rasterize_ref.py is their restatement over all cells.  The host side prunes: per shape a conservative
// cell range, cut into work items; the kernel decides: a workgroup per item, a thread per cell, x fastest.
#include "scp_common.h"
#include "scp_corridor_device.h"
#include "scp_rasterize_device.h"

#include <cmath>
#include <vector>

namespace {

constexpr int RAST_THREADS = 256;
constexpr int RAST_ITEM_CELLS = 1024;    // "raster_item_cells" = 0
constexpr int64_t RAST_MAX_ITEMS = 1 << 18;
constexpr int RAST_MAX_ITEM_CELLS = 1 << 24;  // (the whole of the largest grid: then a shape is one item)
constexpr int RAST_VERTEX_BLOCK = 256;   // edges of a polygon staged in LDS at a time

struct RasterItem {  // a box of cells of one shape's range: 32 bytes
  int32_t shape;
  int32_t x0, y0, z0;
  int32_t wx, wy, wz;
  int32_t reserved;
};

template <int D>
__global__ __launch_bounds__(RAST_THREADS) void rasterize_kernel(CorridorGrid g, double margin,
                                                                  const scp_obstacle_shape* __restrict__ shapes,
                                                                  const double* __restrict__ vertices,
                                                                  const RasterItem* __restrict__ items,
                                                                  uint8_t* __restrict__ occ) {
#pragma clang fp contract(off)
  __shared__ double vx[RAST_VERTEX_BLOCK + 1], vy[RAST_VERTEX_BLOCK + 1];
  const RasterItem it = items[blockIdx.x];                // (uniform: scalar loads)
  const scp_obstacle_shape* s = shapes + it.shape;
  const int kind = s->kind;
  const int cells = it.wx * it.wy * it.wz;                // <= 2^24
  const int trips = (cells + RAST_THREADS - 1) / RAST_THREADS;
  const double m2 = margin * margin;
  for (int trip = 0; trip < trips; ++trip) {
    const int i = trip * RAST_THREADS + (int)threadIdx.x;
    const int ii = i < cells ? i : 0;
    const int row = ii / it.wx;
    const int c[3] = {it.x0 + (ii - row * it.wx), it.y0 + row % it.wy, it.z0 + row / it.wy};
    // (the host cut the items inside the grid; a cell outside it is never stored)
    const bool mine = i < cells && c[0] < g.dims[0] && c[1] < g.dims[1] && c[2] < g.dims[2];
    double lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double a = g.cell * (double)c[d];
      const double b = g.cell * ((double)c[d] + 1.0);
      lo[d] = g.origin[d] + a;
      hi[d] = g.origin[d] + b;
    }
    bool hit = false;
    if (kind == SCP_SHAPE_SPHERE) {
      const double reach = s->p[6] + margin;
      hit = rast_box_g2<D>(lo, hi, s->p, s->p) < reach * reach;
    } else if (kind == SCP_SHAPE_BOX) {
      const double g2 = rast_box_g2<D>(lo, hi, s->p, s->p + 3);
      hit = g2 < m2 || g2 == 0.0;
    } else if (kind == SCP_SHAPE_CAPSULE) {
      double a[D], e[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        a[d] = s->p[d];
        e[d] = s->p[3 + d] - s->p[d];
      }
      const double reach = s->p[6] + margin;
      const double g2 = rast_segment_g2<D>(lo, hi, a, e);
      hit = g2 < reach * reach || g2 == 0.0;
    } else {  // SCP_SHAPE_POLYGON: every thread of the workgroup takes every barrier (kind, trips and n are uniform)
      const int n = s->n_vertices;
      const double* v = vertices + 2 * (int64_t)s->first_vertex;
      double gz = 0.0;
      if (D == 3) gz = rast_max(rast_max(lo[2] - s->p[1], s->p[0] - hi[2]), 0.0);
      const double gz2 = gz * gz;
      const bool level = gz2 < m2 || gz == 0.0;  // (without it g2 = g2xy + gz2 >= gz2 >= m2 and g2 != 0: no edge can hit)
      const double cx = g.origin[0] + g.cell * ((double)c[0] + 0.5);
      const double cy = g.origin[1] + g.cell * ((double)c[1] + 0.5);
      bool odd = false;
      for (int first = 0; first < n; first += RAST_VERTEX_BLOCK) {
        const int count = n - first < RAST_VERTEX_BLOCK ? n - first : RAST_VERTEX_BLOCK;  // edges first .. first + count
        __syncthreads();  // (the previous block's readers)
        for (int j = (int)threadIdx.x; j <= count; j += RAST_THREADS) {
          const int k = first + j < n ? first + j : first + j - n;  // (the closing edge ends at v_0)
          vx[j] = v[2 * k];
          vy[j] = v[2 * k + 1];
        }
        __syncthreads();
        if (mine && level && !hit) {
          for (int j = 0; j < count; ++j) {  // every lane reads the same edge: a broadcast
            const double p[2] = {vx[j], vy[j]};
            const double q[2] = {vx[j + 1], vy[j + 1]};
            const double e[2] = {q[0] - p[0], q[1] - p[1]};
            const double g2 = rast_segment_g2<2>(lo, hi, p, e) + gz2;
            if (g2 < m2 || g2 == 0.0) {  // (the parity decides nothing any more)
              hit = true;
              break;
            }
            odd = odd != rast_crossed(p[0], p[1], q[0], q[1], cx, cy);
          }
        }
      }
      hit = level && (hit || odd);
    }
    if (mine && hit) occ[((int64_t)c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0]] = 1;
  }
}

bool all_finite(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// the inclusive cell range of [vmin - reach, vmax + reach] in coordinate d with two cells of slack, clipped to the grid; a
// value that is not a number keeps the whole side (the range only prunes)
void cell_range(const CorridorGrid& g, int d, double vmin, double vmax, double reach, int& lo, int& hi) {
  const double n = (double)g.dims[d];
  const double flo = std::floor((vmin - reach - g.origin[d]) / g.cell) - 2.0;
  const double fhi = std::floor((vmax + reach - g.origin[d]) / g.cell) + 2.0;
  lo = flo > 0.0 ? (flo < n ? (int)flo : g.dims[d]) : 0;
  hi = fhi < n - 1.0 ? (fhi >= 0.0 ? (int)fhi : -1) : g.dims[d] - 1;
}

struct ShapeRange {
  int lo[3], hi[3];
  bool empty;
};

// how the range is cut at `item_cells` cells per item: rows along x first
void tile_of(const ShapeRange& r, int item_cells, int tile[3]) {
  int64_t left = item_cells;
  for (int d = 0; d < 3; ++d) {
    const int64_t w = r.hi[d] - r.lo[d] + 1;
    tile[d] = (int)(w < left ? w : left);
    left = left / tile[d] > 1 ? left / tile[d] : 1;
  }
}

int64_t count_items(const std::vector<ShapeRange>& ranges, int item_cells) {
  int64_t total = 0;
  for (const ShapeRange& r : ranges) {
    if (r.empty) continue;
    int tile[3];
    tile_of(r, item_cells, tile);
    int64_t n = 1;
    for (int d = 0; d < 3; ++d) n *= (r.hi[d] - r.lo[d] + tile[d]) / tile[d];
    total += n;
  }
  return total;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int scp_rasterize_shapes(scp_ctx* ctx, int D, const scp_occupancy_grid* grid, int n_shapes,
                                    const scp_obstacle_shape* shapes, int n_vertices, const double* vertices, double margin,
                                    uint8_t* occ) {
  if (!ctx) return SCP_ERR_INVALID;
  CorridorGrid g;
  int rc = corridor_grid(ctx, "rasterize_shapes", D, grid, g);
  if (rc) return rc;
  SCP_REQUIRE(ctx, margin >= 0.0 && margin < __builtin_huge_val(), "rasterize_shapes: margin=%g (finite, >= 0)", margin);
  SCP_REQUIRE(ctx, n_shapes >= 0 && n_shapes <= SCP_RASTER_MAX_SHAPES, "rasterize_shapes: n_shapes=%d (0 .. %d)", n_shapes,
              SCP_RASTER_MAX_SHAPES);
  SCP_REQUIRE(ctx, n_vertices >= 0 && n_vertices <= SCP_RASTER_MAX_VERTICES, "rasterize_shapes: n_vertices=%d (0 .. %d)",
              n_vertices, SCP_RASTER_MAX_VERTICES);
  SCP_REQUIRE(ctx, occ && (shapes || n_shapes == 0) && (vertices || n_vertices == 0), "rasterize_shapes: null pointer");
  SCP_REQUIRE(ctx, all_finite(vertices, 2 * n_vertices), "rasterize_shapes: a vertex is not finite");

  // the checks and the cell range of every shape
  std::vector<ShapeRange> ranges((size_t)n_shapes);
  for (int i = 0; i < n_shapes; ++i) {
    const scp_obstacle_shape& s = shapes[i];
    double vmin[3] = {0.0, 0.0, 0.0}, vmax[3] = {0.0, 0.0, 0.0}, reach = margin;
    if (s.kind == SCP_SHAPE_SPHERE || s.kind == SCP_SHAPE_CAPSULE || s.kind == SCP_SHAPE_BOX) {
      const bool two = s.kind != SCP_SHAPE_SPHERE, round = s.kind != SCP_SHAPE_BOX;
      SCP_REQUIRE(ctx, all_finite(s.p, D) && (!two || all_finite(s.p + 3, D)) && (!round || std::isfinite(s.p[6])),
                  "rasterize_shapes: shape %d (kind %d) has a parameter that is not finite", i, s.kind);
      SCP_REQUIRE(ctx, !round || s.p[6] >= 0.0, "rasterize_shapes: shape %d has the radius %g (>= 0)", i, s.p[6]);
      for (int d = 0; d < D; ++d) {
        const double other = two ? s.p[3 + d] : s.p[d];
        SCP_REQUIRE(ctx, s.kind != SCP_SHAPE_BOX || other >= s.p[d], "rasterize_shapes: box %d has max < min in coordinate %d", i, d);
        vmin[d] = std::fmin(s.p[d], other);
        vmax[d] = std::fmax(s.p[d], other);
      }
      if (round) reach = s.p[6] + margin;
    } else if (s.kind == SCP_SHAPE_POLYGON) {
      SCP_REQUIRE(ctx, s.n_vertices >= 3 && s.n_vertices <= SCP_RASTER_MAX_POLYGON,
                  "rasterize_shapes: polygon %d has %d vertices (3 .. %d)", i, s.n_vertices, SCP_RASTER_MAX_POLYGON);
      SCP_REQUIRE(ctx, s.first_vertex >= 0 && s.first_vertex <= n_vertices - s.n_vertices,
                  "rasterize_shapes: polygon %d reads the vertices %d .. %d of %d", i, s.first_vertex,
                  s.first_vertex + s.n_vertices - 1, n_vertices);
      if (D == 3) {
        SCP_REQUIRE(ctx, all_finite(s.p, 2), "rasterize_shapes: polygon %d has a height that is not finite", i);
        SCP_REQUIRE(ctx, s.p[1] >= s.p[0], "rasterize_shapes: polygon %d has z1 < z0", i);
        vmin[2] = s.p[0];
        vmax[2] = s.p[1];
      }
      const double* v = vertices + 2 * (size_t)s.first_vertex;
      for (int d = 0; d < 2; ++d) {
        vmin[d] = vmax[d] = v[d];
        for (int k = 1; k < s.n_vertices; ++k) {
          vmin[d] = std::fmin(vmin[d], v[2 * k + d]);
          vmax[d] = std::fmax(vmax[d], v[2 * k + d]);
        }
      }
    } else {
      return scp_fail(ctx, SCP_ERR_INVALID, "rasterize_shapes: shape %d has the kind %d (0 .. 3)", i, s.kind);
    }
    ShapeRange& r = ranges[i];
    r.empty = false;
    for (int d = 0; d < 3; ++d) {
      if (d < D)
        cell_range(g, d, vmin[d], vmax[d], reach, r.lo[d], r.hi[d]);
      else
        r.lo[d] = r.hi[d] = 0;
      if (r.hi[d] < r.lo[d]) r.empty = true;
    }
  }

  // the work items
  int item_cells = ctx->raster_item_cells ? ctx->raster_item_cells : RAST_ITEM_CELLS;
  int64_t n_items = count_items(ranges, item_cells);
  while (n_items > RAST_MAX_ITEMS && item_cells < RAST_MAX_ITEM_CELLS) {  // (at 2^24 a shape is one item: <= 65536 items)
    item_cells *= 2;
    n_items = count_items(ranges, item_cells);
  }
  const int64_t cells = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];
  const size_t o_vertices = align16((size_t)n_shapes * sizeof(scp_obstacle_shape));
  const size_t o_items = align16(o_vertices + (size_t)n_vertices * 2 * sizeof(double));
  const size_t total = o_items + (size_t)n_items * sizeof(RasterItem);
  if (n_items > 0) {
    SCP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = scp_ctx_ensure_bytes(ctx, &ctx->rast_ws, &ctx->rast_ws_bytes, total))) return rc;
    if (!ctx->rast_copied)
      SCP_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->rast_copied, hipEventDisableTiming));
    else
      SCP_HIP_CHECK(ctx, hipEventSynchronize(ctx->rast_copied));  // the previous call's copy has left the host buffer
    if (ctx->rast_host_bytes < total) {
      if (ctx->rast_host) SCP_HIP_CHECK(ctx, hipHostFree(ctx->rast_host));
      ctx->rast_host = nullptr;
      ctx->rast_host_bytes = 0;
      SCP_HIP_CHECK(ctx, hipHostMalloc(&ctx->rast_host, total));
      ctx->rast_host_bytes = total;
    }
    char* h = (char*)ctx->rast_host;
    memcpy(h, shapes, (size_t)n_shapes * sizeof(scp_obstacle_shape));
    if (n_vertices > 0) memcpy(h + o_vertices, vertices, (size_t)n_vertices * 2 * sizeof(double));
    RasterItem* item = (RasterItem*)(h + o_items);
    for (int i = 0; i < n_shapes; ++i) {
      const ShapeRange& r = ranges[i];
      if (r.empty) continue;
      int tile[3];
      tile_of(r, item_cells, tile);
      for (int z = r.lo[2]; z <= r.hi[2]; z += tile[2])
        for (int y = r.lo[1]; y <= r.hi[1]; y += tile[1])
          for (int x = r.lo[0]; x <= r.hi[0]; x += tile[0]) {
            const int wx = r.hi[0] - x + 1, wy = r.hi[1] - y + 1, wz = r.hi[2] - z + 1;
            *item++ = RasterItem{i, x, y, z, wx < tile[0] ? wx : tile[0], wy < tile[1] ? wy : tile[1], wz < tile[2] ? wz : tile[2], 0};
          }
    }
    if (item - (RasterItem*)(h + o_items) != n_items)
      return scp_fail(ctx, SCP_ERR_STATE, "rasterize_shapes: %lld work items counted, %lld made", (long long)n_items,
                      (long long)(item - (RasterItem*)(h + o_items)));
  }

  if ((rc = corridor_begin(ctx))) return rc;
  SCP_HIP_CHECK(ctx, hipMemsetAsync(occ, 0, (size_t)cells, ctx->stream));
  if (n_items > 0) {
    char* ws = (char*)ctx->rast_ws;
    SCP_HIP_CHECK(ctx, hipMemcpyAsync(ws, ctx->rast_host, total, hipMemcpyHostToDevice, ctx->stream));
    SCP_HIP_CHECK(ctx, hipEventRecord(ctx->rast_copied, ctx->stream));
    hipLaunchKernelGGL(D == 2 ? rasterize_kernel<2> : rasterize_kernel<3>, dim3((unsigned)n_items), dim3(RAST_THREADS), 0,
                       ctx->stream, g, margin, (const scp_obstacle_shape*)ws, (const double*)(ws + o_vertices),
                       (const RasterItem*)(ws + o_items), occ);
  }
  return corridor_end(ctx);
}
