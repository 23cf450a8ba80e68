// Static obstacles on gfx950: shortened reference paths.  Per vehicle the lattice path of scp_reference_paths is cut down to
// the nodes that cannot be skipped (a node sees another if every lattice step of the straight run between them is free), and
// the K + 1 reference points are placed by chord length along p0, the kept block centres, pf (ONE wave per vehicle, no LDS,
// no barrier).  The rules are stated in include/scp_hip.h ("shortened reference paths"); tests/shorten_ref.py is their
// restatement (integers exactly, lengths and points bit for bit: no contraction).
#include "scp_common.h"
#include "scp_lattice_device.h"

#include <cmath>

namespace {

// clear(A, B): no lattice step of the straight run from node a to node b holds an occupied cell within `clearance` cells.
// A node id outside the lattice is never clear (the caller's path is not trusted with the table's bounds).
template <int D>
__device__ inline bool nodes_clear(const Lattice& lt, const CorridorGrid& g, const int32_t* __restrict__ sat, int clearance,
                                   int a, int b) {
  if ((unsigned)a >= (unsigned)lt.nodes || (unsigned)b >= (unsigned)lt.nodes) return false;
  int XA[3] = {0, 0, 0}, dX[3] = {0, 0, 0};
  int n = 0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    XA[q] = lattice_coord(lt, a, q);
    dX[q] = lattice_coord(lt, b, q) - XA[q];
    const int len = dX[q] < 0 ? -dX[q] : dX[q];
    n = len > n ? len : n;
  }
  for (int k = 0; k < n; ++k) {  // (n <= max L_d - 1; X n + d k <= 32767^2: no overflow)
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const int u0 = XA[q] * n + dX[q] * k, u1 = u0 + dX[q];
      const int first = (u0 < u1 ? u0 : u1) / n;
      const int last = ((u0 < u1 ? u1 : u0) + n - 1) / n;
      const int from = first * lt.stride - clearance;
      const int to = last * lt.stride + (lt.stride - 1) + clearance;
      lo[q] = from < 0 ? 0 : from;
      hi[q] = to > g.dims[q] - 1 ? g.dims[q] - 1 : to;
    }
    if (occupied_in<D>(sat, g, lo, hi) != 0) return false;
  }
  return true;
}

// W_e of the shortened polyline, coordinate d: p0, the centres of the kept nodes other than the first and the last, pf
__device__ inline double shortened_vertex(const Lattice& lt, const CorridorGrid& g, const int32_t* path, const int32_t* kept,
                                          int nv, const double* p0, const double* pf, int e, int d) {
  if (e == 0) return p0[d];
  if (e == nv - 1) return pf[d];
  return lattice_centre(lt, g, path[kept[e]], d);
}

template <int D>
__global__ __launch_bounds__(256) void shorten_paths_kernel(int N, int K, Lattice lt, CorridorGrid g,
                                                             const int32_t* __restrict__ sat, int clearance,
                                                             const double* __restrict__ p0, const double* __restrict__ pf,
                                                             int max_path, const int32_t* __restrict__ path,
                                                             const scp_path_info* __restrict__ info, double* __restrict__ ref,
                                                             int32_t* kept, bool kept_wanted, scp_shorten_info* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= N) return;  // (the whole wave: a wave owns a vehicle and waits for nobody)
  const int32_t* my_path = path + i * max_path;
  int32_t* my_kept = kept + i * max_path;
  const double* a0 = p0 + i * D;
  const double* af = pf + i * D;
  const scp_path_info rec = info[i];
  int m = rec.status == 0 ? rec.n_nodes : 0;
  m = m > max_path ? max_path : m;
  if (m < 1) {
    if (kept_wanted)
      for (int t = lane; t < max_path; t += 64) my_kept[t] = -1;
    if (lane == 0) {
      scp_shorten_info r;
      r.n_kept = r.n_vertices = 0;
      r.length = r.length_before = 0.0;
      out[i] = r;
    }
    return;
  }

  // the kept nodes: from anchor t_e the LARGEST t in (t_e, m - 1] that the anchor sees, 64 candidates at a time from the
  // goal's end; at most m anchors, ceil(m / 64) blocks each.  Every quantity that steers a loop is the same in all lanes.
  int n = 0;
  for (int anchor = 0;;) {
    if (lane == 0) my_kept[n] = anchor;
    ++n;
    if (anchor >= m - 1 || n >= m) break;
    const int node_a = my_path[anchor];
    int next = anchor + 1;  // (seen over a set edge; also what a path of another lattice or clearance falls back to)
    for (int top = m - 1; top > anchor + 1; top -= 64) {
      const int t = top - lane;
      const bool sees = t > anchor + 1 && nodes_clear<D>(lt, g, sat, clearance, node_a, my_path[t]);
      const unsigned long long found = __ballot(sees);
      if (found) {
        next = top - (__ffsll(found) - 1);
        break;
      }
    }
    anchor = next;
  }
  const int nv = n < 2 ? 2 : n;
  if (kept_wanted)
    for (int t = n + lane; t < max_path; t += 64) my_kept[t] = -1;
  __threadfence_block();  // (lane 0's kept entries, read by every lane below)

  {
#pragma clang fp contract(off)
    // length_before: the lanes take 64 edges of p0, the block centres, pf at a time; the sum runs in order
    double before = 0.0;
    for (int base = 0; base < m + 1; base += 64) {
      const int t = base + lane;
      double len = 0.0;
      if (t < m + 1) {
        double sum = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double diff = reference_vertex(lt, g, my_path, m, a0, af, t + 1, d) - reference_vertex(lt, g, my_path, m, a0, af, t, d);
          const double sq = diff * diff;
          sum = sum + sq;
        }
        len = sqrt(sum);
      }
      const int count = m + 1 - base < 64 ? m + 1 - base : 64;
      for (int l = 0; l < count; ++l) before = before + __shfl(len, l);
    }

    // length: every lane walks the nv - 1 edges of the shortened polyline (the same loads and sums in all of them)
    double length = 0.0;
    for (int e = 0; e + 1 < nv; ++e) {
      double sum = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double diff = shortened_vertex(lt, g, my_path, my_kept, nv, a0, af, e + 1, d) -
                            shortened_vertex(lt, g, my_path, my_kept, nv, a0, af, e, d);
        const double sq = diff * diff;
        sum = sum + sq;
      }
      length = length + sqrt(sum);
    }
    if (lane == 0) {
      scp_shorten_info r;
      r.n_kept = n;
      r.n_vertices = nv;
      r.length = length;
      r.length_before = before;
      out[i] = r;
    }

    // the reference points.  States 0 and K are p0 and pf; lane l owns the states l, l + 64, ... in between, whose targets
    // grow, so one more walk over the edges serves them all: a state is placed on the first edge with S_{e+1} >= target.
    double* my_ref = ref + i * (int64_t)(K + 1) * D;
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        my_ref[d] = a0[d];
        my_ref[(int64_t)K * D + d] = af[d];
      }
    }
    int j = lane == 0 ? 64 : lane;
    double S = 0.0;
    for (int e = 0; e + 1 < nv; ++e) {
      double W0[3] = {0.0, 0.0, 0.0}, W1[3] = {0.0, 0.0, 0.0};
      double sum = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        W0[d] = shortened_vertex(lt, g, my_path, my_kept, nv, a0, af, e, d);
        W1[d] = shortened_vertex(lt, g, my_path, my_kept, nv, a0, af, e + 1, d);
        const double diff = W1[d] - W0[d];
        const double sq = diff * diff;
        sum = sum + sq;
      }
      const double len = sqrt(sum);
      const double S1 = S + len;
      while (j < K) {  // (at most ceil(K / 64) states per lane over the whole walk)
        const double frac = (double)j / (double)K;
        const double target = frac * length;
        if (!(S1 >= target)) break;
        double w = 0.0;
        if (len != 0.0) {
          const double along = target - S;
          const double q = along / len;
          w = q < 1.0 ? q : 1.0;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
          if (len == 0.0) {
            my_ref[(int64_t)j * D + d] = W0[d];
          } else {
            const double step = w * (W1[d] - W0[d]);
            my_ref[(int64_t)j * D + d] = W0[d] + step;
          }
        }
        j += 64;
      }
      S = S1;
    }
  }
}

}  // namespace

extern "C" int scp_shorten_paths(scp_ctx* ctx, int N, int K, int D, const scp_occupancy_grid* grid, const int32_t* sat, int stride,
                                 int clearance, const double* p0, const double* pf, int max_path, const int32_t* path,
                                 const scp_path_info* info, double* ref, int32_t* kept, scp_shorten_info* out) {
  CorridorGrid g;
  Lattice lt;
  int rc = lattice_begin(ctx, "shorten_paths", D, grid, stride, g, lt);
  if (rc) return rc;
  SCP_REQUIRE(ctx, clearance >= 0, "shorten_paths: clearance=%d (>= 0 cells)", clearance);
  SCP_REQUIRE(ctx, N >= 1 && K >= 1, "shorten_paths: bad shape N=%d K=%d", N, K);
  SCP_REQUIRE(ctx, max_path >= 1 && max_path <= lt.nodes, "shorten_paths: max_path=%d (1 .. %d nodes)", max_path, lt.nodes);
  SCP_REQUIRE(ctx, sat && p0 && pf && path && info && ref && out, "shorten_paths: null pointer");
  clearance = clipped_clearance(D, g, clearance);
  const bool kept_wanted = kept != nullptr;
  if ((rc = path_table(ctx, N, max_path, kept))) return rc;
  // measured with 64, 128 and 256 threads (1, 2 and 4 vehicles per workgroup) on a 46 x 46 and a 32 x 32 x 32 lattice with
  // 1024 vehicles: within 2 % of each other on both, so the finest grain
  const int threads = ctx->shorten_threads ? ctx->shorten_threads : 64;
  const int per_group = threads / 64;
  if ((rc = corridor_begin(ctx))) return rc;
  hipLaunchKernelGGL(D == 2 ? shorten_paths_kernel<2> : shorten_paths_kernel<3>, dim3(scp_cdiv(N, per_group)), dim3(threads), 0,
                     ctx->stream, N, K, lt, g, sat, clearance, p0, pf, max_path, path, info, ref, kept, kept_wanted, out);
  return corridor_end(ctx);
}
