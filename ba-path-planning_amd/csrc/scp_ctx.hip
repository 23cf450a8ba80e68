// The context of libscp_hip.so: its lifecycle and options, the scratch buffers it owns, and how the host waits for the words
// kernels leave in mapped host memory.
#include "scp_common.h"
#include "scp_traj_device.h"

#include <sys/prctl.h>
#include <time.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

// ----------------------------------------------------------------------------------------------------
// context
// ----------------------------------------------------------------------------------------------------
extern "C" int scp_abi_version(void) { return SCP_ABI_VERSION; }

extern "C" int scp_ctx_create(int device, void* hip_stream, scp_ctx** out) {
  if (!out) return SCP_ERR_INVALID;
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return SCP_ERR_HIP;
  scp_ctx* ctx = new scp_ctx();
  memset(ctx, 0, sizeof(*ctx));
  ctx->device = device;
  ctx->stream = (hipStream_t)hip_stream;
  ctx->timing = 1;
  ctx->small_pass = getenv("SCP_NO_SMALL_PASS") ? 0 : 1;  // (developer switch; scp_ctx_set_option at run time)
  ctx->fused_step_prep = 1;
  ctx->near_pass = 1;  // auto (scp_ctx_set_near_pass)
  ctx->asgw_prices_in_lds = -1;  // auto
  ctx->stg_batch_transposed = -1;  // auto
  if (hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->n_cu = 0;
  if (hipMalloc(&ctx->d_scratch, 72 * sizeof(double)) != hipSuccess ||
      hipMemset(ctx->d_scratch, 0, 72 * sizeof(double)) != hipSuccess ||  // ([64]: ticket counter of scp_rel_step)
      hipHostMalloc(&ctx->h_scratch, 72 * sizeof(double)) != hipSuccess ||
      memset(ctx->h_scratch, 0, 72 * sizeof(double)) == nullptr ||        // ([64]: its completion word)
      hipHostGetDevicePointer((void**)&ctx->h_scratch_dev, ctx->h_scratch, 0) != hipSuccess ||
      hipHostMalloc(&ctx->h_mirror, sizeof(scp_stats_mirror)) != hipSuccess ||
      hipHostGetDevicePointer((void**)&ctx->d_mirror, ctx->h_mirror, 0) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipEventCreate(&ctx->pair_ev0) != hipSuccess || hipEventCreate(&ctx->pair_ev1) != hipSuccess ||
      hipMalloc(&ctx->wg_part, 4 * SCP_SMALL_MAX_WG * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc(&ctx->d_ticket, 64) != hipSuccess || hipMemset(ctx->d_ticket, 0, 64) != hipSuccess) {
    delete ctx;
    return SCP_ERR_HIP;
  }
  ctx->solved = (unsigned long long*)(ctx->d_ticket + 12);  // the last 16 of its 64 bytes
  ctx->delay_solved = (unsigned long long*)(ctx->d_ticket + 10);  // the 8 before them
  ctx->lag_solved = (unsigned long long*)(ctx->d_ticket + 8);     // and the 8 before those
  *out = ctx;
  return SCP_OK;
}

// Per-context switches (include/scp_hip.h).  "kernel_timing": HIP events around every pairwise kernel and every QP solve
// (two queue packets each) are what `linearize_ms`, `violations_ms` and `solve_ms` are read from; 0: none are recorded --
// the pass times read 0, solve_ms becomes the host's wall clock around the solve (the host waits for its result anyway).
// "single_launch_passes": the one-launch form of the pairwise passes of small problems (pair_pass_kernel<.., SMALL>); 0:
// prep kernel + pass + compaction as for large problems (same results; tests compare the two).
// "fused_step_prep": where a pass runs as several launches, its prep launch derives the positions it stages -- from the
// accelerations at the start of a step, from the QP's time-major solution in a round -- instead of following a layout change
// and a kinematics launch; 0: those launches run as before (same results; tests/test_step_prep_gpu.py compares the two).
// "delay_lag_chunk" / "delay_time_chunk": lags / global segments per workgroup of scp_delay_margins; 0 (default): the call
// chooses (same results; tests/test_delay_gpu.py compares forced chunks with the call's own).
// "lagc_lag_chunk" / "lagc_time_chunk": the same two of scp_lag_conflicts (tests/test_stagger_gpu.py).
// "stg_batch_threads": threads per workgroup of scp_schedule_starts_batch, 0 (default): the call chooses by N, or 256 / 1024
// (same results; tests/test_stagger_search_gpu.py compares the two).  "stg_batch_transposed": it reads the columns of the masks
// from a transposed copy made per call in the workspace of the continuous-time passes (-1, default: from 16 candidates on; 0 never;
// 1 always; same results, same test).
// "assign_wide_min_bidders" / "assign_wide_prices_in_lds" / "assign_wide_control_threads": scp_assign_goals_wide's three
// size-dependent forks -- the bidder count from which a round runs on the whole chip (0: the call chooses; 1: every round;
// >= N: none), where its narrow runs keep the prices (-1 auto, 0 global memory, 1 LDS where 8 N bytes fit) and the threads
// of its control workgroup (0: 256 up to N = 512, else 1024; or either number); same results
// (tests/test_assignment_wide_gpu.py compares them).
extern "C" int scp_ctx_set_option(scp_ctx* ctx, const char* key, int value) {
  if (!ctx || !key) return SCP_ERR_INVALID;
  if (strcmp(key, "kernel_timing") == 0) {
    ctx->timing = value ? 1 : 0;
    if (!ctx->timing) ctx->pair_timed = false;
    return SCP_OK;
  }
  if (strcmp(key, "single_launch_passes") == 0) {
    ctx->small_pass = value ? 1 : 0;
    return SCP_OK;
  }
  if (strcmp(key, "fused_step_prep") == 0) {
    ctx->fused_step_prep = value ? 1 : 0;
    return SCP_OK;
  }
  if (strcmp(key, "delay_lag_chunk") == 0 || strcmp(key, "delay_time_chunk") == 0) {
    if (value < 0) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d is negative", key, value);
    (key[6] == 'l' ? ctx->delay_lag_chunk : ctx->delay_time_chunk) = value;
    return SCP_OK;
  }
  if (strcmp(key, "lagc_lag_chunk") == 0 || strcmp(key, "lagc_time_chunk") == 0) {
    if (value < 0) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d is negative", key, value);
    (key[5] == 'l' ? ctx->lagc_lag_chunk : ctx->lagc_time_chunk) = value;
    return SCP_OK;
  }
  if (strcmp(key, "stg_batch_threads") == 0) {
    if (value != 0 && value != 256 && value != 1024)
      return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need 0, 256 or 1024)", key, value);
    ctx->stg_batch_threads = value;
    return SCP_OK;
  }
  if (strcmp(key, "stg_batch_transposed") == 0) {
    if (value < -1 || value > 1) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need -1, 0 or 1)", key, value);
    ctx->stg_batch_transposed = value;
    return SCP_OK;
  }
  if (strcmp(key, "ref_path_threads") == 0) {  // scp_reference_paths, scp_reference_paths_weighted, scp_reference_paths_shared, scp_lattice_distances and scp_lattice_costs (same results; the GPU tests compare them)
    if (value != 0 && value != 64 && value != 256 && value != 512 && value != 1024)
      return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need 0, 64, 256, 512 or 1024)", key, value);
    ctx->ref_path_threads = value;
    return SCP_OK;
  }
  if (strcmp(key, "shorten_threads") == 0) {  // scp_shorten_paths (same results; tests/test_shorten_gpu.py compares them)
    if (value != 0 && value != 64 && value != 128 && value != 256)
      return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need 0, 64, 128 or 256)", key, value);
    ctx->shorten_threads = value;
    return SCP_OK;
  }
  if (strcmp(key, "raster_item_cells") == 0) {  // scp_rasterize_shapes (same grid; tests/test_rasterize_gpu.py compares them)
    if (value != 0 && (value < 64 || value > (1 << 24)))
      return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need 0 or 64 .. 2^24)", key, value);
    ctx->raster_item_cells = value;
    return SCP_OK;
  }
  if (strcmp(key, "assign_wide_min_bidders") == 0) {
    if (value < 0) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d is negative", key, value);
    ctx->asgw_min_bidders = value;
    return SCP_OK;
  }
  if (strcmp(key, "assign_wide_prices_in_lds") == 0) {
    if (value < -1 || value > 1) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need -1, 0 or 1)", key, value);
    ctx->asgw_prices_in_lds = value;
    return SCP_OK;
  }
  if (strcmp(key, "assign_wide_control_threads") == 0) {
    if (value != 0 && value != 256 && value != 1024)
      return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: %s=%d (need 0, 256 or 1024)", key, value);
    ctx->asgw_control_threads = value;
    return SCP_OK;
  }
  return scp_fail(ctx, SCP_ERR_INVALID, "ctx_set_option: unknown key '%s'", key);
}

extern "C" void scp_ctx_destroy(scp_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ctx->d_scratch);
  if (ctx->wg_part) (void)hipFree(ctx->wg_part);
  if (ctx->wg_rows) (void)hipFree(ctx->wg_rows);
  if (ctx->d_ticket) (void)hipFree(ctx->d_ticket);
  if (ctx->cmp_map) (void)hipFree(ctx->cmp_map);
  if (ctx->cmp_tot) (void)hipFree(ctx->cmp_tot);
  if (ctx->tm_scratch) (void)hipFree(ctx->tm_scratch);
  if (ctx->gen_ws) (void)hipFree(ctx->gen_ws);
  if (ctx->sep_ws) (void)hipFree(ctx->sep_ws);
  if (ctx->asg_ws) (void)hipFree(ctx->asg_ws);
  if (ctx->asgw_ws) (void)hipFree(ctx->asgw_ws);
  if (ctx->rast_ws) (void)hipFree(ctx->rast_ws);
  if (ctx->rast_host) (void)hipHostFree(ctx->rast_host);
  if (ctx->rast_copied) (void)hipEventDestroy(ctx->rast_copied);
  if (ctx->h_gen_flag) (void)hipHostFree(ctx->h_gen_flag);
  (void)hipHostFree(ctx->h_scratch);
  (void)hipHostFree(ctx->h_mirror);
  (void)hipEventDestroy(ctx->ev0);
  (void)hipEventDestroy(ctx->ev1);
  (void)hipEventDestroy(ctx->pair_ev0);
  (void)hipEventDestroy(ctx->pair_ev1);
  delete ctx;
}

// At least `need` bytes of device memory behind a (pointer, size) pair the ctx owns.  Growing frees the old buffer: work on
// the ctx stream may still use it, so the stream is drained first.  The new contents are undefined.
int scp_ctx_ensure_bytes(scp_ctx* ctx, void** buf, size_t* have, size_t need) {
  if (*have >= need) return SCP_OK;
  if (*buf) {
    SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    SCP_HIP_CHECK(ctx, hipFree(*buf));
    *buf = nullptr;
    *have = 0;
  }
  SCP_HIP_CHECK(ctx, hipMalloc(buf, need));
  *have = need;
  return SCP_OK;
}

hipError_t scp_raise_lds_limit(int device, const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> allowed;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = allowed[std::make_pair(device, kernel)];
  if (have >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

static std::atomic<int> g_host_wait_mode{0};

extern "C" void scp_set_host_wait(int mode) {
  g_host_wait_mode.store(mode == 1 || mode == 2 ? mode : 0, std::memory_order_relaxed);
}

bool scp_wait_host_word(volatile unsigned long long* word, unsigned long long seq, int timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  const int wait_mode = g_host_wait_mode.load(std::memory_order_relaxed);
  const bool sleepy = wait_mode != 0;
  const unsigned spin_first = wait_mode == 2 ? 0u : 2000u;  // mode 2: nap at once (more solver threads than cores)
  if (sleepy) {
    // the kernel's default timer slack (50 us) would stretch every 20 us nap to ~75 us -- a third of a 25-step persistent
    // launch; 1 us of slack for this thread
    static thread_local bool slack_set = false;
    if (!slack_set) {
      (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
      slack_set = true;
    }
  }
  unsigned spins = 0;
  while (*word != seq) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
    ++spins;
    if (sleepy && spins > spin_first) {  // mode 1: ~20 us of spinning first: the kernel is a long one, give the core away
      struct timespec ts = {0, 20000};
      nanosleep(&ts, nullptr);
      if ((spins & 0x3FF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s)) break;
    } else if ((spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s)) {
      break;
    }
  }
  const bool ok = *word == seq;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return ok;
}

int scp_ctx_wait_stats(scp_ctx* ctx, scp_pair_stats* out) {
  if (ctx->mirror_seq == 0) return scp_fail(ctx, SCP_ERR_STATE, "no pass with a row list has run yet");
  if (!scp_wait_host_word(&ctx->h_mirror->seq, ctx->mirror_seq, 30)) {
    SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // surfaces a launch failure, if that is why nothing arrived
    if (ctx->h_mirror->seq != ctx->mirror_seq) return scp_fail(ctx, SCP_ERR_HIP, "pair pass: the stats mirror was not written");
  }
  *out = ctx->h_mirror->stats;
  return SCP_OK;
}

// scp_rel_step's result from the partial sums the latest small-problem violations pass left in the mirror (call after
// scp_ctx_wait_stats): the same sums in the same order as scp_rel_step's host side
void scp_ctx_mirror_rel(scp_ctx* ctx, int64_t n, double* out) {
  const int blocks = rel_step_blocks(n);
  double d2 = 0.0, b2 = 0.0;
  for (int b = 0; b < blocks; ++b) {
    d2 += ctx->h_mirror->rel[2 * b];
    b2 += ctx->h_mirror->rel[2 * b + 1];
  }
  out[0] = std::sqrt(d2);
  out[1] = std::sqrt(b2);
  out[2] = out[0] / out[1];
}

// ---- test hooks for the state a context carries from one call to the next ("What a context owns") ----
// Scratch: every word is written by the call that reads it, so any pattern between two calls must change nothing.  The
// invariants (cmp_map, the d_ticket block, scp_rel_step's ticket and completion word, the stats mirror) are left alone.
extern "C" int scp_ctx_debug_fill(scp_ctx* ctx, uint32_t word) {
  if (!ctx) return SCP_ERR_INVALID;
  const struct { void* p; size_t bytes; } scratch[] = {
      {ctx->tm_scratch, ctx->tm_bytes},     {ctx->cmp_tot, ctx->cmp_tot_bytes},
      {ctx->wg_part, 4 * SCP_SMALL_MAX_WG * sizeof(unsigned long long)},
      {ctx->wg_rows, ctx->wg_rows_bytes},   {ctx->gen_ws, ctx->gen_ws_bytes},
      {ctx->sep_ws, ctx->sep_ws_bytes},     {ctx->asg_ws, ctx->asg_ws_bytes},
      {ctx->asgw_ws, ctx->asgw_ws_bytes},   {ctx->rast_ws, ctx->rast_ws_bytes},
      {ctx->d_scratch, 64 * sizeof(double)}, {ctx->h_scratch_dev, 64 * sizeof(double)},
  };
  for (const auto& s : scratch)
    if (s.p && s.bytes >= sizeof(uint32_t))
      SCP_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)s.p, (int)word, s.bytes / sizeof(uint32_t), ctx->stream));
  return SCP_OK;
}

extern "C" int scp_ctx_debug_state(scp_ctx* ctx, scp_ctx_state* out) {
  if (!ctx || !out) return SCP_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  SCP_HIP_CHECK(ctx, hipMemcpy(out->ticket, ctx->d_ticket, 64, hipMemcpyDeviceToHost));
  SCP_HIP_CHECK(ctx, hipMemcpy(&out->rel_ticket, ctx->d_scratch + 64, sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t map_words = ctx->cmp_map_bytes / sizeof(uint32_t);
  if (map_words > 0) {
    uint32_t* map = (uint32_t*)malloc(map_words * sizeof(uint32_t));
    if (!map) return scp_fail(ctx, SCP_ERR_INVALID, "ctx_debug_state: no host memory for %zu map words", map_words);
    const hipError_t e = hipMemcpy(map, ctx->cmp_map, map_words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    for (size_t w = 0; e == hipSuccess && w < map_words; ++w) out->cmp_map_nonzero += map[w] != 0u;
    free(map);
    SCP_HIP_CHECK(ctx, e);
  }
  out->tm_bytes = ctx->tm_bytes;
  out->cmp_map_bytes = ctx->cmp_map_bytes;
  out->cmp_tot_bytes = ctx->cmp_tot_bytes;
  out->wg_rows_bytes = ctx->wg_rows_bytes;
  out->gen_ws_bytes = ctx->gen_ws_bytes;
  out->sep_ws_bytes = ctx->sep_ws_bytes;
  out->asg_ws_bytes = ctx->asg_ws_bytes;
  out->asgw_ws_bytes = ctx->asgw_ws_bytes;
  out->rast_ws_bytes = ctx->rast_ws_bytes;
  out->rast_host_bytes = ctx->rast_host_bytes;
  return SCP_OK;
}

extern "C" const char* scp_last_error(const scp_ctx* ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int scp_ctx_synchronize(scp_ctx* ctx) {
  if (!ctx) return SCP_ERR_INVALID;
  SCP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return SCP_OK;
}
