// capi_msm.hip -- the MSM entry points of the C ABI: base registration and parking, every hm_msm_* form, tickets, the drop-in call's
// converted-base cache (keyed by digest.hip), hm_set_msm_devices, hm_g1_sum and the MSM settings and statistics.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "hm_internal.h"

namespace hm {

static std::mutex g_msm_devices_mu;
static std::vector<int> g_msm_devices;             // hm_set_msm_devices; empty = the calling thread's device (under g_msm_devices_mu)
static std::atomic<int> g_host_base_cache{1};      // hm_set_host_base_cache
static std::atomic<uint32_t> g_fixed_base_from_log{[] {      // hm_set_fixed_base_threshold
  const char* v = std::getenv("HALO2_MI355X_FIXED_BASE_FROM_LOG");
  return (uint32_t)(v && *v ? std::atoi(v) : 17);
}()};

std::vector<int> msm_device_list() {
  std::lock_guard<std::mutex> lk(g_msm_devices_mu);
  return g_msm_devices;
}

void msm_set_window_override(int c);  // msm.hip
void msm_set_phase_timing(int mode);   // msm.hip

// device_ms: the hipEvent span of the launch chain that carried this MSM -- passed ONCE per chain (a grouped chain
// carries up to eight MSMs: the others pass 0).  Chains in flight overlap, so msm_device_us is a sum of spans, not a
// wall time: hm_stats documents it as such.
static void count_msm(DeviceCtx& ctx, size_t n, double device_ms) {
  uint32_t lg = 0;
  while ((n >> (lg + 1)) != 0) ++lg;
  ctx.calls.msm_calls += 1;
  ctx.calls.msm_points += n;
  ctx.calls.msm_by_log[lg & 31] += 1;
  ctx.calls.msm_device_us += device_ms * 1e3;
}

// Released buffers are parked for the next registration of that size instead of hipFree'd (which waits for the whole
// device): at most four sets and at most kParkedBytesMax in total -- a caller that registers a plain set per call (the
// tensor form of best_multiexp) recycles its 64 B/point buffer for ever, while a released fixed-base table (W copies:
// 12 GiB at 2^24 points) goes back to the allocator instead of sitting in the park.
constexpr size_t kParkedBytesMax = (size_t)2 << 30;
static size_t parked_bytes(const DeviceCtx& ctx) {
  size_t t = 0;
  for (const auto& f : ctx.free_bases) t += f.xy_bytes + f.inf_bytes;
  return t;
}
static void free_bases_entry(DeviceCtx& ctx, BasesEntry& b) {
  // no kernel reads these buffers any more (synchronous calls have returned, tickets were awaited)
  if (ctx.free_bases.size() < 4 && parked_bytes(ctx) + b.xy_bytes + b.inf_bytes <= kParkedBytesMax) {
    ctx.free_bases.push_back(FreeBases{b.d_xy, b.d_inf, b.xy_bytes, b.inf_bytes});
  } else {
    if (b.d_xy) (void)hipFree(b.d_xy);
    if (b.d_inf) (void)hipFree(b.d_inf);
  }
  b.d_xy = nullptr;
  b.d_inf = nullptr;
}
// hipFree every parked buffer (an allocation failed: the memory may be sitting here); true when there was anything
bool drop_parked_bases(DeviceCtx& ctx) {
  const bool any = !ctx.free_bases.empty();
  for (auto& f : ctx.free_bases) {
    if (f.d_xy) (void)hipFree(f.d_xy);
    if (f.d_inf) (void)hipFree(f.d_inf);
  }
  ctx.free_bases.clear();
  return any;
}

static BasesEntry* find_bases(DeviceCtx& ctx, uint64_t handle) {
  for (auto& b : ctx.bases)
    if (b.handle == handle) return &b;
  return nullptr;
}

// Which copy of the points a registration stores: DEFAULT = the table from hm_set_fixed_base_threshold's size on (falls back to
// the plain layout when W copies do not fit), TABLE = the caller asked for it (no fallback), PLAIN = one copy, never a table
// (transient sets: the table build costs ten MSMs).
enum class BaseLayout { DEFAULT, TABLE, PLAIN };
static std::atomic<uint64_t> g_default_table_dropped{0};   // DEFAULT registrations that fell back to the plain layout (hm_get_bases_info)

static int register_from_device(DeviceCtx& ctx, const uint32_t* d_ext, size_t n, hipStream_t stream, uint64_t* out_handle,
                                BaseLayout layout = BaseLayout::DEFAULT) {
  BasesEntry e;
  e.n = n;
  bool precomp = layout == BaseLayout::TABLE, by_default = false;
  if (layout == BaseLayout::DEFAULT) {   // the fixed-base table by default from the size where it pays (hm_set_fixed_base_threshold)
    const uint32_t from = g_fixed_base_from_log.load(std::memory_order_relaxed);
    if (from != 0 && from < 40 && n >= ((size_t)1 << from)) precomp = by_default = true;
  }
  if (precomp && n >= 256) {   // tiny sets gain nothing from a shared bucket set
    e.pc_c = msm_precomp_window(n);
    e.pc_W = (255 + e.pc_c - 1) / e.pc_c;
    if ((uint64_t)n * e.pc_W >= (1ull << 31)) { e.pc_c = 0; e.pc_W = 0; }
  }
  const size_t copies = e.pc_c ? e.pc_W : 1;
  const size_t xy_bytes = n ? n * 64 * copies : 64, inf_bytes = n ? n : 1;
  // buffers of a released set of the same size are reused (a caller that registers per call -- the
  // tensor form of best_multiexp -- then never reaches hipMalloc / hipFree and their device-wide waits)
  for (size_t i = 0; i < ctx.free_bases.size(); ++i) {
    if (ctx.free_bases[i].xy_bytes == xy_bytes && ctx.free_bases[i].inf_bytes == inf_bytes) {
      e.d_xy = ctx.free_bases[i].d_xy;
      e.d_inf = ctx.free_bases[i].d_inf;
      ctx.free_bases.erase(ctx.free_bases.begin() + i);
      break;
    }
  }
  if (!e.d_xy) {
    hipError_t err = hipMalloc((void**)&e.d_xy, xy_bytes);
    if (err != hipSuccess && drop_parked_bases(ctx)) {     // the memory may be parked: give it back and try once more
      (void)hipGetLastError();
      err = hipMalloc((void**)&e.d_xy, xy_bytes);
    }
    if (err != hipSuccess) {
      (void)hipGetLastError();
      e.d_xy = nullptr;
      // no room for W copies: a caller of the plain entry point asked for a base set, not for the table
      if (by_default && e.pc_c) {
        g_default_table_dropped.fetch_add(1, std::memory_order_relaxed);
        return register_from_device(ctx, d_ext, n, stream, out_handle, BaseLayout::PLAIN);
      }
      return hm_fail(HM_ERR_HIP, "register bases: allocation failed");
    }
    if (hipMalloc((void**)&e.d_inf, inf_bytes) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(e.d_xy);
      return hm_fail(HM_ERR_HIP, "register bases: allocation failed");
    }
  }
  e.xy_bytes = xy_bytes;
  e.inf_bytes = inf_bytes;
  int rc = msm_convert_bases(d_ext, e.d_xy, e.d_inf, n, stream);
  if (rc == HM_OK && e.pc_c) rc = msm_precompute(e.d_xy, e.d_inf, n, e.pc_c, e.pc_W, stream);
  if (rc != HM_OK) {
    (void)hipStreamSynchronize(stream);
    (void)hipFree(e.d_xy);
    (void)hipFree(e.d_inf);
    return rc;
  }
  e.handle = ctx.next_handle++;
  ctx.bases.push_back(e);
  *out_handle = e.handle;
  return HM_OK;
}

static int jac_to_affine_out(const uint64_t jac[12], int is_id, uint64_t out_xy[8], int* out_is_identity) {
  if (is_id) {
    std::memset(out_xy, 0, 64);
  } else {
    std::memcpy(out_xy, jac, 64);  // msm_run returns (x, y, 1): already affine
  }
  if (out_is_identity) *out_is_identity = is_id;
  return HM_OK;
}

// one device: upload the scalars, run against the registered set, Jacobian (x, y, 1) / zeros out
int msm_h_local(uint64_t handle, size_t offset, const uint64_t* scalars, size_t n, uint64_t jac[12], int* is_id) {
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BasesEntry* b = find_bases(*ctx, handle);
  if (!b) return hm_fail(HM_ERR_NOT_FOUND, "hm_msm_bn256_g1_h: unknown base handle");
  if (offset > b->n || n > b->n - offset) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1_h: offset + n exceeds the base set");
  void* d_s = ctx->io.ensure(n ? n * 32 : 32);
  if (!d_s) return hm_fail(HM_ERR_HIP, "hm_msm_bn256_g1_h: staging allocation failed");
  const double t0 = now_us();
  {
    const int rc = xfer_h2d(*ctx, d_s, scalars, n * 32, "hm_msm_bn256_g1_h: scalar upload");
    if (rc != HM_OK) return rc;
  }
  ctx->calls.msm_h2d_us += now_us() - t0;
  ctx->calls.h2d_bytes += n * 32;
  const uint32_t pc = (offset == 0 && n == b->n) ? b->pc_c : 0u;
  int rc = msm_run(*ctx, (const uint32_t*)d_s, b->d_xy + offset * 16, b->d_inf + offset, n, pc, jac, is_id, nullptr);
  if (rc != HM_OK) return rc;
  count_msm(*ctx, n, ctx->last_msm.t_total_ms);
  return HM_OK;
}


}  // namespace hm

using namespace hm;

extern "C" {

int hm_set_fixed_base_threshold(uint32_t log2_n) try {
  if (log2_n != 0 && (log2_n < 8 || log2_n > 31)) return hm_fail(HM_ERR_BAD_ARG, "hm_set_fixed_base_threshold: 0 or a size in [2^8, 2^31]");
  g_fixed_base_from_log.store(log2_n, std::memory_order_relaxed);
  return HM_OK;
} HM_API_CATCH("hm_set_fixed_base_threshold")

int hm_set_host_base_cache(int enable) try {
  g_host_base_cache.store(enable != 0, std::memory_order_relaxed);
  return HM_OK;
} HM_API_CATCH("hm_set_host_base_cache")

int hm_msm_set_window(int c) try {
  if (c != 0 && (c < 2 || c > 22)) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_set_window: c must be 0 or in [2, 22]");
  msm_set_window_override(c);
  return HM_OK;
} HM_API_CATCH("hm_msm_set_window")

int hm_msm_set_phase_timing(int mode) try {
  msm_set_phase_timing(mode);
  return HM_OK;
} HM_API_CATCH("hm_msm_set_phase_timing")

// the six registration entry points: {host array, device array} x {default, table, plain layout}
static int register_entry(const char* who, const uint64_t* bases_host, const void* d_bases, size_t n, void* stream, BaseLayout layout,
                          uint64_t* out_handle) {
  if (!out_handle || (n && !bases_host && !d_bases)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  {
    const std::vector<int> devs = multi_worker_flag() ? std::vector<int>() : msm_device_list();
    if (devs.size() >= 2) return multi_register(bases_host, d_bases, n, stream, (int)layout, devs, out_handle);
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const uint32_t* d_ext = (const uint32_t*)d_bases;
  hipStream_t st = (hipStream_t)stream;
  if (bases_host) {
    void* stage = ctx->io_bases.ensure(n ? n * 64 : 64);
    if (!stage) return hm_fail(HM_ERR_HIP, std::string(who) + ": staging allocation failed");
    {
      const int rc = xfer_h2d(*ctx, stage, bases_host, n * 64, who);
      if (rc != HM_OK) return rc;
    }
    d_ext = (const uint32_t*)stage;
    st = nullptr;
  }
  const int rc = register_from_device(*ctx, d_ext, n, st, out_handle, layout);
  if (rc != HM_OK) return rc;
  HM_HIP_CHECK(hipStreamSynchronize(st));
  return HM_OK;
}

int hm_register_bases(const uint64_t* bases, size_t n, uint64_t* out_handle) try {
  return register_entry("hm_register_bases", bases, nullptr, n, nullptr, BaseLayout::DEFAULT, out_handle);
} HM_API_CATCH("hm_register_bases")

int hm_register_bases_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle) try {
  return register_entry("hm_register_bases_dev", nullptr, d_bases, n, stream, BaseLayout::DEFAULT, out_handle);
} HM_API_CATCH("hm_register_bases_dev")

int hm_register_bases_precomp(const uint64_t* bases, size_t n, uint64_t* out_handle) try {
  return register_entry("hm_register_bases_precomp", bases, nullptr, n, nullptr, BaseLayout::TABLE, out_handle);
} HM_API_CATCH("hm_register_bases_precomp")

int hm_register_bases_precomp_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle) try {
  return register_entry("hm_register_bases_precomp_dev", nullptr, d_bases, n, stream, BaseLayout::TABLE, out_handle);
} HM_API_CATCH("hm_register_bases_precomp_dev")

int hm_register_bases_plain(const uint64_t* bases, size_t n, uint64_t* out_handle) try {
  return register_entry("hm_register_bases_plain", bases, nullptr, n, nullptr, BaseLayout::PLAIN, out_handle);
} HM_API_CATCH("hm_register_bases_plain")

int hm_register_bases_plain_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle) try {
  return register_entry("hm_register_bases_plain_dev", nullptr, d_bases, n, stream, BaseLayout::PLAIN, out_handle);
} HM_API_CATCH("hm_register_bases_plain_dev")

int hm_get_bases_info(uint64_t handle, hm_bases_info* out) try {
  if (!out) return hm_fail(HM_ERR_BAD_ARG, "hm_get_bases_info: null output");
  std::memset(out, 0, sizeof *out);
  out->default_tables_dropped = g_default_table_dropped.load(std::memory_order_relaxed);
  if (is_multi_handle(handle)) return multi_bases_info(handle, out);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const BasesEntry* b = find_bases(*ctx, handle);
  if (!b) return hm_fail(HM_ERR_NOT_FOUND, "hm_get_bases_info: unknown handle");
  out->n = b->n;
  out->table_windows = b->pc_W;
  out->table_window_bits = b->pc_c;
  out->device_bytes = b->xy_bytes + b->inf_bytes;
  out->devices = 1;
  out->parked_bytes = parked_bytes(*ctx);
  return HM_OK;
} HM_API_CATCH("hm_get_bases_info")

int hm_release_bases(uint64_t handle) try {
  if (is_multi_handle(handle)) return multi_release(handle);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (size_t i = 0; i < ctx->bases.size(); ++i) {
    if (ctx->bases[i].handle == handle) {
      // Every synchronous user has returned by now; only an un-awaited ticket can still read the set.
      // Then the buffers outlive the handle until that ticket's hm_msm_wait -- never a device-wide wait.
      bool in_flight = false;
      for (int k = 1; k < HM_MSM_SLOTS; ++k)
        if (ctx->msm_slots[k].busy && ctx->msm_slots[k].bases_handle == handle) in_flight = true;
      if (in_flight) ctx->zombie_bases.push_back(ctx->bases[i]);
      else free_bases_entry(*ctx, ctx->bases[i]);
      ctx->bases.erase(ctx->bases.begin() + i);
      return HM_OK;
    }
  }
  return hm_fail(HM_ERR_NOT_FOUND, "hm_release_bases: unknown handle");
} HM_API_CATCH("hm_release_bases")

int hm_msm_bn256_g1_dev(uint64_t handle, size_t offset, const void* d_scalars, size_t n, void* stream, uint64_t out_xyz[12]) try {
  if (!out_xyz || (n && !d_scalars)) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1_dev: null argument");
  if (is_multi_handle(handle)) {
    int id = 0;
    return multi_msm(handle, offset, d_scalars, false, n, stream, out_xyz, &id);
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BasesEntry* b = find_bases(*ctx, handle);
  if (!b) return hm_fail(HM_ERR_NOT_FOUND, "hm_msm_bn256_g1_dev: unknown base handle");
  if (offset > b->n || n > b->n - offset) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1_dev: offset + n exceeds the base set");
  int is_id = 0;
  const uint32_t pc = (offset == 0 && n == b->n) ? b->pc_c : 0u;   // the table only fits whole-set calls
  const int rc = msm_run(*ctx, (const uint32_t*)d_scalars, b->d_xy + offset * 16, b->d_inf + offset, n, pc, out_xyz, &is_id,
                         (hipStream_t)stream);
  if (rc == HM_OK) count_msm(*ctx, n, ctx->last_msm.t_total_ms);
  return rc;
} HM_API_CATCH("hm_msm_bn256_g1_dev")

// One ticket = one launch chain = `group` MSMs over the same base range (group > 1 only where the five-launch plan applies).
// use_table = false: run on the plain copy of the points even when the set carries a fixed-base table (the five-launch
// plan with its block compaction is what a SPARSE column of a prover-sized phase wants)
static int submit_chain(DeviceCtx* ctx, uint64_t handle, size_t offset, const void* const* d_scalars_list, uint32_t group, size_t n,
                        void* stream, uint64_t* out_ticket, const char* who, bool* all_busy = nullptr, bool use_table = true,
                        size_t live_rows = 0) {
  if (all_busy) *all_busy = false;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BasesEntry* b = find_bases(*ctx, handle);
  if (!b) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown base handle");
  if (offset > b->n || n > b->n - offset) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": offset + n exceeds the base set");
  int slot = -1;
  for (int i = 1; i < HM_MSM_SLOTS; ++i)        // slot 0 stays free for the synchronous calls
    if (!ctx->msm_slots[i].busy) { slot = i; break; }
  if (slot < 0) {
    if (all_busy) *all_busy = true;             // the batch call retries: another thread's tickets hold the slots
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": every slot is in flight; hm_msm_wait one first");
  }
  const uint32_t pc = (use_table && offset == 0 && n == b->n) ? b->pc_c : 0u;
  int rc;
  if (group == 1 && live_rows == 0) {
    ctx->msm_slots[slot].group = 1;
    rc = msm_enqueue(*ctx, slot, (const uint32_t*)d_scalars_list[0], b->d_xy + offset * 16, b->d_inf + offset, n, pc, (hipStream_t)stream);
  } else if (use_table && live_rows == 0) {     // dense columns of a phase on the table: one chain of the general pipeline for all of them
    if (pc == 0 || group > msm_table_group_max(n, pc)) return hm_fail(HM_ERR_INTERNAL, std::string(who) + ": a dense group needs the set's table");
    rc = msm_enqueue_table_group(*ctx, slot, reinterpret_cast<const uint32_t* const*>(d_scalars_list), group, b->d_xy, b->d_inf, n, pc,
                                 (hipStream_t)stream);
  } else {                                      // the five-launch plan, sized for the rows known to survive (a lone sparse column too)
    rc = msm_enqueue_group(*ctx, slot, reinterpret_cast<const uint32_t* const*>(d_scalars_list), group, b->d_xy + offset * 16,
                           b->d_inf + offset, n, (hipStream_t)stream, live_rows);
  }
  if (rc != HM_OK) return rc;
  ctx->msm_slots[slot].busy = true;
  ctx->msm_slots[slot].bases_handle = handle;
  ctx->msm_slots[slot].ticket = ctx->next_ticket++;
  *out_ticket = ctx->msm_slots[slot].ticket;
  return HM_OK;
}

int hm_msm_submit_dev(uint64_t handle, size_t offset, const void* d_scalars, size_t n, void* stream, uint64_t* out_ticket) try {
  if (!out_ticket || (n && !d_scalars)) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_submit_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (is_multi_handle(handle)) {      // tickets belong to one device: a replicated set is used through its copy here
    const int rc = multi_local_part(handle, ctx->device, &handle);
    if (rc != HM_OK) return rc;
  }
  return submit_chain(ctx, handle, offset, &d_scalars, 1, n, stream, out_ticket, "hm_msm_submit_dev");
} HM_API_CATCH("hm_msm_submit_dev")

static int wait_chain(DeviceCtx* ctx, uint64_t ticket, uint64_t* out_xyz, uint32_t capacity);
// a ticket whose wait failed half-way (an exception): let its chain drain and give the slot back, whatever state it is in
static void abandon_ticket(DeviceCtx* ctx, uint64_t ticket) noexcept {
  try {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int i = 1; i < HM_MSM_SLOTS; ++i) {
      MsmSlot& sl = ctx->msm_slots[i];
      if (!sl.busy || sl.ticket != ticket) continue;
      if (sl.n != 0 && sl.ev_ready) (void)hipEventSynchronize(sl.ev[4]);
      sl.awaiting = false;
      sl.busy = false;
      sl.live_ptr = nullptr;
    }
  } catch (...) {
  }
}

// The commitments of one prover phase in one call: `count` scalar arrays against the same base range, kept eight in
// flight on the library's own streams (created on first use), results in call order.  What a caller of
// hm_msm_submit_dev / hm_msm_wait would write by hand.
static int msm_batch_impl(DeviceCtx* ctx, uint64_t handle, size_t offset, const void* const* d_scalars, bool from_host, size_t n,
                          size_t count, void* stream, uint64_t* out_xyz) {
  constexpr int kLanes = HM_MSM_SLOTS - 1;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->batch_streams_ready) {
      for (int i = 0; i < kLanes; ++i) HM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->batch_streams[i], hipStreamNonBlocking));
      HM_HIP_CHECK(hipEventCreateWithFlags(&ctx->batch_event, hipEventDisableTiming));
      ctx->batch_streams_ready = true;
    }
    // the scalar arrays are produced on the caller's stream: every lane starts behind it
    HM_HIP_CHECK(hipEventRecord(ctx->batch_event, (hipStream_t)stream));
    for (int i = 0; i < kLanes; ++i) HM_HIP_CHECK(hipStreamWaitEvent(ctx->batch_streams[i], ctx->batch_event, 0));
  }
  // Submitting an MSM (launches, event records) and finishing one (the wait, the host fold over its window sums) each
  // cost tens of microseconds of host time, and a prover-sized MSM alone is bound by launch gaps and chain depth, not by
  // the GPU.  So (1) where the five-launch plan applies the commitments go through it in GROUPS -- one launch chain
  // carries up to HM_MSM_GROUP of them -- and (2) the calling thread only submits chains while a second thread of this
  // call awaits the tickets in order and folds.
  for (size_t i = 0; i < count; ++i)
    if (!d_scalars[i] && n) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_batch_bn256_g1_dev: null scalar array");
  // The chain plan: `order` lists the columns in submission order, chain ch carries order[first[ch] .. first[ch + 1]).
  std::vector<uint32_t> order(count), first;
  std::vector<uint8_t> chain_plain;                // per chain: 1 = run on the plain copy of the points (no table)
  std::vector<uint32_t> chain_live;                // per chain: rows known to survive the compaction at most (0 = unknown)
  for (size_t i = 0; i < count; ++i) order[i] = (uint32_t)i;
  {
    bool small_plan = false;
    const uint8_t* d_inf = nullptr;
    uint32_t dense_group = 1;                       // dense columns one chain of the general pipeline may carry (a table set, whole-set MSMs)
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      BasesEntry* b = find_bases(*ctx, handle);
      if (!b) return hm_fail(HM_ERR_NOT_FOUND, "hm_msm_batch_bn256_g1_dev: unknown base handle");
      if (offset > b->n || n > b->n - offset) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_batch_bn256_g1_dev: offset + n exceeds the base set");
      // the five-launch plan applies to the plain copy of the points, which a table set holds too (its first n entries):
      // sparse columns go there, dense ones take the table's shared bucket set through the general pipeline
      small_plan = msm_group_applies(n, 0);
      d_inf = b->d_inf + offset;
      if (offset == 0 && n == b->n && b->pc_c) dense_group = msm_table_group_max(n, b->pc_c);
    }
    static const size_t group_max_n = [] { const char* v = std::getenv("HALO2_MI355X_GROUP_MAX_LOG"); return (size_t)1 << (v && *v ? std::atoi(v) : 16); }();
    static const bool group_sparse = [] { const char* v = std::getenv("HALO2_MI355X_GROUP_SPARSE"); return !(v && *v == '0'); }();
    if (small_plan && n <= group_max_n) {
      // a commitment alone is bound by launch gaps here: consecutive groups, enough chains to keep several in flight,
      // none longer than a group: ceil(count / chains)
      // (and as many chains as waiter threads when there are commitments for them: the host fold of a chain's results is
      // serial per chain)
      const size_t chains_min = (count + HM_MSM_GROUP - 1) / HM_MSM_GROUP;
#ifndef HM_BATCH_SMALL_CHAINS
#define HM_BATCH_SMALL_CHAINS 4
#endif
      const size_t want = count / 2 < (size_t)HM_BATCH_SMALL_CHAINS ? count / 2 : (size_t)HM_BATCH_SMALL_CHAINS;
      const size_t chains = chains_min > want ? chains_min : want;
      size_t per_chain = (count + chains - 1) / (chains ? chains : 1);
      if (per_chain < 1) per_chain = 1;
      for (size_t f = 0; f < count; f += per_chain) {
        first.push_back((uint32_t)f);
        chain_plain.push_back(1);
      }
    } else if (small_plan && group_sparse && count >= 2) {
      // 2^17 .. 2^18: what a column costs depends on how many of its 256-row blocks SURVIVE the digits kernel's
      // compaction (zero scalars and identity bases contribute nothing), not on n.  A dense column is throughput-bound
      // and keeps a chain of its own (eight separate chains in flight interleave their phases better than one chain of
      // eight: measured 0.57 against 0.79 ms per commitment at 2^18); a SPARSE one -- an advice column with ~1 100 used
      // rows of 2^18 -- is pure chain latency (0.098 ms each one chain at a time, 36 of them 3.5 ms), so up to eight of
      // them share one launch chain.  The classification only decides the grouping, never the result.
      std::vector<uint32_t> live(count, 0);
      const uint32_t total_blocks = (uint32_t)((n + 255) / 256);
      int crc = from_host ? HM_OK : msm_count_live_blocks(*ctx, d_scalars, count, d_inf, n, (hipStream_t)stream, live.data());
      if (crc != HM_OK) return crc;
      if (from_host) {
        // host arrays: a sample decides (reading every word on the host would cost more than the upload): every 64th
        // block, never the first two or the last one (used rows lead, blinding rows trail)
        for (size_t i = 0; i < count; ++i) {
          const uint64_t* s = (const uint64_t*)d_scalars[i];
          uint32_t hits = 0, seen = 0;
          for (uint32_t blk = 2; blk + 1 < total_blocks; blk += 64) {
            const size_t lo = (size_t)blk * 256, hi = lo + 256 < n ? lo + 256 : n;
            uint64_t any = 0;
            for (size_t w = lo * 4; w < hi * 4; ++w) any |= s[w];
            hits += any != 0;
            ++seen;
          }
          live[i] = seen == 0 || hits != 0 ? total_blocks : 0;
        }
      }
      // Dense columns on a table set: up to `dense_group` of them share one chain of the general pipeline (every element a
      // bucket set of the same launches): the sort and the two-launch reduction then run at the chip's throughput instead
      // of as 26 small launches per commitment, and K3 is one launch over all of them.  How many per chain: as many chains
      // as keep three in flight, none longer than the plan allows.
      uint32_t n_dense = 0;
      for (size_t i = 0; i < count; ++i) n_dense += (uint64_t)live[i] * 16 > total_blocks ? 1u : 0u;
      uint32_t dense_per_chain = 1;
      if (dense_group > 1 && n_dense > 1) {
        const uint32_t chains = std::max<uint32_t>((n_dense + dense_group - 1) / dense_group, std::min<uint32_t>(3u, n_dense / 2));
        dense_per_chain = (n_dense + chains - 1) / chains;
      }
      std::vector<uint32_t> pending, plan, dense_pending;
      auto flush_dense = [&]() {
        if (dense_pending.empty()) return;
        first.push_back((uint32_t)plan.size());
        chain_plain.push_back(0);
        chain_live.resize(first.size(), 0);
        plan.insert(plan.end(), dense_pending.begin(), dense_pending.end());
        dense_pending.clear();
      };
      auto flush = [&]() {
        if (pending.empty()) return;
        first.push_back((uint32_t)plan.size());
        chain_plain.push_back(1);
        uint64_t rows = 0;                                       // device columns: counted blocks; host columns: a sample said "sparse" only
        if (!from_host)
          for (uint32_t i : pending) rows = std::max<uint64_t>(rows, (uint64_t)live[i] * 256);
        chain_live.resize(first.size() - 1, 0);
        chain_live.push_back((uint32_t)std::min<uint64_t>(rows ? rows : 0, n));
        plan.insert(plan.end(), pending.begin(), pending.end());
        pending.clear();
      };
      for (size_t i = 0; i < count; ++i) {
        if ((uint64_t)live[i] * 16 <= total_blocks) {           // sparse: joins the pending group
          pending.push_back((uint32_t)i);
          if (pending.size() == (size_t)HM_MSM_GROUP) flush();
        } else {                                                 // dense: on the table when the set has one, several per chain
          dense_pending.push_back((uint32_t)i);
          if (dense_pending.size() >= dense_per_chain) flush_dense();
        }
      }
      flush_dense();
      flush();
      order = plan;
    } else {
      for (size_t f = 0; f < count; ++f) first.push_back((uint32_t)f);
    }
    first.push_back((uint32_t)count);
  }
  const size_t n_chains = first.size() - 1;
  chain_plain.resize(n_chains, 0);
  chain_live.resize(n_chains, 0);

  uint64_t tickets[kLanes];
  // chain ch uses lane ch % kLanes; the lane is free again once chain ch - kLanes has been awaited (finished[] is set)
  std::unique_ptr<std::atomic<uint8_t>[]> finished(new std::atomic<uint8_t>[n_chains + 1]);
  for (size_t i = 0; i <= n_chains; ++i) finished[i].store(0, std::memory_order_relaxed);
  std::atomic<size_t> issued{0};
  std::atomic<int> submit_rc{HM_OK}, wait_rc{HM_OK};
  std::atomic<bool> no_more{false};
  int device = 0;
  HM_HIP_CHECK(hipGetDevice(&device));
  auto await_chain = [&](size_t d) {           // chain d carries the MSMs order[first[d] .. first[d + 1])
    int wrc;
    try {
      hm_fault_point("batch_await");
      uint64_t res[12 * HM_MSM_GROUP];
      const uint32_t members = first[d + 1] - first[d];
      wrc = wait_chain(ctx, tickets[d % kLanes], res, members);
      if (wrc == HM_OK)
        for (uint32_t e = 0; e < members; ++e) std::memcpy(out_xyz + 12 * (size_t)order[first[d] + e], res + 12 * e, 96);
    } catch (...) {                            // nothing may escape a waiter thread, and the chain must still count as awaited
      wrc = HM_ERR_INTERNAL;
      abandon_ticket(ctx, tickets[d % kLanes]);
    }
    if (wrc != HM_OK) {
      int expect = HM_OK;
      (void)wait_rc.compare_exchange_strong(expect, wrc);
    }
    finished[d].store(1, std::memory_order_release);
  };
  // Finishing a chain is host work too: the event wait, then a 255-doubling fold per commitment (~50 us each: 2 ms for
  // the 36 advice columns of a k = 18 proof on one thread -- measured as 40 % GPU idle time in that phase).  So up to
  // kWaiters threads of this call await the chains, waiter t taking chains t, t + T, t + 2T, ...; the calling thread
  // only submits.  They are started after the first lanes are filled, so that their creation overlaps the GPU's work.
#ifndef HM_BATCH_WAITERS
#define HM_BATCH_WAITERS 8      // A/B knob (tools/ab_build.sh): 8 against 4 -- 36 sparse commitments at k = 18 1.60 -> 1.41 ms, dense phases unchanged
#endif
  constexpr size_t kWaiters = HM_BATCH_WAITERS;
  size_t n_waiters = 0;                         // set before any waiter starts
  auto waiter = [&](size_t t) {
    (void)hipSetDevice(device);
    for (size_t d = t; d < n_chains; d += n_waiters) {
      while (issued.load(std::memory_order_acquire) <= d) {
        if (no_more.load(std::memory_order_acquire) && issued.load(std::memory_order_acquire) <= d) return;
        std::this_thread::yield();
      }
      await_chain(d);                          // even after an error: no ticket is left behind
    }
  };
  // host arrays are staged per lane in buffers of the device context: whole _h batch calls of different threads take turns.
  // Declared BEFORE the waiter guard, so that on every way out -- an exception unwinding out of the submit loop included --
  // the lock is released only AFTER the waiters have been joined and no chain of this call reads batch_io[] any more.
  std::unique_lock<std::mutex> host_turn;
  if (from_host) host_turn = std::unique_lock<std::mutex>(ctx->batch_h_mu);
  // the waiters are told to finish and are joined on EVERY way out of this function (an exception in the submit loop included)
  struct WaiterGuard {
    std::atomic<bool>& no_more;
    JoinOnExit pool;
    ~WaiterGuard() { no_more.store(true, std::memory_order_release); }     // members are destroyed after this body: then the join
  } guard{no_more, {}};
  bool threaded = false, waiters_started = false;
  size_t next_unthreaded = 0;                   // without waiters: the next chain the calling thread has to await itself
  auto start_waiters = [&]() {
    waiters_started = true;
    if (n_chains <= 1) return;                  // a lone chain: the calling thread awaits it
    n_waiters = n_chains < kWaiters ? n_chains : kWaiters;
    size_t started = 0;
    for (size_t t = 0; t < n_waiters; ++t)
      if (spawn_or_false(guard.pool, "batch_waiter_spawn", [&waiter, t] { waiter(t); })) ++started;
      else break;
    if (started == n_waiters) {
      threaded = true;
    } else {                                    // not every waiter could be had: the ones that started take what they take,
      no_more.store(true, std::memory_order_release);   // ... are drained, and this thread awaits everything still open
      for (auto& th : guard.pool.th) th.join();
      guard.pool.th.clear();
      no_more.store(false, std::memory_order_release);
    }
  };
  auto await_unthreaded_upto = [&](size_t limit) {      // the calling thread awaits every issued, unfinished chain below `limit`
    for (; next_unthreaded < limit && next_unthreaded < issued.load(); ++next_unthreaded)
      if (!finished[next_unthreaded].load(std::memory_order_acquire)) await_chain(next_unthreaded);
  };
  std::string submit_error;
  try {
  for (size_t ch = 0; ch < n_chains; ++ch) {
    hm_fault_point("batch_submit");
    if (ch >= (size_t)kLanes) {                 // every lane holds a ticket: chain ch - kLanes has to be awaited first
      if (!waiters_started) start_waiters();
      while (!finished[ch - kLanes].load(std::memory_order_acquire)) {
        if (threaded) std::this_thread::yield();
        else await_unthreaded_upto(ch - kLanes + 1);
      }
    }
    const uint32_t group = first[ch + 1] - first[ch];
    int rc;
    // host arrays: this chain's scalars cross PCIe on its own lane's stream (the lane's staging buffer is free again:
    // the chain that used it eight chains ago has been awaited), while the other lanes' chains compute
    const void* staged[HM_MSM_GROUP];
    for (uint32_t e = 0; e < group; ++e) staged[e] = d_scalars[order[first[ch] + e]];
    const void* const* chain_scalars = staged;
    if (from_host && n) {
      const int lane = (int)(ch % kLanes);
      const double t_h2d0 = now_us();
      uint8_t* buf;
      {
        std::lock_guard<std::mutex> lk(ctx->mu);
        buf = (uint8_t*)ctx->batch_io[lane].ensure((size_t)group * n * 32);
      }
      if (!buf) {
        submit_rc.store(hm_fail(HM_ERR_HIP, "hm_msm_batch_bn256_g1_h: staging allocation failed"));
        submit_error = hm_last_error();
        break;
      }
      // through the library's pinned lanes (xfer.hip), synchronous for this thread: the other lanes' chains compute meanwhile, and
      // this lane's chain is submitted behind it (a pageable hipMemcpyAsync blocked the submitting thread just the same)
      // the chain's arrays as ONE job of the lanes (an 8 MiB copy alone spends half its time starting threads and filling its pipeline)
      void* up_dev[HM_MSM_GROUP];
      void* up_host[HM_MSM_GROUP];
      size_t up_bytes[HM_MSM_GROUP];
      for (uint32_t e = 0; e < group; ++e) {
        up_dev[e] = buf + (size_t)e * n * 32;
        up_host[e] = const_cast<void*>(staged[e]);
        up_bytes[e] = n * 32;
      }
      const int xrc = xfer_many(*ctx, true, up_dev, up_host, up_bytes, group, "hm_msm_batch_bn256_g1_h: scalar upload");
      for (uint32_t e = 0; e < group; ++e) staged[e] = up_dev[e];
      if (xrc != HM_OK) {
        submit_rc.store(xrc);
        submit_error = hm_last_error();
        break;
      }
      std::lock_guard<std::mutex> lk(ctx->mu);
      ctx->calls.msm_h2d_us += now_us() - t_h2d0;
      ctx->calls.h2d_bytes += (uint64_t)group * n * 32;
    }
    const double t_wait0 = now_us();
    for (;;) {                                  // slots held by other callers' tickets (another thread's batch): wait for one
      bool all_busy = false;
      rc = submit_chain(ctx, handle, offset, chain_scalars, group, n, ctx->batch_streams[ch % kLanes], &tickets[ch % kLanes],
                        "hm_msm_batch_bn256_g1_dev", &all_busy, chain_plain[ch] == 0, chain_live[ch]);
      if (rc == HM_OK || !all_busy) break;
      if (now_us() - t_wait0 > 60e6) break;     // nobody awaits the tickets that hold the slots: report instead of spinning
      if (!waiters_started) start_waiters();
      if (!threaded && next_unthreaded < issued.load()) await_unthreaded_upto(next_unthreaded + 1);     // free one of our own first
      else std::this_thread::yield();
    }
    if (rc != HM_OK) {
      submit_rc.store(rc);
      submit_error = hm_last_error();
      break;
    }
    issued.store(ch + 1, std::memory_order_release);
  }
  } catch (...) {
    // Something threw between two submissions (vector growth, a fault point).  Chains already issued are in flight on the
    // lanes' staging buffers: the waiters (if any) are drained, then this thread awaits -- or, failing that, abandons --
    // every ticket no waiter took, so that no slot stays busy and nothing reads batch_io[] when host_turn is released.
    no_more.store(true, std::memory_order_release);
    for (auto& t : guard.pool.th)
      if (t.joinable()) t.join();
    guard.pool.th.clear();
    const size_t upto = issued.load();
    for (size_t d = 0; d < upto; ++d)
      if (!finished[d].load(std::memory_order_acquire)) await_chain(d);      // await_chain never throws: it abandons the ticket instead
    throw;
  }
  if (!waiters_started) start_waiters();
  no_more.store(true, std::memory_order_release);
  if (threaded) {
    for (auto& t : guard.pool.th) t.join();
    guard.pool.th.clear();
  }
  await_unthreaded_upto(n_chains);              // whatever no waiter took (none when they all started)
  if (submit_rc.load() != HM_OK) return hm_fail(submit_rc.load(), submit_error);
  if (wait_rc.load() != HM_OK) return hm_fail(wait_rc.load(), "hm_msm_batch_bn256_g1_dev: a commitment of the batch failed (see the waiter's error)");
  return HM_OK;
}

int hm_msm_batch_bn256_g1_dev(uint64_t handle, size_t offset, const void* const* d_scalars, size_t n, size_t count, void* stream,
                              uint64_t* out_xyz) try {
  if ((count && (!d_scalars || !out_xyz))) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_batch_bn256_g1_dev: null argument");
  if (is_multi_handle(handle)) return multi_msm_batch(handle, offset, d_scalars, false, n, count, stream, out_xyz);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return msm_batch_impl(ctx, handle, offset, d_scalars, false, n, count, stream, out_xyz);
} HM_API_CATCH("hm_msm_batch_bn256_g1_dev")

// The same for scalar arrays in HOST memory (what halo2's prover holds today): each chain's upload runs on its own
// lane's stream, so PCIe time hides behind the other chains' kernels.
int hm_msm_batch_bn256_g1_h(uint64_t handle, size_t offset, const uint64_t* const* scalars, size_t n, size_t count, uint64_t* out_xyz) try {
  if ((count && (!scalars || !out_xyz))) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_batch_bn256_g1_h: null argument");
  if (is_multi_handle(handle))
    return multi_msm_batch(handle, offset, reinterpret_cast<const void* const*>(scalars), true, n, count, nullptr, out_xyz);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return msm_batch_impl(ctx, handle, offset, reinterpret_cast<const void* const*>(scalars), true, n, count, nullptr, out_xyz);
} HM_API_CATCH("hm_msm_batch_bn256_g1_h")

// Await one ticket: out_xyz receives 12 words per MSM of its chain (at most `capacity` of them).
static int wait_chain(DeviceCtx* ctx, uint64_t ticket, uint64_t* out_xyz, uint32_t capacity) {
  int slot = -1;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int i = 1; i < HM_MSM_SLOTS; ++i)
      if (ctx->msm_slots[i].busy && ctx->msm_slots[i].ticket == ticket) slot = i;
    if (slot < 0) return hm_fail(HM_ERR_NOT_FOUND, "hm_msm_wait: unknown ticket");
    if (ctx->msm_slots[slot].awaiting) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_wait: another thread is already waiting for this ticket");
    if (ctx->msm_slots[slot].n != 0 && ctx->msm_slots[slot].group > capacity)
      return hm_fail(HM_ERR_BAD_ARG, "hm_msm_wait: the ticket belongs to a batch call");
    ctx->msm_slots[slot].awaiting = true;
  }
  // the blocking part -- the device-side wait and the host fold -- runs WITHOUT the context lock: other threads keep
  // submitting while this one waits (the slot stays busy, so nobody else touches it)
  MsmSlot& sl = ctx->msm_slots[slot];
  int is_id[HM_MSM_GROUP] = {};
  double host_us = 0;
  const int rc = msm_finish_wait_fold(sl, out_xyz, is_id, &host_us);
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rc != HM_OK) sl.live_ptr = nullptr;      // a chain that failed may have left its block counters anywhere
  if (rc == HM_OK) {
    msm_finish_record(*ctx, slot, host_us);
    for (uint32_t e = 0; e < (sl.n ? sl.group : 1u); ++e) count_msm(*ctx, sl.n, e == 0 ? ctx->last_msm.t_total_ms : 0.0);
  }
  sl.awaiting = false;
  sl.busy = false;
  // a base set released while this ticket was in flight: free it once no other ticket reads it
  for (size_t z = 0; z < ctx->zombie_bases.size();) {
    bool used = false;
    for (int k = 1; k < HM_MSM_SLOTS; ++k)
      if (ctx->msm_slots[k].busy && ctx->msm_slots[k].bases_handle == ctx->zombie_bases[z].handle) used = true;
    if (used) { ++z; continue; }
    free_bases_entry(*ctx, ctx->zombie_bases[z]);
    ctx->zombie_bases.erase(ctx->zombie_bases.begin() + z);
  }
  return rc;
}

int hm_msm_wait(uint64_t ticket, uint64_t out_xyz[12]) try {
  if (!out_xyz) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_wait: null output");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return wait_chain(ctx, ticket, out_xyz, 1);
} HM_API_CATCH("hm_msm_wait")

int hm_msm_bn256_g1_h(uint64_t handle, size_t offset, const uint64_t* scalars, size_t n, uint64_t out_xy[8],
                      int* out_is_identity) try {
  if (!out_xy || (n && !scalars)) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1_h: null argument");
  uint64_t jac[12];
  int is_id = 0;
  const int rc = is_multi_handle(handle) ? multi_msm(handle, offset, scalars, true, n, nullptr, jac, &is_id)
                                         : msm_h_local(handle, offset, scalars, n, jac, &is_id);
  if (rc != HM_OK) return rc;
  return jac_to_affine_out(jac, is_id, out_xy, out_is_identity);
} HM_API_CATCH("hm_msm_bn256_g1_h")

// The drop-in form of best_multiexp: both arrays are host memory.  The scalars cross PCIe in every call; the converted
// bases of the previous call are kept per device and reused only when the FULL-CONTENT digest and the length match (the
// pointer is not part of the key: create_proof passes the same params.g / g_lagrange prefix to every commitment, and a
// buffer reused with other contents -- the verifier's MSMs -- simply misses).  hm_set_host_base_cache(0) disables it.
static int msm_host_one(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t jac[12], int* is_id) {
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return msm_run(*ctx, nullptr, nullptr, nullptr, 0, 0, jac, is_id, nullptr);
  uint32_t* d_xy = (uint32_t*)ctx->conv_bases.ensure(n * 64);
  uint8_t* d_inf = (uint8_t*)ctx->conv_inf.ensure(n);
  void* d_s = ctx->io.ensure(n * 32);
  if (!d_xy || !d_inf || !d_s) return hm_fail(HM_ERR_HIP, "hm_msm_bn256_g1: staging allocation failed");
  const double t0 = now_us();
  uint64_t dg[4] = {0, 0, 0, 0};
  const bool use_cache = g_host_base_cache.load(std::memory_order_relaxed) != 0;
  if (use_cache) digest_bases(bases, n, dg);
  const bool hit = use_cache && ctx->cached_host_n == n && ctx->cached_xy == d_xy &&
                   std::memcmp(dg, ctx->cached_digest, sizeof dg) == 0;
  if (!hit) {
    ctx->cached_host_n = 0;
    void* stage = ctx->io_bases.ensure(n * 64);
    if (!stage) return hm_fail(HM_ERR_HIP, "hm_msm_bn256_g1: staging allocation failed");
    int rc = xfer_h2d(*ctx, stage, bases, n * 64, "hm_msm_bn256_g1: base upload");
    if (rc != HM_OK) return rc;
    rc = msm_convert_bases((const uint32_t*)stage, d_xy, d_inf, n, nullptr);
    if (rc != HM_OK) return rc;
    ctx->calls.h2d_bytes += n * 64;
    if (use_cache) {
      ctx->cached_host_n = n;
      ctx->cached_xy = d_xy;                    // a regrown buffer is a miss
      std::memcpy(ctx->cached_digest, dg, sizeof dg);
    }
  }
  {
    const int rc = xfer_h2d(*ctx, d_s, scalars, n * 32, "hm_msm_bn256_g1: scalar upload");
    if (rc != HM_OK) return rc;
  }
  ctx->calls.msm_h2d_us += now_us() - t0;
  ctx->calls.h2d_bytes += n * 32;
  int rc = msm_run(*ctx, (const uint32_t*)d_s, d_xy, d_inf, n, 0, jac, is_id, nullptr);
  if (rc == HM_OK) count_msm(*ctx, n, ctx->last_msm.t_total_ms);
  return rc;
}

// Single-process multi-GPU form of the host-pointer call (hm_set_msm_devices): contiguous index ranges, one host
// thread per device (multi.hip: run_per_device), each running the ordinary one-device path on its slice (its own
// uploads, no shared state), partial sums folded on the host.  No inter-GPU traffic: the only thing that leaves a
// device is a 96-byte point.
static int msm_host(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t jac[12], int* is_id) {
  if (n && (!scalars || !bases)) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1: null argument");
  const std::vector<int> devs = msm_device_list();
  const size_t parts = devs.size();
  if (parts < 2) return msm_host_one(scalars, bases, n, jac, is_id);
  if (n < parts * kMinShardPoints)     // too small to be worth splitting: the first listed device takes it whole
    return run_per_device({devs[0]}, [&](size_t) { return msm_host_one(scalars, bases, n, jac, is_id); });
  std::vector<uint64_t> partial(parts * 12, 0);
  const int rc = run_per_device(devs, [&](size_t r) {
    const size_t lo = n * r / parts, hi = n * (r + 1) / parts;
    int id = 0;
    return msm_host_one(scalars + lo * 4, bases + lo * 8, hi - lo, &partial[r * 12], &id);
  });
  if (rc != HM_OK) return rc;
  host_sum_points(partial.data(), parts, jac, is_id);
  return HM_OK;
}

int hm_set_msm_devices(const int* devices, int count) try {
  if (count < 0 || count > 64 || (count && !devices)) return hm_fail(HM_ERR_BAD_ARG, "hm_set_msm_devices: bad device list");
  const int visible = hm_device_count();
  if (count && visible <= 0) return hm_fail(HM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  for (int i = 0; i < count; ++i)
    if (devices[i] < 0 || devices[i] >= visible) return hm_fail(HM_ERR_BAD_ARG, "hm_set_msm_devices: device index out of range");
  std::lock_guard<std::mutex> lk(g_msm_devices_mu);
  g_msm_devices.assign(devices, devices + count);
  return HM_OK;
} HM_API_CATCH("hm_set_msm_devices")

int hm_msm_bn256_g1(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xy[8], int* out_is_identity) try {
  if (!out_xy) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1: null output");
  uint64_t jac[12];
  int is_id = 0;
  int rc = msm_host(scalars, bases, n, jac, &is_id);
  if (rc != HM_OK) return rc;
  return jac_to_affine_out(jac, is_id, out_xy, out_is_identity);
} HM_API_CATCH("hm_msm_bn256_g1")

int hm_msm_bn256_g1_jacobian(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xyz[12]) try {
  if (!out_xyz) return hm_fail(HM_ERR_BAD_ARG, "hm_msm_bn256_g1_jacobian: null output");
  int is_id = 0;
  return msm_host(scalars, bases, n, out_xyz, &is_id);
} HM_API_CATCH("hm_msm_bn256_g1_jacobian")

int hm_g1_sum(const uint64_t* points_xyz, size_t count, uint64_t out_xyz[12]) try {
  if (!out_xyz || (count && !points_xyz)) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_sum: null argument");
  if (count > (1u << 20)) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_sum: meant for a handful of partial results");
  hm_fault_point("g1_sum");
  int is_id = 0;
  host_sum_points(points_xyz, count, out_xyz, &is_id);
  return HM_OK;
} HM_API_CATCH("hm_g1_sum")

int hm_get_msm_stats(hm_msm_stats* out) try {
  if (!out) return hm_fail(HM_ERR_BAD_ARG, "hm_get_msm_stats: null output");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const MsmStats& s = ctx->last_msm;
  out->digits_ms = s.t_digits_ms; out->sort_ms = s.t_sort_ms; out->accumulate_ms = s.t_accum_ms;
  out->reduce_ms = s.t_reduce_ms; out->total_ms = s.t_total_ms; out->accumulate_kernel_ms = s.t_accum_kernel_ms;
  out->pairs = s.pairs; out->tasks = s.tasks; out->window_bits = s.c; out->windows = s.windows;
  return HM_OK;
} HM_API_CATCH("hm_get_msm_stats")

}  // extern "C"
