// capi.hip -- the core of the extern "C" boundary declared in include/halo2_mi355x.h: the error state and the exception barrier's
// handler, the fault points of the test build, the device contexts, memory, copies, settings and the call counters.  The entry points
// of each subsystem live in capi_msm.hip, capi_poly.hip, capi_g1.hip and capi_hash.hip.  Per-call device scratch (aux_scope's slots,
// stream_scratch's memory) is here too: this unit owns DeviceCtx, resets the slots in hm_shutdown, and is built with the fault points.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <initializer_list>
#include <map>
#include <stdexcept>
#include <string>

#include "hm_internal.h"

namespace hm {

// The commitments of a prover phase run eight at a time on eight streams (hm_msm_batch_bn256_g1_dev, hm_msm_submit_dev);
// the HIP runtime maps streams onto 4 hardware queues unless told otherwise, which caps the kernels actually in flight
// (measured at k = 18: a sparse column costs 0.215 ms with 4 queues, 0.136 ms with 16; a dense one 0.654 / 0.578 ms).
// The variable is read when the runtime initialises, so it is set -- without overriding the caller's own choice -- when
// this library is loaded; a process whose runtime is already up (e.g. torch touched the GPU first) keeps what it has.
namespace {
struct HwQueueDefault {
  HwQueueDefault() { (void)setenv("GPU_MAX_HW_QUEUES", "16", 0); }
} g_hw_queue_default;
}  // namespace

static thread_local std::string g_last_error;
static std::mutex g_ctx_mu;
static std::map<int, std::unique_ptr<DeviceCtx>> g_ctx;

int hm_fail(int code, const std::string& what) {
  g_last_error = what;
  return code;
}
const std::string& hm_last_error_string() { return g_last_error; }

// The handler of HM_API_CATCH: must not throw itself (the message is built inside its own try; when even that
// fails -- no memory for a short string -- the code alone goes back and the message stays empty).
int hm_guard_fail(const char* entry, const char* what) noexcept {
  try {
    g_last_error.assign(entry);
    g_last_error.append(": internal error caught at the C boundary: ");
    g_last_error.append(what ? what : "unknown exception");
  } catch (...) {
    g_last_error.clear();
  }
  return HM_ERR_INTERNAL;
}

#ifdef HM_FAULT_INJECTION
std::mutex g_fault_mu;
std::string g_fault_name;
long g_fault_after = -1;        // < 0: disarmed
void hm_fault_point(const char* point) {
  std::lock_guard<std::mutex> lk(g_fault_mu);
  if (g_fault_after < 0 || g_fault_name != point) return;
  if (g_fault_after-- == 0) throw std::runtime_error(std::string("injected fault at ") + point);
}
#endif

// ---- per-call device scratch: the stream slots behind aux_scope, the stream-ordered memory behind stream_scratch (hm_internal.h) ----
AuxSlot* aux_acquire(DeviceCtx& ctx, hipStream_t stream) {
  AuxSlot* pick = nullptr;
  for (auto& s : ctx.aux)
    if (s.used && s.stream == stream) pick = &s;        // stream order already protects its buffers
  if (!pick)
    for (auto& s : ctx.aux)
      if (!s.used) { pick = &s; break; }
  if (!pick) {
    for (auto& s : ctx.aux)                              // a slot whose last user has finished
      if (hipEventQuery(s.done) == hipSuccess && (!pick || s.last_use < pick->last_use)) pick = &s;
  }
  if (!pick) {                                           // all busy on other streams: queue behind the oldest
    pick = &ctx.aux[0];
    for (auto& s : ctx.aux)
      if (s.last_use < pick->last_use) pick = &s;
    if (hipStreamWaitEvent(stream, pick->done, 0) != hipSuccess) {
      hm_fail(HM_ERR_HIP, "aux slot: hipStreamWaitEvent failed");
      return nullptr;
    }
  }
  if (!pick->done && hipEventCreateWithFlags(&pick->done, hipEventDisableTiming) != hipSuccess) {
    hm_fail(HM_ERR_HIP, "aux slot: event creation failed");
    return nullptr;
  }
  pick->used = true;
  pick->stream = stream;
  pick->last_use = ++ctx.aux_clock;
  return pick;
}

int aux_release(DeviceCtx& ctx, AuxSlot* slot, hipStream_t stream) {
  (void)ctx;
  HM_HIP_CHECK(hipEventRecord(slot->done, stream));
  return HM_OK;
}

// Every request passes this first, whatever the buffers already hold.  Test build: an armed "scratch_alloc" makes the request fail like
// an exhausted device (as "device_malloc_oom" below).
static bool scratch_alloc_refused() {
  try { hm_fault_point("scratch_alloc"); } catch (const std::exception&) { return true; }      // product build: the empty inline
  return false;
}
void* aux_buffer(AuxSlot& slot, AuxBuf which, size_t bytes, const char* who) {
  DevBuf* const bufs[] = {&slot.scratch, &slot.table, &slot.args, &slot.work};
  if (which == AuxBuf::table && bytes < HM_AUX_TABLE_MIN) bytes = HM_AUX_TABLE_MIN;
  void* p = scratch_alloc_refused() ? nullptr : bufs[(int)which]->ensure(bytes);
  if (!p) hm_fail(HM_ERR_HIP, std::string(who) + ": scratch allocation failed");
  return p;
}
bool stream_scratch_alloc(const char* who, size_t bytes, hipStream_t stream, uint8_t** ws) {
  *ws = nullptr;                                         // stays null for 0 bytes: nothing to free
  const hipError_t e = scratch_alloc_refused() ? hipErrorOutOfMemory : bytes ? hipMallocAsync((void**)ws, bytes, stream) : hipSuccess;
  if (e != hipSuccess) hm_fail(HM_ERR_HIP, std::string(who) + ": scratch allocation failed");
  return e == hipSuccess;
}
int stream_scratch_free(const char* who, uint8_t* ws, hipStream_t stream, int rc) {
  const hipError_t fe = ws ? hipFreeAsync(ws, stream) : hipSuccess;
  if (rc == HM_OK && fe != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": hipFreeAsync: " + hipGetErrorString(fe));
  return rc;
}

DeviceCtx* ctx_for_current_device() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    hm_fail(HM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    return nullptr;
  }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    hm_fail(HM_ERR_NO_DEVICE, "hipGetDevice failed");
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  auto it = g_ctx.find(dev);
  if (it == g_ctx.end()) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
      hm_fail(HM_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
      return nullptr;
    }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
      hm_fail(HM_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
      return nullptr;
    }
    auto c = std::make_unique<DeviceCtx>();
    c->device = dev;
    it = g_ctx.emplace(dev, std::move(c)).first;
  }
  return it->second.get();
}

}  // namespace hm

using namespace hm;

extern "C" {

int hm_device_count(void) {      // no allocation, nothing that throws: "never fails" stays literal
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

int hm_set_device(int device) try {
  int count = hm_device_count();
  if (count <= 0) return hm_fail(HM_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= count) return hm_fail(HM_ERR_BAD_ARG, "hm_set_device: device index out of range");
  HM_HIP_CHECK(hipSetDevice(device));
  return HM_OK;
} HM_API_CATCH("hm_set_device")

const char* hm_last_error(void) { return g_last_error.c_str(); }
const char* hm_version(void) { return "halo2_mi355x 0.3 (gfx950; ff29 field layer)"; }

int hm_shutdown(void) try {
  int dev = 0;
  if (hm_device_count() <= 0 || hipGetDevice(&dev) != hipSuccess) return HM_OK;
  multi_release_touching(dev);     // multi-device sets with a part here go first (their parts elsewhere are released too)
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  auto it = g_ctx.find(dev);
  if (it == g_ctx.end()) return HM_OK;
  DeviceCtx& c = *it->second;
  std::lock_guard<std::mutex> lk2(c.mu);
  (void)hipDeviceSynchronize();
  for (auto& t : c.ntt_tables) ntt_tables_release(*t);
  c.ntt_tables.clear();
  c.ntt_table_bytes = 0;
  xfer_release(c);
  coset_tables_release(c);
  for (auto* list : {&c.bases, &c.zombie_bases}) {
    for (auto& b : *list) {
      if (b.d_xy) (void)hipFree(b.d_xy);
      if (b.d_inf) (void)hipFree(b.d_inf);
    }
    list->clear();
  }
  for (auto& f : c.free_bases) {
    if (f.d_xy) (void)hipFree(f.d_xy);
    if (f.d_inf) (void)hipFree(f.d_inf);
  }
  c.free_bases.clear();
  for (auto& g : c.graphs) graph_release(*g);
  c.graphs.clear();
  for (auto& p : c.poseidon) poseidon_spec_release(*p);
  c.poseidon.clear();
  if (c.batch_streams_ready) {
    for (auto& st : c.batch_streams) (void)hipStreamDestroy(st);
    (void)hipEventDestroy(c.batch_event);
    c.batch_streams_ready = false;
  }
  for (auto& b : c.batch_io) b.release();
  {
    std::lock_guard<std::mutex> lk3(c.live_mu);
    c.live_io.release();
  }
  c.io.release(); c.io_bases.release(); c.conv_bases.release(); c.conv_inf.release();
  c.cached_host_n = 0;
  c.cached_xy = nullptr;
  for (auto& a : c.aux) {
    a.scratch.release();
    a.table.release();
    a.args.release();
    a.work.release();
    if (a.done) (void)hipEventDestroy(a.done);
    a = AuxSlot{};
  }
  for (auto& sl : c.msm_slots) {
    sl.ws.release();
    sl.live_ptr = nullptr;
    sl.busy = false;
    if (sl.h_land) { (void)hipHostFree(sl.h_land); sl.h_land = nullptr; }
    if (sl.ev_ready) { for (auto& e : sl.ev) (void)hipEventDestroy(e); sl.ev_ready = false; }
  }
  return HM_OK;
} HM_API_CATCH("hm_shutdown")

int hm_device_malloc(size_t bytes, void** d_out) try {
  if (!d_out) return hm_fail(HM_ERR_BAD_ARG, "hm_device_malloc: null output");
  *d_out = nullptr;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (bytes == 0) return HM_OK;
  void* p = nullptr;
  hipError_t e = hipSuccess;
#ifdef HM_FAULT_INJECTION      // test build: an armed "device_malloc_oom" makes the FIRST attempt fail like an exhausted device
  try {
    hm_fault_point("device_malloc_oom");
    e = hipMalloc(&p, bytes);
  } catch (const std::exception&) {
    e = hipErrorOutOfMemory;
  }
#else
  e = hipMalloc(&p, bytes);
#endif
  if (e != hipSuccess) {                                  // the library's own caches give back what they can: parked base sets first,
    (void)hipGetLastError();                              // then every cached twiddle / coset table (up to 3 GiB, rebuilt on demand)
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (drop_parked_bases(*ctx)) e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      if (ntt_caches_give_back(*ctx) != 0) e = hipMalloc(&p, bytes);
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return hm_fail(HM_ERR_HIP, std::string("hm_device_malloc: ") + hipGetErrorString(e));
  }
  *d_out = p;
  return HM_OK;
} HM_API_CATCH("hm_device_malloc")

int hm_device_free(void* d_ptr) try {
  if (!d_ptr) return HM_OK;
  if (!ctx_for_current_device()) return HM_ERR_NO_DEVICE;
  HM_HIP_CHECK(hipFree(d_ptr));
  return HM_OK;
} HM_API_CATCH("hm_device_free")

int hm_copy_to_device(void* d_dst, const void* src, size_t bytes) try {
  if (bytes && (!d_dst || !src)) return hm_fail(HM_ERR_BAD_ARG, "hm_copy_to_device: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  // the same ordering whichever way the bytes travel (the lanes' streams are non-blocking; hipMemcpy alone would wait for the
  // default stream and every blocking stream): behind everything queued on the default stream / the blocking streams
  HM_HIP_CHECK(hipStreamSynchronize(nullptr));
  const int rc = xfer_h2d(*ctx, d_dst, src, bytes, "hm_copy_to_device");
  if (rc == HM_OK) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->calls.h2d_bytes += bytes;
  }
  return rc;
} HM_API_CATCH("hm_copy_to_device")

int hm_copy_to_host(void* dst, const void* d_src, size_t bytes) try {
  if (bytes && (!dst || !d_src)) return hm_fail(HM_ERR_BAD_ARG, "hm_copy_to_host: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  HM_HIP_CHECK(hipStreamSynchronize(nullptr));              // (see hm_copy_to_device)
  if (xfer_d2h(*ctx, dst, d_src, bytes, "hm_copy_to_host") != HM_OK)
    return hm_fail(HM_ERR_PARTIAL_OUTPUT, "hm_copy_to_host: the destination is partly written: " + hm_last_error_string());
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->calls.d2h_bytes += bytes;
  return HM_OK;
} HM_API_CATCH("hm_copy_to_host")

static int copy_many(const char* who, bool up, void* const* dev, void* const* host, const size_t* bytes, size_t count) {
  if (count && (!dev || !host || !bytes)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  size_t total = 0;
  for (size_t i = 0; i < count; ++i) {
    if (bytes[i] && (!dev[i] || !host[i])) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null array");
    total += bytes[i];
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (total == 0) return HM_OK;
  HM_HIP_CHECK(hipStreamSynchronize(nullptr));              // the same ordering as hm_copy_to_device / _to_host
  const int rc = xfer_many(*ctx, up, dev, host, bytes, count, who);
  if (rc != HM_OK) return up ? rc : hm_fail(HM_ERR_PARTIAL_OUTPUT, std::string(who) + ": the destinations are partly written: " + hm_last_error_string());
  std::lock_guard<std::mutex> lk(ctx->mu);
  (up ? ctx->calls.h2d_bytes : ctx->calls.d2h_bytes) += total;
  return HM_OK;
}

int hm_copy_many_to_device(void* const* d_dsts, const void* const* srcs, const size_t* bytes, size_t count) try {
  return copy_many("hm_copy_many_to_device", true, d_dsts, const_cast<void* const*>(srcs), bytes, count);
} HM_API_CATCH("hm_copy_many_to_device")

int hm_copy_many_to_host(void* const* dsts, const void* const* d_srcs, const size_t* bytes, size_t count) try {
  return copy_many("hm_copy_many_to_host", false, const_cast<void* const*>(d_srcs), dsts, bytes, count);
} HM_API_CATCH("hm_copy_many_to_host")

int hm_host_register(const void* p, size_t bytes) try {
  if (!ctx_for_current_device()) return HM_ERR_NO_DEVICE;
  return xfer_host_register(p, bytes);
} HM_API_CATCH("hm_host_register")

int hm_host_unregister(const void* p) try {
  if (!ctx_for_current_device()) return HM_ERR_NO_DEVICE;
  return xfer_host_unregister(p);
} HM_API_CATCH("hm_host_unregister")

int hm_device_synchronize(void) try {
  if (!ctx_for_current_device()) return HM_ERR_NO_DEVICE;
  HM_HIP_CHECK(hipDeviceSynchronize());
  return HM_OK;
} HM_API_CATCH("hm_device_synchronize")

int hm_set_host_copies(int mode) try {
  if (xfer_set_policy(mode) != 0) return hm_fail(HM_ERR_BAD_ARG, "hm_set_host_copies: mode must be 0 (auto), 1 (lanes) or 2 (direct)");
  return HM_OK;
} HM_API_CATCH("hm_set_host_copies")

int hm_get_stats(hm_stats* out) try {
  if (!out) return hm_fail(HM_ERR_BAD_ARG, "hm_get_stats: null output");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const CallStats& c = ctx->calls;
  std::memset(out, 0, sizeof *out);
  out->msm_calls = c.msm_calls; out->msm_points = c.msm_points;
  out->ntt_calls = c.ntt_calls; out->ntt_elements = c.ntt_elements;
  for (int i = 0; i < 32; ++i) { out->msm_calls_by_log2[i] = c.msm_by_log[i]; out->ntt_calls_by_log2[i] = c.ntt_by_log[i]; }
  out->msm_h2d_us = c.msm_h2d_us; out->msm_device_us = c.msm_device_us; out->msm_host_us = c.msm_host_us;
  out->ntt_h2d_us = c.ntt_h2d_us; out->ntt_device_us = c.ntt_device_us; out->ntt_d2h_us = c.ntt_d2h_us;
  out->h2d_bytes = c.h2d_bytes; out->d2h_bytes = c.d2h_bytes;
  for (int i = 0; i < 8; ++i) { out->vector_calls[i] = c.vector_calls[i]; out->vector_elements[i] = c.vector_elements[i]; }
  out->coset_table_bytes = ctx->coset_table_bytes;
  out->coset_tables = ctx->coset_tables.size();
  out->ntt_table_bytes = ctx->ntt_table_bytes;
  out->ntt_tables = ctx->ntt_tables.size();
  out->host_copies_direct = ctx->xfer.direct.load(std::memory_order_relaxed);
  out->host_copies_staged = ctx->xfer.staged.load(std::memory_order_relaxed);
  out->host_ranges_registered = xfer_host_ranges();
  return HM_OK;
} HM_API_CATCH("hm_get_stats")

int hm_reset_stats(void) try {
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->calls = CallStats{};
  return HM_OK;
} HM_API_CATCH("hm_reset_stats")

#ifdef HM_FAULT_INJECTION
// test build only (libhalo2_mi355x_fi.so; not declared in the public header): the (after + 1)-th passage through the
// named fault point throws std::runtime_error; point == NULL disarms
int hm_test_arm_fault(const char* point, long after) {
  std::lock_guard<std::mutex> lk(g_fault_mu);
  g_fault_name = point ? point : "";
  g_fault_after = point ? after : -1;
  return HM_OK;
}
#endif

}  // extern "C"
