// hm_internal.h -- private declarations shared by the translation units of libhalo2_mi355x.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/halo2_mi355x.h"

namespace hm {

int hm_fail(int code, const std::string& what);  // records the message for hm_last_error(), returns code

#define HM_HIP_CHECK(expr)                                                                          \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return ::hm::hm_fail(HM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)
#define HM_HIP_CHECK_PTR(expr)                                                                      \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) {                                                                         \
      ::hm::hm_fail(HM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
      return nullptr;                                                                               \
    }                                                                                               \
  } while (0)

// ---- the exception barrier of the C ABI ------------------------------------------------------------
// include/halo2_mi355x.h promises "never aborts or throws across the boundary": every extern "C" entry is a
// function-try-block closed by HM_API_CATCH, so a std::bad_alloc / std::system_error / anything else raised under
// it (vector growth, std::string, std::thread creation) comes back as HM_ERR_INTERNAL with the message in
// hm_last_error().  Locks are std::lock_guard (released by the unwinding), helper threads are owned by JoinOnExit.
int hm_guard_fail(const char* entry, const char* what) noexcept;
#define HM_API_CATCH(entry)                                                                         \
  catch (const std::exception& e) { return ::hm::hm_guard_fail(entry, e.what()); }                  \
  catch (...) { return ::hm::hm_guard_fail(entry, nullptr); }

// Fault points: compiled in only for the test build (libhalo2_mi355x_fi.so, -DHM_FAULT_INJECTION), where
// hm_test_arm_fault(point, after) makes the (after + 1)-th passage through the named point throw.  In the product
// build the call is an empty inline function.
#ifdef HM_FAULT_INJECTION
void hm_fault_point(const char* point);
#else
inline void hm_fault_point(const char*) {}
#endif

// Helper threads of a call (digest lanes, per-device workers, the batch waiter): joined on every way out of the
// scope that owns them -- a throw between two spawns must not destroy a joinable std::thread (std::terminate).
struct JoinOnExit {
  std::vector<std::thread> th;
  ~JoinOnExit() {
    for (auto& t : th)
      if (t.joinable()) t.join();
  }
};
// Start `f` on a new thread owned by `pool`; false when no thread can be had (the caller then runs f itself).
template <class F>
inline bool spawn_or_false(JoinOnExit& pool, const char* point, F&& f) {
  try {
    hm_fault_point(point);
    pool.th.emplace_back(std::forward<F>(f));
    return true;
  } catch (...) {
    return false;
  }
}
const std::string& hm_last_error_string();   // the calling thread's message (workers carry theirs back to the caller's thread)

inline double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

#include "ntt_plan.inc"   // what an NTT call asks for, its check and its launch plan (ntt.hip)

// How a cached device table built on one stream reaches the callers on the others (ctx.mu held).  The build kernels run on the stream
// of the call that first needed the table; record() puts `ready` behind them.  Until that event has been seen complete (`published`),
// wait_or_publish() makes a caller on another stream wait for it on the device.
struct Publication {
  hipStream_t build_stream = nullptr;
  hipEvent_t ready = nullptr;
  bool published = false;
  hipError_t wait_or_publish(hipStream_t stream) {      // the hit path
    if (published) return hipSuccess;
    if (hipEventQuery(ready) == hipSuccess) published = true;
    else if (stream != build_stream) return hipStreamWaitEvent(stream, ready, 0);
    return hipSuccess;
  }
  bool record(hipStream_t stream) {                     // the build path; false: the caller drops the table (the failure path)
    if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess) return false;
    build_stream = stream;
    return hipEventRecord(ready, stream) == hipSuccess;
  }
  void release() {
    if (ready) (void)hipEventDestroy(ready);
    ready = nullptr;
  }
};

struct NttTables {
  uint32_t log_n = 0;
  uint64_t omega[4] = {0, 0, 0, 0};
  Publication pub;
  uint32_t* d[NTT_TABLES_MAX] = {};   // the tables of ntt_table_set(log_n), in its order
  size_t bytes = 0;            // device memory of all of the above: the set's byte total
  uint64_t last_use = 0;       // ctx.ntt_table_clock at the last ntt_get_tables hit (LRU)
};

// The powers table of a transform on a coset shift * <omega> (ntt.hip: coset_table_get): n external words holding
// 32 * shift^i (or 1024 * shift^i for outputs in the evaluator's internal column form).  Built on the first caller's
// stream and published to the others behind `ready`, like the twiddle tables.
struct CosetTable {
  uint64_t shift[4] = {0, 0, 0, 0};
  uint32_t log_n = 0;
  uint32_t internal = 0;
  uint32_t* d = nullptr;
  Publication pub;
  uint64_t last_use = 0;
};

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  void* ensure(size_t bytes) {
    if (bytes <= cap) return p;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    cap = bytes;
    return p;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// xfer.hip: host <-> device copies of the host-pointer entry points through pinned staging the library owns (never the caller's
// pages: see the file's head).  One transfer at a time per device (mu); lanes are created on first use and kept.
constexpr int HM_XFER_LANES = 8;
struct XferLane {
  void* pin[2] = {nullptr, nullptr};      // 2 MiB each, carved from HostXfer::block
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t stream = nullptr;
  double t_wait_us = 0, t_copy_us = 0, t_issue_us = 0, t_start_us = 0;    // of the lane's last share: waiting for DMAs / host memcpy (HALO2_MI355X_XFER_TRACE)
};
struct HostXfer {
  std::mutex mu;
  XferLane lanes[HM_XFER_LANES];
  int ready = 0;
  void* block = nullptr;                  // ONE pinned allocation for every lane's slots (16 separate ones took 49 ms to make)
  void* d_warm = nullptr;                 // 4 KiB of device memory: a new lane's stream is used once in both directions when it is made
  std::atomic<uint64_t> direct{0}, staged{0};   // copies handed to hipMemcpy on the caller's pointers / moved through the lanes (policy: xfer.hip)
};

struct BasesEntry {          // device-resident, converted base set (hm_register_bases)
  uint64_t handle = 0;
  size_t n = 0;
  uint32_t* d_xy = nullptr;  // n x 16 u32: x, y packed internal form
  uint8_t* d_inf = nullptr;  // n flags: base is the identity
  uint32_t pc_c = 0;         // != 0: d_xy holds pc_W * n points, entry j*n + i = 2^(pc_c * j) * P_i
  uint32_t pc_W = 0;
  size_t xy_bytes = 0, inf_bytes = 0;
};

struct MsmStats {
  double t_digits_ms = 0, t_sort_ms = 0, t_accum_ms = 0, t_reduce_ms = 0, t_total_ms = 0, t_accum_kernel_ms = 0;
  uint64_t pairs = 0, tasks = 0;
  uint32_t c = 0, windows = 0;
};

constexpr int HM_MSM_GROUP = 8;   // scalar arrays one launch chain of the five-launch plan carries (msm_small.hip)
#ifndef HM_MSM_SLOTS_N
#define HM_MSM_SLOTS_N 9
#endif
constexpr int HM_MSM_SLOTS = HM_MSM_SLOTS_N;   // slot 0: synchronous calls; 1..8: asynchronous tickets (workspaces allocated on first use)

struct MsmSlot {            // one in-flight MSM: its workspace, events and host landing buffers
  DevBuf ws;
  hipEvent_t ev[7] = {};
  bool ev_ready = false;
  bool busy = false;        // held by a ticket of hm_msm_submit_dev
  bool awaiting = false;    // a thread is inside hm_msm_wait for this ticket (it waits and folds without the context lock)
  bool phase_timed = false; // the MSM in flight recorded its per-phase events (ev[1..3], ev[5..6]), not only ev[0] / ev[4]
  uint64_t ticket = 0;
  uint64_t bases_handle = 0;   // base set the MSM in flight reads (a released set is freed only after its last ticket)
  size_t n = 0;
  hipStream_t stream = nullptr;
  uint32_t* h_land = nullptr;   // pinned host landing zone: 4 totals words, then the window sums (as on the device)
  uint32_t* totals() { return h_land; }
  uint32_t* win() { return h_land + 4; }
  uint32_t SW = 0, c = 0, W = 0;
  uint32_t group = 1;       // MSMs the chain in flight carries (msm_small.hip groups); their results land res_stride words apart
  uint32_t res_stride = 0;
  const uint32_t* live_ptr = nullptr;   // where the last five-launch chain left its (zeroed) block counters; null after any other use of ws
  const uint32_t* d_win = nullptr;   // device locations of the results of the MSM in flight (inside ws)
  const uint32_t* d_tot = nullptr;
  uint64_t T_max = 0;
  bool balanced = false;             // windows of unequal widths (msm_small.hip): the host fold shifts by win_bits[w]
  uint8_t win_bits[128] = {};
  // what msm_finish needs to know of the chain being enqueued: `records` window sums (or one-bit records) per element behind 4 totals
  // words, `stride` words apart, at d_totals; the caller fills win_bits where `balanced_`
  void describe(uint32_t records, uint32_t c_, uint32_t W_, uint32_t group_, uint32_t stride, uint64_t T_max_, const uint32_t* d_totals,
                bool balanced_, bool timed) {
    SW = records, c = c_, W = W_, group = group_, res_stride = stride, T_max = T_max_;
    d_tot = d_totals, d_win = d_totals + 4;
    balanced = balanced_, phase_timed = timed;
  }
};

// Transient device state of the stream-asynchronous entry points (NTT ping-pong buffer, fixed-base
// table): one slot per stream in use, so that calls on different streams never share a buffer.  A slot
// is handed to a new stream only behind the event recorded after its previous user's launches.
struct AuxSlot {
  DevBuf scratch;                 // NTT ping-pong buffer
  DevBuf table;                   // multiples table of hm_g1_fixed_base_mul_dev
  DevBuf args;                    // per-call argument block of hm_graph_evaluate_dev (column table + per-proof constants)
  DevBuf work;                    // hm_quotient_by_cosets_bn256_fr_dev: the columns on the cosets, the numerator's values
  hipStream_t stream = nullptr;   // stream of the last user
  hipEvent_t done = nullptr;      // recorded behind the last user's launches
  bool used = false;
  uint64_t last_use = 0;
};
constexpr int HM_AUX_SLOTS = 4;
// never shrink `table` below the fixed-base table (64 windows x 15 multiples x PT_WORDS u32): the floor of every request for it
constexpr size_t HM_AUX_TABLE_MIN = (size_t)64 * 15 * 28 * 4;
enum class AuxBuf { scratch, table, args, work };

struct GraphVariant {       // the program lowered for one column format (graph.hip: graph_lower)
  void* d_calcs = nullptr;
  uint32_t n_calc = 0, n_slots = 1, result_src = 0, result_prev = 0;
  bool ready = false;
};
struct GraphProgram {       // a compiled evaluate_h program (graph.hip): the validated program + its lowered device forms
  uint64_t handle = 0;
  void* d_blob = nullptr;     // constants + rotations
  uint32_t* d_consts = nullptr;
  int32_t* d_rot = nullptr;
  std::vector<uint32_t> calcs5;      // as given to hm_graph_create
  std::vector<uint64_t> consts_ext;  // its constants as given (graph_run raises the circuits kind's Horner factor to a power on the host)
  uint32_t n_intermediates = 0, n_static = 0, n_dynamic = 0;
  size_t n_columns = 0;
  GraphVariant variant[2];           // [0] external-form columns, [1] internal-form columns (HM_GRAPH_COLUMNS_INTERNAL)
};

struct PoseidonSpec {       // hm_poseidon_create: the constants of one spec on the device, internal form (poseidon.inc's layout)
  uint64_t handle = 0;
  uint32_t width = 0, rate = 0, r_f = 0, r_p = 0;
  uint32_t* d_consts = nullptr;
};

struct FreeBases {          // buffers of a released base set, kept for the next registration of that size
  uint32_t* d_xy = nullptr;
  uint8_t* d_inf = nullptr;
  size_t xy_bytes = 0, inf_bytes = 0;
};

// per-call counters (hm_get_stats): what the shim of INTEGRATION.md reads to replace call-trace estimates
struct CallStats {
  uint64_t msm_calls = 0, msm_points = 0, ntt_calls = 0, ntt_elements = 0;
  uint64_t msm_by_log[32] = {}, ntt_by_log[32] = {};
  double msm_h2d_us = 0, msm_device_us = 0, msm_host_us = 0, ntt_h2d_us = 0, ntt_device_us = 0, ntt_d2h_us = 0;
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
  uint64_t vector_calls[8] = {}, vector_elements[8] = {};    // HM_STAT_* kinds (include/halo2_mi355x.h)
};

struct DeviceCtx {
  int device = 0;
  std::mutex mu;
  std::vector<std::unique_ptr<NttTables>> ntt_tables;   // LRU, bounded by count and bytes (ntt.hip: kNttTablesMax, kNttTableBytesMax)
  size_t ntt_table_bytes = 0;
  uint64_t ntt_table_clock = 0;
  std::vector<std::unique_ptr<CosetTable>> coset_tables;
  uint64_t coset_clock = 0;
  size_t coset_table_bytes = 0;        // HBM held by coset_tables (capped: ntt.hip kCosetTableBytesMax)
  AuxSlot aux[HM_AUX_SLOTS];
  uint64_t aux_clock = 0;
  HostXfer xfer;          // pinned staging lanes of the host-pointer forms' copies (xfer.hip)
  DevBuf io;              // staging for host-pointer calls (scalars / NTT array)
  DevBuf io_bases;        // staging for raw external bases of host-pointer MSM calls
  DevBuf conv_bases;      // converted bases of un-registered calls
  DevBuf conv_inf;
  MsmSlot msm_slots[HM_MSM_SLOTS];   // MSM workspaces (digits, sort scratch, sorted indices, bucket sums ...)
  uint64_t next_ticket = 1;
  std::vector<BasesEntry> bases;
  std::vector<BasesEntry> zombie_bases;   // released while a ticket still reads them: freed by the last hm_msm_wait
  std::vector<FreeBases> free_bases;      // recycled buffers (no hipFree => no device-wide synchronisation)
  std::vector<std::unique_ptr<GraphProgram>> graphs;
  std::vector<std::unique_ptr<PoseidonSpec>> poseidon;   // live specs: freed by hm_poseidon_destroy / hm_shutdown only, never by a give-back
  hipStream_t batch_streams[HM_MSM_SLOTS - 1] = {};   // hm_msm_batch_bn256_g1_dev: one per asynchronous slot
  hipEvent_t batch_event = nullptr;
  bool batch_streams_ready = false;
  DevBuf batch_io[HM_MSM_SLOTS - 1];                  // hm_msm_batch_bn256_g1_h: per-lane staging of host scalar arrays
  DevBuf live_io;                                     // msm_count_live_blocks: column pointers in, block counts out
  std::mutex live_mu;                                 // ... one counting call at a time (never taken under mu)
  std::mutex batch_h_mu;                              // ... which belong to ONE _h batch call at a time (taken before mu, never under it)
  uint64_t next_handle = 1;
  // drop-in MSM: the converted bases of the previous call, keyed by a digest of the WHOLE host array (capi_msm.hip, digest.hip)
  size_t cached_host_n = 0;
  const void* cached_xy = nullptr;
  uint64_t cached_digest[4] = {0, 0, 0, 0};
  MsmStats last_msm;
  CallStats calls;
  bool msm_attr_set = false, ntt_attr_set = false, msm_small_attr_set = false, lookup_attr_set = false;
};

// Slot for a call on `stream` (ctx.mu held): the stream's own slot, else a free or finished one, else the
// least recently used one behind a device-side wait for its event.  aux_release records the event.
AuxSlot* aux_acquire(DeviceCtx& ctx, hipStream_t stream);
int aux_release(DeviceCtx& ctx, AuxSlot* slot, hipStream_t stream);
// A call's use of its slot with ONE way out: body(slot) enqueues on `stream`, and the slot's event is recorded behind whatever it
// enqueued, whatever it returns or throws -- a slot left `used` without a recorded event would hand aux_acquire's hipEventQuery /
// hipStreamWaitEvent a null or stale event.  Refuse arguments before this, not inside.  Nesting on ONE stream is intended: a body's
// own calls on `stream` (the quotient's transforms and numerator) are handed the same slot and use other buffers of it.
template <class Body>
int aux_scope(DeviceCtx& ctx, hipStream_t stream, Body&& body) {
  AuxSlot* slot = aux_acquire(ctx, stream);
  if (!slot) return HM_ERR_HIP;
  int rc;
  try { rc = body(*slot); } catch (...) { (void)aux_release(ctx, slot, stream); throw; }
  const int released = aux_release(ctx, slot, stream);
  return rc != HM_OK ? rc : released;
}
// The slot's buffer of at least `bytes` (`table`: HM_AUX_TABLE_MIN); null, and "<who>: scratch allocation failed", when it cannot be had.
void* aux_buffer(AuxSlot& slot, AuxBuf which, size_t bytes, const char* who);
// The other way to per-call scratch (there are these two): stream-ordered memory of `bytes` (0: none) for body(uint8_t* ws), freed behind
// what the body enqueued, whatever it returns or throws.  The body's code, or the free's failure when the body succeeded.
bool stream_scratch_alloc(const char* who, size_t bytes, hipStream_t stream, uint8_t** ws);      // false: the message is set
int stream_scratch_free(const char* who, uint8_t* ws, hipStream_t stream, int rc);
template <class Body>
int stream_scratch(const char* who, size_t bytes, hipStream_t stream, Body&& body) {
  uint8_t* ws = nullptr;
  if (!stream_scratch_alloc(who, bytes, stream, &ws)) return HM_ERR_HIP;
  int rc;
  try { rc = body(ws); } catch (...) { (void)stream_scratch_free(who, ws, stream, HM_ERR_INTERNAL); throw; }
  return stream_scratch_free(who, ws, stream, rc);
}

DeviceCtx* ctx_for_current_device();     // capi.hip; null (and the message set) without a gfx950 device

// xfer.hip.  Synchronous; the device side must be idle on the range (the callers synchronise their stream first).  May be called
// with or without ctx.mu held (takes ctx.xfer.mu, never ctx.mu).  d2h failures leave `dst` partly written.
int xfer_h2d(DeviceCtx& ctx, void* d_dst, const void* src, size_t bytes, const char* who);
int xfer_d2h(DeviceCtx& ctx, void* dst, const void* d_src, size_t bytes, const char* who);
// `count` arrays as ONE job of the lanes (hm_copy_many_to_device / _to_host): dev[i] <-> host[i], bytes[i] each
int xfer_many(DeviceCtx& ctx, bool up, void* const* dev, void* const* host, const size_t* bytes, size_t count, const char* who);
void xfer_release(DeviceCtx& ctx);
void xfer_prefault(void* p, size_t bytes);      // first-touch a fresh destination from helper threads (contents kept)
int xfer_set_policy(int mode);                  // 0 auto, 1 lanes, 2 direct; -1 on anything else
int xfer_mode(const void* host, size_t bytes);  // which way a copy of this host range goes NOW: 0 = hipMemcpy on the caller's pointers, 1 = the library's pinned lanes
int xfer_host_register(const void* p, size_t bytes);   // hm_host_register / hm_host_unregister: ranges the caller declares long-lived
int xfer_host_unregister(const void* p);
size_t xfer_host_ranges();

// The round trip of a host-pointer form through ctx.io, the ONE implementation of the drop-in contract's ordering (xfer.hip).  The
// caller holds ctx.mu and lays the staging buffer out itself: `at` is a byte offset into it, outputs may alias inputs (the in-place
// forms) and may download less than the device holds.  In order: fault point "<fault_prefix>_upload" (none when null), the staging
// allocation, the uploads, launch(staging) on the null stream (a non-zero code goes back as it is), the stream synchronisation, fault
// point "<fault_prefix>_download" (when there is an output), the buffered outputs into a local buffer (a failure returns its plain
// code: nothing of the caller's is written yet), the direct outputs (a failure is HM_ERR_PARTIAL_OUTPUT), the buffered outputs to
// their destinations.  Only then do ctx.calls.h2d_bytes / d2h_bytes grow, by the bytes copied.
struct HostIn { const void* src; size_t bytes, at; };
struct HostOut { void* dst; size_t bytes, at; bool buffered; };      // buffered: small (a root, an instance); bytes == 0: skipped
struct HostSpans { double h2d_us = 0, device_us = 0, d2h_us = 0; };
using HostLaunch = std::function<int(uint8_t* staging)>;
int host_round_trip(const char* who, DeviceCtx& ctx, const char* fault_prefix, size_t staging_bytes, const HostIn* in, size_t n_in,
                    const HostOut* out, size_t n_out, const HostLaunch& launch, HostSpans* spans = nullptr);
inline size_t pad64(size_t bytes) { return (bytes + 63) / 64 * 64; }

// capi_msm.hip: the one-device bodies the multi-device layer runs per part (Jacobian results, so that partials fold)
int msm_h_local(uint64_t handle, size_t offset, const uint64_t* scalars, size_t n, uint64_t jac[12], int* is_id);
std::vector<int> msm_device_list();            // copy of hm_set_msm_devices' list (empty: one device)
constexpr size_t kMinShardPoints = 1 << 14;    // below this many points per device a split only adds latency
constexpr size_t kSliceBasesFrom = (size_t)1 << 22;   // base sets from this size are SLICED over the devices, smaller ones replicated
bool drop_parked_bases(DeviceCtx& ctx);        // hipFree every parked base buffer (an allocation failed); true when there was anything; ctx.mu held
// digest.hip: keyed digest over EVERY word of n external points -> out = { poly1, poly2, words, parts }
void digest_bases(const uint64_t* bases, size_t n, uint64_t out[4]);

// multi.hip: single-process multi-GPU layer over the one-device entry points (hm_set_msm_devices).  A handle with
// HM_MULTI_HANDLE_BIT names a base set registered on several devices; every form that takes a handle dispatches on it.
constexpr uint64_t HM_MULTI_HANDLE_BIT = 1ull << 62;
inline bool is_multi_handle(uint64_t h) { return (h & HM_MULTI_HANDLE_BIT) != 0; }
// fn(r) for every part r, part r on device devs[r] from its own host thread (the calling thread runs the parts no thread
// could be had for); the first failure is reported on the caller's thread.  Nothing escapes a worker.
int run_per_device(const std::vector<int>& devs, const std::function<int(size_t)>& fn);
bool& multi_worker_flag();                     // true on a thread that is running a part (registrations there stay on one device)
int multi_register(const uint64_t* bases_host, const void* d_bases, size_t n, void* stream, int layout, const std::vector<int>& devs,
                   uint64_t* out_handle);
int multi_bases_info(uint64_t handle, hm_bases_info* out);   // sums over the parts
int multi_release(uint64_t handle);
void multi_release_touching(int device);       // hm_shutdown: drop every multi handle with a part on `device`
int multi_msm(uint64_t handle, size_t offset, const void* scalars, bool from_host, size_t n, void* stream, uint64_t jac[12], int* is_id);
int multi_msm_batch(uint64_t handle, size_t offset, const void* const* scalars, bool from_host, size_t n, size_t count, void* stream,
                    uint64_t* out_xyz);
int multi_local_part(uint64_t handle, int device, uint64_t* local_handle);   // replicated sets: the copy on `device`

// ntt.hip
// What the driver reads beside the NttCall (ntt_plan.inc).  d_a: the arrays of the call, transformed in place, or written from d_in
// when that is set.  The constants are external (4 x u64 Montgomery) words on the HOST, each present iff its NTT_F_* bit is set; they
// travel to the kernels by value, so no call shares a constants buffer with another.  shifts: 4 words per coset table of the call (one,
// fwd_cosets or inv_cosets); the tables themselves are the driver's (a bounded cache); internal: the forward tables hold 1024 * shift^i,
// so that the outputs are in the evaluator's internal column form (HM_GRAPH_COLUMNS_INTERNAL).
struct NttPointers {
  uint32_t* d_a = nullptr;
  const uint32_t* d_in = nullptr;
  const uint64_t* omega = nullptr;    // 4 words
  const uint64_t* scale = nullptr;    // 4 words
  const uint64_t* coset = nullptr;    // 12 words
  const uint64_t* post3 = nullptr;    // 12 words
  const uint64_t* shifts = nullptr;
  bool internal = false;
};
inline NttCall ntt_bind(NttCall c, const NttPointers& p) {       // the call's addresses are the pointers': never stated twice
  c.out = (uintptr_t)p.d_a, c.in = (uintptr_t)p.d_in, c.in_place = p.d_in == nullptr;
  return c;
}
// The one driver: the check (HM_ERR_BAD_ARG with the reason), the plan, the twiddle and coset tables, the fused constants, then the
// launches -- inside aux_scope when the plan has scratch.
int ntt_run(DeviceCtx& ctx, const NttCall& call, const NttPointers& p, hipStream_t stream);
int fr_scale_run(uint32_t* d_a, const uint64_t c_ext[4], uint64_t n, hipStream_t stream);
int fr_mul_pattern3_run(uint32_t* d_a, const uint64_t c3_ext[12], uint64_t n, hipStream_t stream);
void ntt_tables_release(NttTables& t);
void coset_tables_release(DeviceCtx& ctx);
size_t ntt_caches_give_back(DeviceCtx& ctx);   // every cached twiddle / coset table freed (after a device synchronise); bytes given back

// graph.hip
int graph_create(DeviceCtx& ctx, const uint32_t* calcs5, size_t n_calc, const uint64_t* constants_ext, size_t n_const_static,
                 size_t n_dynamic, const int32_t* rotations, size_t n_rot, size_t n_columns, uint32_t n_intermediates,
                 uint64_t* out_handle);
struct GraphCall;                // graph_lower.h: what one call asks for
uint32_t graph_max_blocks();     // HALO2_MI355X_GRAPH_BLOCKS (default 1280), at least 1: the grid cap of every interpreter launch
int graph_run(DeviceCtx& ctx, GraphProgram& g, const GraphCall& call, hipStream_t stream);     // single, circuits or proofs: graph_lower.h
void graph_release(GraphProgram& g);

// poly.hip
int fr_powers_run(uint32_t* d_out, uint64_t n, const uint64_t x_ext[4], hipStream_t stream);
int fr_dot_run(DeviceCtx& ctx, const uint32_t* d_a, const uint32_t* d_b, uint64_t n, uint64_t out_ext[4], hipStream_t stream);
int fr_affine_sequence_run(uint32_t* d_out, uint64_t n, const uint64_t a_ext[4], const uint64_t b_ext[4], hipStream_t stream);
int fr_random_run(uint32_t* d_out, uint64_t n, uint64_t seed, hipStream_t stream);
int fr_eval_polynomial_run(DeviceCtx& ctx, const uint32_t* d_polys, uint64_t n, const uint32_t* poly_index, const uint64_t* points_ext,
                           size_t q, uint64_t* out_ext, hipStream_t stream);

// polyops.hip
int fr_kate_division_run(DeviceCtx& ctx, const uint32_t* d_a, uint64_t n, const uint64_t z_ext[4], uint32_t* d_q, hipStream_t stream);
int fr_grand_product_run(DeviceCtx& ctx, const uint32_t* d_m, uint64_t n, const uint64_t start_ext[4], uint32_t* d_out, hipStream_t stream);
int fr_shplonk_set_quotient_run(const void* const* d_polys, const uint64_t* weights_ext, size_t m, uint64_t n, const uint64_t* points_ext,
                                uint32_t t, const uint64_t scale_ext[4], uint32_t* d_out, bool accumulate, hipStream_t stream);
int fr_kate_division_batch_run(DeviceCtx& ctx, const void* const* d_a, uint64_t n, const uint64_t* z_ext, void* const* d_q, size_t count,
                               hipStream_t stream);
int fr_grand_product_batch_run(DeviceCtx& ctx, const void* const* d_m, uint64_t n, const uint64_t start_ext[4], uint64_t chain_row,
                               void* const* d_out, size_t count, hipStream_t stream);
int fr_batch_invert_run(uint32_t* d_v, uint64_t n, hipStream_t stream);
int fr_mul_periodic_run(uint32_t* d_a, uint64_t n, const uint64_t* pattern_ext, uint32_t period, hipStream_t stream);
int fr_linear_combination_run(const void* const* d_polys, const uint64_t* coeffs_ext, size_t count, uint64_t n, uint32_t* d_out,
                              hipStream_t stream);
// the same for `proofs` independent proofs in one launch chain (blockIdx.y = the proof); nullptr, or why the pointers are refused
const char* fr_batch_alias_check(const void* const* d_polys, size_t count, void* const* d_outs, size_t proofs);
int fr_linear_combination_batch_run(const void* const* d_polys, const uint64_t* coeffs_ext, size_t count, uint64_t n, void* const* d_outs,
                                    size_t proofs, hipStream_t stream);
int fr_shplonk_set_quotient_batch_run(const void* const* d_polys, const uint64_t* weights_ext, size_t m, uint64_t n, const uint64_t* points_ext,
                                      uint32_t t, const uint64_t* scales_ext, void* const* d_outs, bool accumulate, size_t proofs,
                                      hipStream_t stream);
// keygen's sigma columns: d_out[c] = delta^j' * omega^i' (external words) for d_sigma_cells[c] = j' * 2^k + i'
int perm_columns_run(const uint32_t* d_sigma_cells, uint32_t columns, uint32_t k, const uint64_t omega_ext[4], const uint64_t delta_ext[4],
                     uint32_t* d_out, hipStream_t stream);

// poseidon.hip: Poseidon and Merkle trees.  Everything is asynchronous on `stream`; pointers are device memory of u32 words.
int poseidon_spec_create(DeviceCtx& ctx, uint32_t width, uint32_t rate, uint32_t r_f, uint32_t r_p, const uint64_t* rc_ext,
                         const uint64_t* mds_ext, uint64_t* out_handle);
void poseidon_spec_release(PoseidonSpec& s);
// digest i of the rate consecutive elements at d_in + i * in_stride words -> d_out + i * out_stride words
int poseidon_hash_run(const PoseidonSpec& s, const uint32_t* d_in, uint64_t in_stride, uint32_t* d_out, uint64_t out_stride, size_t n,
                      hipStream_t stream);
// levels 1 .. depth of a tree whose level 0 (2^depth nodes) is already at the start of d_nodes; width 5: (hash, balance) nodes
// with the balances summed, width 3: one hash per node
int merkle_build_run(const PoseidonSpec& s, uint32_t* d_nodes, uint32_t depth, hipStream_t stream);
int merkle_paths_run(const uint32_t* d_nodes, uint32_t depth, uint32_t words_per_node, const uint64_t* d_indices, size_t m,
                     uint32_t* d_out, hipStream_t stream);
// the built tree updated in place: entry p sets leaf d_indices[p] to element p of d_new_leaves, in array order (the last entry of an
// index wins, an index >= 2^depth is dropped); d_counts: null, or depth + 1 words: live entries, nodes hashed at levels 1 .. depth
int merkle_update_run(const PoseidonSpec& s, uint32_t* d_nodes, uint32_t depth, const uint64_t* d_indices, const uint32_t* d_new_leaves,
                      size_t m, uint32_t* d_counts, hipStream_t stream);
// the roots of m paths (siblings as merkle_paths_run writes them); the spec's width selects the elements per node
int merkle_roots_run(const PoseidonSpec& s, uint32_t depth, size_t m, const uint32_t* d_leaves, const uint32_t* d_siblings,
                     const uint64_t* d_indices, uint32_t* d_roots, hipStream_t stream);
// ascending bitonic sort of n_pow2 64-bit keys in place (the Merkle update's network; keygen.hip sorts its endpoint keys with it)
int merkle_update_sort(uint64_t* d_keys, uint64_t n_pow2, hipStream_t stream);
// The witnesses of the three circuits.  E, the elements per node, selects the circuit: 2 MerkleSumTree, 1 MerkleTreeV3,
// 0 the Poseidon circuit (depth is ignored; its level_rows counts every row before the constants).
// out = rows_used, n_advice, perm_rows, level_rows, lt_row (E = 2 only), const_row
void witness_rows(uint32_t E, uint32_t depth, uint32_t r_f, uint32_t r_p, uint32_t (&out)[6]);
// E = 2 or 1; assets_ext is read for E = 2 only; d_nodes: the built tree, or null
int merkle_witness_run(uint32_t E, const PoseidonSpec& s, uint32_t depth, uint32_t log_n, size_t m, const uint32_t* d_leaves,
                       const uint32_t* d_siblings, const uint64_t* d_indices, const uint64_t* assets_ext, const uint32_t* d_nodes,
                       uint32_t* d_advice, uint32_t* d_instance, hipStream_t stream);
int poseidon_witness_run(const PoseidonSpec& s, uint32_t log_n, size_t m, const uint32_t* d_msgs, uint32_t* d_advice, uint32_t* d_instance,
                         hipStream_t stream);

// range.hip: the range-check circuit's witness: column 0 the m x rows values, columns 1 .. acc_cols their limbs of max_bits bits, most
// significant first; every row of every column is written; d_over: null, or m counters of the values with higher bits.  Asynchronous
// on `stream`; the arguments were checked by the caller (capi_hash.hip).
int range_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_values,
                      uint32_t* d_advice, uint32_t* d_over, hipStream_t stream);

// sorted.hip: the sorted-column circuit's witness: column 0 the m x rows ids, columns 1 .. acc_cols the limbs of id[i+1] - id[i] - 1
// mod r on rows 0 .. rows - 2, most significant first; every row of every column is written; d_over: null, or m counters of the gaps
// with higher bits.  Asynchronous on `stream`; the arguments were checked by the caller (capi_hash.hip).
int sorted_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_ids,
                       uint32_t* d_advice, uint32_t* d_over, hipStream_t stream);
// d_perm[0 .. n): the rows of the n canonical Montgomery elements of d_values in the order of their canonical integers, equal
// elements by ascending row.  Asynchronous on `stream`, stream-ordered scratch of its own; 1 <= n <= 2^26 checked by the caller.
int fr_argsort_run(const uint32_t* d_values, size_t n, uint64_t* d_perm, hipStream_t stream);
// its launch chain on the caller's scratch: d_keys (n_pow2 x 8 words) and d_rows (n_pow2 words) leave as the sorted records, n_pow2
// the next power of two of n; d_perm (n rows widened to 64 bits) may be null
int fr_sort_records_run(const uint32_t* d_values, uint64_t n, uint64_t n_pow2, uint32_t* d_keys, uint32_t* d_rows, uint64_t* d_perm,
                        hipStream_t stream);

// logup.hip: the logUp lookup argument's multiplicity columns and running sums; the arguments were checked by
// the caller (capi_poly.hip).  logup_multiplicities_run synchronises `stream` (it reads the key bits and the missing flags back);
// fr_grand_sum_batch_run is asynchronous on it.
int logup_multiplicities_run(const void* const* d_tables, const void* const* d_inputs, const uint32_t* input_counts, size_t count, uint64_t rows,
                             void* const* d_m, int* missing, hipStream_t stream);
int fr_grand_sum_batch_run(const void* const* d_terms, uint64_t n, void* const* d_out, size_t count, hipStream_t stream);

// accumulator.hip: the SafeAccumulator circuit's witness: m running totals of acc_cols limbs of max_bits bits (max_bits * acc_cols <= 64),
// row 0 the initial limbs, row r the value r, the top limb's inverse, the carries and the limbs after adding it; every row of every
// column is written.  inverses_ext: HOST memory, the 2^max_bits - 1 inverses of 1 .. 2^max_bits - 1 (host_fr.h: fr_small_inverses);
// d_finals: m x acc_cols plain limbs; d_over: null, or m counters of the failing rows.  Asynchronous on `stream`, stream-ordered
// scratch of its own; the arguments were checked by the caller (capi_hash.hip).  part_ms: null, or 4 doubles for the device times of
// the four launches (reduce, scan, rows, count); the call then waits for `stream`.
int accumulator_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_values,
                            const uint64_t* d_initial, const uint64_t* inverses_ext, uint32_t* d_advice, uint64_t* d_finals, uint32_t* d_over,
                            hipStream_t stream, double* part_ms = nullptr);

// keygen.hip: keygen's permutation assembly.  d_copies: m pairs of cell ids, a cell being column * 2^k + row; d_sigma_cells receives
// columns * 2^k ids (it is the union-find's parent array on the way); a pair with an id out of range is dropped and counted in
// *d_dropped (null: not counted).  Asynchronous on `stream`; the arguments were checked by the caller (capi_keygen.hip).
int perm_assemble_run(const uint32_t* d_copies, size_t m, uint32_t columns, uint32_t k, uint32_t* d_sigma_cells, uint32_t* d_dropped,
                      hipStream_t stream);

// lookup.hip
int lookup_permute_run(DeviceCtx& ctx, const void* const* d_inputs, const void* const* d_tables, size_t pairs, uint64_t rows,
                       void* const* d_out_inputs, void* const* d_out_tables, int* missing, hipStream_t stream);

// the sorted canonical keys of the first `live` (>= 1) elements of d_values, for a binary search (mock.hip): d_ws, of
// lookup_sorted_keys_bytes(live) bytes and 256-byte aligned, starts with the keys -- the next power of two of them, all-ones behind
// the live ones.  Asynchronous on `stream`.
size_t lookup_sorted_keys_bytes(uint64_t live);
int lookup_sorted_keys_run(DeviceCtx& ctx, const uint32_t* d_values, uint64_t live, uint8_t* d_ws, hipStream_t stream);

// mock.hip: the batched witness checker.  MockTable: per column of the program's table its base, the words from one user's column
// to the next user's (0: shared) and the rows present (cells above read as zero) -- HOST arrays.  MockSink: where failures go, all
// DEVICE memory of the caller's: `cap` records, one counter that keeps counting past cap, one byte per user.
struct MockTable { const void* const* bases; const uint64_t* strides; const uint32_t* rows; size_t n; };
struct MockSink { uint64_t* d_records; uint64_t cap; uint64_t* d_counter; uint8_t* d_user_flags; };
// program `g` on the (user, row < usable) lanes of m users, or on the n_list lanes of d_list (records of an earlier pass); a lane
// fails when its value is != 0, or, with d_table_values (2^k elements of which the first `usable` are the table), when its value
// is not in the table.  The arguments were checked by the caller (capi_mock.hip).
int mock_program_run(DeviceCtx& ctx, GraphProgram& g, const MockTable& t, const uint64_t* dyn_ext, size_t n_dyn, uint32_t k,
                     uint32_t usable, size_t m, uint32_t user_base, const uint64_t* d_list, size_t n_list, const uint32_t* d_table_values,
                     const MockSink& out, hipStream_t stream);
// d_pairs: n_copies pairs of cell ids (permutation column j * 2^k + row); perm[j]: the table entry that column is
int mock_copies_run(DeviceCtx& ctx, const MockTable& t, const uint32_t* perm, size_t n_perm, const uint32_t* d_pairs, size_t n_copies,
                    uint32_t k, size_t m, const MockSink& out, hipStream_t stream);

// msm.hip
int msm_convert_bases(const uint32_t* d_bases_ext, uint32_t* d_xy, uint8_t* d_inf, size_t n, hipStream_t stream);
// out_windows: host buffer of W x 12 u64 external Jacobian + flags
int msm_enqueue(DeviceCtx& ctx, int slot, const uint32_t* d_scalars_ext, const uint32_t* d_xy, const uint8_t* d_inf, size_t n,
                uint32_t precomp_c, hipStream_t stream);
// `group` dense MSMs over one fixed-base table through one chain of the general pipeline (msm.hip); 1 when it does not apply
uint32_t msm_table_group_max(size_t n, uint32_t precomp_c);
int msm_enqueue_table_group(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                            const uint8_t* d_inf, size_t n, uint32_t precomp_c, hipStream_t stream);
int msm_finish(DeviceCtx& ctx, int slot, uint64_t out_jac_ext[12], int* out_is_identity);
// the two halves of msm_finish: the blocking part touches only the slot (callable without ctx.mu while the slot is
// busy), the bookkeeping part runs under ctx.mu
int msm_finish_wait_fold(MsmSlot& sl, uint64_t* out_jac_ext /* 12 words per MSM of the group */, int* out_is_identity /* one per MSM */,
                         double* host_us);
void msm_finish_record(DeviceCtx& ctx, int slot, double host_us);
bool msm_phase_timing(bool small_plan);    // hm_msm_set_phase_timing: -1 auto (general pipeline only), 0 never, 1 always
int msm_slot_prepare(MsmSlot& sl);   // events + pinned landing zone, on first use
// msm_small.hip: the five-launch chain for n < 2^19 (plain base sets, c <= 15)
int msm_issue_small(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                    const uint8_t* d_inf, size_t n, uint32_t c, hipStream_t stream);
// live_out[i] = how many 256-row blocks of column i hold a row that survives the digits kernel's compaction (a non-zero
// scalar on a non-identity base); synchronises `stream` (one small copy).  Decides the grouping of a phase of commitments.
int msm_count_live_blocks(DeviceCtx& ctx, const void* const* d_columns, size_t count, const uint8_t* d_inf, size_t n, hipStream_t stream,
                          uint32_t* live_out);
// a group of MSMs over the same points through one chain (only where the five-launch plan applies: msm_group_applies)
bool msm_group_applies(size_t n, uint32_t precomp_c);
int msm_enqueue_group(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                      const uint8_t* d_inf, size_t n, hipStream_t stream, size_t live_rows = 0);
int msm_run(DeviceCtx& ctx, const uint32_t* d_scalars_ext, const uint32_t* d_xy, const uint8_t* d_inf, size_t n,
            uint32_t precomp_c, uint64_t out_jac_ext[12], int* out_is_identity, hipStream_t stream);
uint32_t msm_precomp_window(size_t n);
int msm_precompute(uint32_t* d_table, const uint8_t* d_inf, size_t n, uint32_t c, uint32_t W, hipStream_t stream);
void host_sum_points(const uint64_t* pts, size_t count, uint64_t out_jac_ext[12], int* out_is_identity);
int g1_fixed_base_mul_run(DeviceCtx& ctx, const uint32_t* d_scalars_ext, size_t n, const uint64_t base_affine_ext[8],
                          uint32_t* d_out_affine_ext, hipStream_t stream);

// g1_fft.hip
// best_fft over G1 in place on n = 2^log_n <= 2^24 points of `words` u32 each: 16 affine external ((0, 0) = identity) or 24
// Jacobian external (z = 0 = identity; outputs (x, y, 1) / zeros).  scale_ext: optional Fr Montgomery words multiplied into every output.
int g1_fft_run(DeviceCtx& ctx, uint32_t* d_points, uint32_t words, const uint64_t omega_ext[4], uint32_t log_n,
               const uint64_t* scale_ext, hipStream_t stream);
// All KZG openings of a polynomial on its domain (FK20), n = 2^log_n <= 2^23, asynchronous on `stream`.  table: the
// G1 FFT of size 2n of the reversed first n monomial points (16-word affine external, (0, 0) = identity), written from them by
// kzg_open_table_run; open_all: `count` polynomials of n x 8 Fr words back to back -> count x n affine proofs, proof t the opening at
// omega_n^t.  part_ms: null, or 7 doubles for the step times of the last polynomial (the call then waits for `stream`).
int kzg_open_table_run(DeviceCtx& ctx, const uint32_t* d_g_xy, uint32_t log_n, uint32_t* d_table_xy, hipStream_t stream);
int kzg_open_all_run(DeviceCtx& ctx, const uint32_t* d_table_xy, const uint32_t* d_coeffs, uint32_t log_n, size_t count,
                     uint32_t* d_proofs_xy, hipStream_t stream, double* part_ms = nullptr);

// ledger.hip: the pair (pi_b, -R_b) of every user's ledger opening check, one lane per user (ledger.inc): 2 rows of affine Montgomery
// words per user at d_g1 and one flag word at d_flags.  gamma, omega (the 2^log_n-th root of unity) and c_gamma are host words.
// Arguments checked by the caller, the word arrays with kzg_ledger_words_problem (null: nothing wrong); one launch, asynchronous on `stream`.
const char* kzg_ledger_words_problem(const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8]);
int kzg_ledger_pairs_run(const uint32_t* d_openings, const uint32_t* d_indices, const uint32_t* d_ids, const uint32_t* d_balances,
                         const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8], uint32_t log_n, uint32_t assets,
                         size_t users, uint32_t* d_g1, uint32_t* d_flags, hipStream_t stream);

// g1_codec.hip: SRS point encodings: 16-word affine external points <-> 8-word compressed encodings.  compress is asynchronous;
// decompress / check wait for `stream` and answer HM_ERR_INVALID_DATA with the smallest invalid index in *first_invalid (n if none).
int g1_compress_run(const uint32_t* d_xy, size_t n, uint32_t* d_out32, hipStream_t stream);
int g1_decompress_run(const uint32_t* d_in32, size_t n, uint32_t* d_xy, uint64_t* first_invalid, hipStream_t stream);
int g1_check_run(const uint32_t* d_xy, size_t n, uint64_t* first_invalid, hipStream_t stream);

// verify.hip: the device side of a batch verification
// A batch of proofs: every 32-byte slot of n_proofs proofs read by the kinds of the device table (points decompressed,
// scalars checked), and the sum of rows [lo, hi) of every column of a (rows, cols) array of Fr words.  Both asynchronous on `stream`.
int verify_read_run(const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                    uint32_t n_points, uint32_t n_scalars, uint32_t* d_points, uint32_t* d_tail, uint32_t* d_ybytes, uint32_t* d_scalars,
                    uint32_t* d_bad, hipStream_t stream);
int verify_colsum_run(const uint32_t* d_rows, uint32_t cols, size_t lo, size_t hi, uint32_t* d_out, hipStream_t stream);
// r_b x the scalars of every proof of a batch, one lane per proof; `plan` (host memory) is checked word by word before anything is
// launched and uploaded with the call.  Asynchronous on `stream`.
int verify_terms_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                     const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst, uint32_t* d_bad, uint32_t* d_own,
                     uint32_t* d_shared, uint32_t* d_h2r, uint32_t* d_h2l, hipStream_t stream);
// The same for proofs of `circuits` circuits each (create_proof_multi): one wavefront per proof, lane c is circuit c; `plan` is the
// multi plan (verify_terms.inc, vtm_plan_problem).  Asynchronous on `stream`.
int verify_terms_multi_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic,
                           size_t n_proofs, uint32_t circuits, const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst,
                           uint32_t* d_bad, uint32_t* d_own, uint32_t* d_shared, uint32_t* d_h2r, uint32_t* d_h2l, hipStream_t stream);
// The same for proofs that end in the GWC multiopen, one lane per proof: `plan` is a GWC plan (verify_terms.inc, vg_plan_problem),
// the records hold 8 elements, d_w_left (n_proofs x q x 4 words) receives r_b u^i.  Asynchronous on `stream`.
int verify_terms_gwc_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic,
                         size_t n_proofs, const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst, uint32_t* d_bad,
                         uint32_t* d_own, uint32_t* d_shared, uint32_t* d_w_left, hipStream_t stream);
// The pair (L_b, -R_b) of every proof's own opening check, one workgroup per proof (verify_sums.inc): 2 rows of affine Montgomery
// words per proof, zeros for a proof whose flag is set.  Asynchronous on `stream`.
int verify_sums_run(const uint32_t* d_bases, size_t n_proofs, uint32_t own_points, uint32_t shared_points, const uint32_t* d_own,
                    const uint32_t* d_shared, const uint32_t* d_h2r, const uint32_t* d_h2l, const uint32_t* d_bad, uint32_t* d_pairs,
                    hipStream_t stream);
// Blake2b-512 of n messages at a fixed byte stride (personal16: host memory or null), and the transcripts
// of n_proofs proofs -- `schedule` (host memory, n_pairs pairs) is checked before anything is launched and uploaded with the call.
// Both asynchronous on `stream`.
int blake2b_run(const uint8_t* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, const uint8_t* personal16, uint32_t* d_out,
                hipStream_t stream);
int verify_transcript_run(DeviceCtx& ctx, const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots,
                          uint32_t n_points, const uint32_t* d_ybytes, const uint32_t* d_preamble, const uint32_t* d_counts, uint32_t stride,
                          const uint32_t* schedule, size_t n_pairs, uint32_t* d_bad, uint32_t* d_records, uint32_t record_elems,
                          hipStream_t stream);
// Keccak-256 and the EVM encoding's read and transcripts (keccak.inc), as their Blake2b and compressed siblings above
int keccak256_run(const uint8_t* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, uint32_t* d_out, hipStream_t stream);
int verify_read_evm_run(const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                        uint32_t n_scalars, uint32_t* d_points, uint32_t* d_tail, uint32_t* d_scalars, uint32_t* d_bad, hipStream_t stream);
int verify_transcript_evm_run(DeviceCtx& ctx, const uint32_t* d_proofs, size_t n_proofs, uint32_t slots, const uint32_t* d_preamble,
                              const uint32_t* d_counts, uint32_t stride, const uint32_t* schedule, size_t n_pairs, uint32_t* d_bad,
                              uint32_t* d_records, uint32_t record_elems, hipStream_t stream);

// pairing.hip: the Miller loops of n_pairs pairs, then product and final exponentiation of n_checks checks, in d_work
// (pairing_work_words u32 words); both launches asynchronous on `stream`
size_t pairing_work_words(size_t n_pairs, size_t n_checks);
int pairing_check_run(const uint32_t* d_g1, const uint32_t* d_g2, size_t n_pairs, const uint32_t* d_offsets, size_t n_checks, uint32_t* d_gt,
                      uint32_t* d_status, uint32_t* d_work, hipStream_t stream);

}  // namespace hm
