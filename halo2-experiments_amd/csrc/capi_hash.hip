// capi_hash.hip -- the hashing entry points of the C ABI: Poseidon specs and hashes, Merkle (sum) tree build / paths / update / roots and
// the witnesses of the three circuits (poseidon.inc, polyops.hip).
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "hm_internal.h"
#include "host_fr.h"

using namespace hm;

extern "C" {

static constexpr size_t POSEIDON_MAX_N = (size_t)1 << 31;
static constexpr uint32_t MERKLE_MAX_DEPTH = 30;

int hm_poseidon_create(uint32_t width, uint32_t rate, uint32_t r_f, uint32_t r_p, const uint64_t* round_constants, const uint64_t* mds,
                       uint64_t* out_handle) try {
  if (!round_constants || !mds || !out_handle) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_create: null argument");
  if (width != 3 && width != 5) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_create: width must be 3 or 5");
  if (rate != width - 1) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_create: rate must be width - 1");
  if ((r_f & 1) || r_f > 1024 || r_p > 1024 || r_f + r_p == 0 || r_f + r_p > 1024)
    return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_create: r_f must be even and 0 < r_f + r_p <= 1024");
  for (size_t i = 0, n_rc = (size_t)(r_f + r_p) * width, total = n_rc + (size_t)width * width; i < total; ++i) {
    const uint64_t* w = i < n_rc ? round_constants + i * 4 : mds + (i - n_rc) * 4;
    bool lt = false;
    for (int k = 3; k >= 0; --k)
      if (w[k] != host::FR_MOD[k]) {
        lt = w[k] < host::FR_MOD[k];
        break;
      }
    if (!lt) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_create: a constant is not below the modulus");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return poseidon_spec_create(*ctx, width, rate, r_f, r_p, round_constants, mds, out_handle);
} HM_API_CATCH("hm_poseidon_create")

int hm_poseidon_destroy(uint64_t handle) try {
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (size_t i = 0; i < ctx->poseidon.size(); ++i)
    if (ctx->poseidon[i]->handle == handle) {
      (void)hipDeviceSynchronize();          // a launch may still read the constants (rare call: once per spec)
      poseidon_spec_release(*ctx->poseidon[i]);
      ctx->poseidon.erase(ctx->poseidon.begin() + i);
      return HM_OK;
    }
  return hm_fail(HM_ERR_NOT_FOUND, "hm_poseidon_destroy: unknown spec handle");
} HM_API_CATCH("hm_poseidon_destroy")

static PoseidonSpec* find_poseidon(DeviceCtx& ctx, uint64_t handle) {      // ctx.mu held
  for (auto& p : ctx.poseidon)
    if (p->handle == handle) return p.get();
  return nullptr;
}
// the spec of a tree call: `width` 5 for the sum tree, 3 for the plain tree
static int merkle_spec(const char* who, DeviceCtx& ctx, uint64_t handle, uint32_t width, PoseidonSpec** out) {
  *out = find_poseidon(ctx, handle);
  if (!*out) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown spec handle");
  if ((*out)->width != width)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the spec has width " + std::to_string((*out)->width) + ", this tree needs width " +
                                       std::to_string(width));
  return HM_OK;
}

int hm_poseidon_hash_bn256_fr_dev(uint64_t handle, const void* d_msgs, size_t n, void* d_out, void* stream) try {
  if (n && (!d_msgs || !d_out)) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_hash_bn256_fr_dev: null argument");
  if (n > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_hash_bn256_fr_dev: n > 2^31");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = find_poseidon(*ctx, handle);
  if (!s) return hm_fail(HM_ERR_NOT_FOUND, "hm_poseidon_hash_bn256_fr_dev: unknown spec handle");
  return poseidon_hash_run(*s, (const uint32_t*)d_msgs, (uint64_t)s->rate * 8, (uint32_t*)d_out, 8, n, (hipStream_t)stream);
} HM_API_CATCH("hm_poseidon_hash_bn256_fr_dev")

// Host forms: input and output share one staging buffer; the caller's outputs are written only by the last copies.
int hm_poseidon_hash_bn256_fr(uint64_t handle, const uint64_t* msgs, size_t n, uint64_t* out) try {
  if (n && (!msgs || !out)) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_hash_bn256_fr: null argument");
  if (n > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_hash_bn256_fr: n > 2^31");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = find_poseidon(*ctx, handle);
  if (!s) return hm_fail(HM_ERR_NOT_FOUND, "hm_poseidon_hash_bn256_fr: unknown spec handle");
  if (n == 0) return HM_OK;
  const size_t in_bytes = n * s->rate * 32, out_bytes = n * 32;
  const HostIn in{msgs, in_bytes, 0};
  const HostOut res{out, out_bytes, in_bytes, false};
  return host_round_trip("hm_poseidon_hash_bn256_fr", *ctx, "poseidon", in_bytes + out_bytes, &in, 1, &res, 1, [&](uint8_t* d) {
    return poseidon_hash_run(*s, (const uint32_t*)d, (uint64_t)s->rate * 8, (uint32_t*)(d + in_bytes), 8, n, nullptr);
  });
} HM_API_CATCH("hm_poseidon_hash_bn256_fr")

static int merkle_build_dev(const char* who, uint64_t handle, uint32_t width, const void* d_leaves, uint32_t depth, void* d_nodes,
                            void* stream) {
  if (!d_leaves || !d_nodes) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": depth > 30");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  if (int rc = merkle_spec(who, *ctx, handle, width, &s)) return rc;
  const size_t leaf_bytes = ((size_t)1 << depth) * (width == 5 ? 64 : 32);
  if (d_leaves != d_nodes) {
    if (ranges_overlap(d_leaves, leaf_bytes, d_nodes, 2 * leaf_bytes))
      return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_leaves partially overlaps d_nodes");
    HM_HIP_CHECK(hipMemcpyAsync(d_nodes, d_leaves, leaf_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return merkle_build_run(*s, (uint32_t*)d_nodes, depth, (hipStream_t)stream);
}

int hm_merkle_sum_tree_build_dev(uint64_t handle, const void* d_leaves, uint32_t depth, void* d_nodes, void* stream) try {
  return merkle_build_dev("hm_merkle_sum_tree_build_dev", handle, 5, d_leaves, depth, d_nodes, stream);
} HM_API_CATCH("hm_merkle_sum_tree_build_dev")

int hm_merkle_tree_build_dev(uint64_t handle, const void* d_leaves, uint32_t depth, void* d_nodes, void* stream) try {
  return merkle_build_dev("hm_merkle_tree_build_dev", handle, 3, d_leaves, depth, d_nodes, stream);
} HM_API_CATCH("hm_merkle_tree_build_dev")

int hm_merkle_sum_tree_build(uint64_t handle, const uint64_t* leaves, uint32_t depth, uint64_t* root, uint64_t* nodes_or_null) try {
  if (!leaves || !root) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_sum_tree_build: null argument");
  if (depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_sum_tree_build: depth > 30");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  if (int rc = merkle_spec("hm_merkle_sum_tree_build", *ctx, handle, 5, &s)) return rc;
  const size_t leaf_bytes = ((size_t)1 << depth) * 64, node_bytes = 2 * leaf_bytes - 64;
  const HostIn in{leaves, leaf_bytes, 0};                  // the tree is built in place behind its leaves
  const HostOut out[2] = {{root, 64, node_bytes - 64, true}, {nodes_or_null, node_bytes, 0, false}};
  return host_round_trip("hm_merkle_sum_tree_build", *ctx, "poseidon", node_bytes, &in, 1, out, nodes_or_null ? 2 : 1,
                         [&](uint8_t* d) { return merkle_build_run(*s, (uint32_t*)d, depth, nullptr); });
} HM_API_CATCH("hm_merkle_sum_tree_build")

int hm_merkle_paths_dev(const void* d_nodes, uint32_t depth, uint32_t words_per_node, const uint64_t* d_indices, size_t m, void* d_out,
                        void* stream) try {
  if (m && depth && (!d_nodes || !d_indices || !d_out)) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_paths_dev: null argument");
  if (depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_paths_dev: depth > 30");
  if (words_per_node != 1 && words_per_node != 2) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_paths_dev: words_per_node must be 1 or 2");
  if (m > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, "hm_merkle_paths_dev: m > 2^31");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return merkle_paths_run((const uint32_t*)d_nodes, depth, words_per_node, d_indices, m, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_merkle_paths_dev")

// ---- the witnesses of the three circuits (poseidon.inc: merkle_witness_lane<E>, poseidon_witness_lane) -------------------------------
// E, the elements per node, names the circuit: 2 MerkleSumTree (width 5), 1 MerkleTreeV3 (width 3), 0 the Poseidon circuit (width 5,
// one hash, no levels: depth is ignored)
static constexpr uint32_t WITNESS_MAX_DEPTH = 32, WITNESS_MAX_LOG_N = 24;
static constexpr size_t WITNESS_HOST_MAX_BYTES = (size_t)1 << 28;

// out = rows_used, n_advice, perm_rows, level_rows, lt_row, const_row
static int witness_layout(const char* who, uint32_t E, uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, uint32_t (&out)[6]) {
  if (E && (depth == 0 || depth > WITNESS_MAX_DEPTH)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": depth must be 1 .. 32");
  if ((r_f & 1) || (r_p & 1) || r_f + r_p == 0 || r_f > 1024 || r_p > 1024)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the Pow5 chip needs even r_f and r_p");
  if (log_n > WITNESS_MAX_LOG_N) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": log_n > 24");
  witness_rows(E, depth, r_f, r_p, out);
  if (((uint64_t)1 << log_n) < (uint64_t)out[0] + 6)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the circuit needs " + std::to_string(out[0]) + " rows, 2^log_n - 6 is fewer");
  return HM_OK;
}

// the hm_*_witness_layout entry points; out_regions: perm_rows, level_rows, (E = 2: lt_row,) const_row
static int witness_layout_api(const char* who, uint32_t E, uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n,
                              uint32_t* out_rows_used, uint32_t* out_n_advice, uint32_t* out_regions) {
  if (!out_rows_used || !out_n_advice) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  uint32_t t[6];
  if (int rc = witness_layout(who, E, r_f, r_p, depth, log_n, t)) return rc;
  *out_rows_used = t[0];
  *out_n_advice = t[1];
  if (out_regions) {
    *out_regions++ = t[2];
    *out_regions++ = t[3];
    if (E == 2) *out_regions++ = t[4];
    *out_regions = t[5];
  }
  return HM_OK;
}

int hm_merkle_sum_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, uint32_t* out_rows_used,
                                 uint32_t* out_n_advice, uint32_t* out_regions) try {
  return witness_layout_api("hm_merkle_sum_witness_layout", 2, r_f, r_p, depth, log_n, out_rows_used, out_n_advice, out_regions);
} HM_API_CATCH("hm_merkle_sum_witness_layout")

int hm_merkle_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, uint32_t* out_rows_used, uint32_t* out_n_advice,
                             uint32_t* out_regions) try {
  return witness_layout_api("hm_merkle_witness_layout", 1, r_f, r_p, depth, log_n, out_rows_used, out_n_advice, out_regions);
} HM_API_CATCH("hm_merkle_witness_layout")

int hm_poseidon_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t log_n, uint32_t* out_rows_used, uint32_t* out_n_advice,
                               uint32_t* out_regions) try {
  return witness_layout_api("hm_poseidon_witness_layout", 0, r_f, r_p, 0, log_n, out_rows_used, out_n_advice, out_regions);
} HM_API_CATCH("hm_poseidon_witness_layout")

// Everything that can be refused is refused here, before the first launch; -> the spec and n_advice.  The sum tree's forms accept
// m == 0 (nothing is written), the two others refuse it.
static int witness_args(const char* who, DeviceCtx& ctx, uint64_t handle, uint32_t E, uint32_t depth, uint32_t log_n, size_t m,
                        bool with_nodes, PoseidonSpec** s, uint32_t* n_advice) {
  if (m == 0 && E != 2) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": m must be at least 1");
  if (int rc = merkle_spec(who, ctx, handle, E == 1 ? 3 : 5, s)) return rc;
  uint32_t t[6];
  if (int rc = witness_layout(who, E, (*s)->r_f, (*s)->r_p, depth, log_n, t)) return rc;
  if (with_nodes && depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a built tree has depth <= 30");
  if ((uint64_t)m * (E ? depth : 1u) > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": more than 2^31 hashes");
  *n_advice = t[1];
  return HM_OK;
}

// the lanes move elements as 16-byte vectors; p8: the indices (or null)
static int witness_aligned(const char* who, std::initializer_list<const void*> p16, const void* p8) {
  uintptr_t bits = (uintptr_t)p8 & 7u;
  for (const void* p : p16) bits |= (uintptr_t)p & 15u;
  if (bits) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a device pointer is not 16-byte aligned (d_indices: 8)");
  return HM_OK;
}

// the device forms of the two path circuits
static int merkle_witness_dev(const char* who, uint32_t E, uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const void* d_leaves,
                              const void* d_siblings, const uint64_t* d_indices, const uint64_t* assets_sum, const void* d_nodes_or_null,
                              void* d_advice, void* d_instance, void* stream) {
  if (!d_leaves || !d_siblings || !d_indices || (E == 2 && !assets_sum) || !d_advice || !d_instance)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (int rc = witness_aligned(who, {d_leaves, d_siblings, d_nodes_or_null, d_advice, d_instance}, d_indices)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  uint32_t n_advice = 0;
  if (int rc = witness_args(who, *ctx, handle, E, depth, log_n, m, d_nodes_or_null != nullptr, &s, &n_advice)) return rc;
  return merkle_witness_run(E, *s, depth, log_n, m, (const uint32_t*)d_leaves, (const uint32_t*)d_siblings, d_indices, assets_sum,
                            (const uint32_t*)d_nodes_or_null, (uint32_t*)d_advice, (uint32_t*)d_instance, (hipStream_t)stream);
}

int hm_merkle_sum_witness_bn256_dev(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const void* d_leaves,
                                    const void* d_siblings, const uint64_t* d_indices, const uint64_t* assets_sum,
                                    const void* d_nodes_or_null, void* d_advice, void* d_instance, void* stream) try {
  return merkle_witness_dev("hm_merkle_sum_witness_bn256_dev", 2, handle, depth, log_n, m, d_leaves, d_siblings, d_indices, assets_sum,
                            d_nodes_or_null, d_advice, d_instance, stream);
} HM_API_CATCH("hm_merkle_sum_witness_bn256_dev")

int hm_merkle_witness_bn256_dev(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const void* d_leaves, const void* d_siblings,
                                const uint64_t* d_indices, const void* d_nodes_or_null, void* d_advice, void* d_instance, void* stream) try {
  return merkle_witness_dev("hm_merkle_witness_bn256_dev", 1, handle, depth, log_n, m, d_leaves, d_siblings, d_indices, nullptr,
                            d_nodes_or_null, d_advice, d_instance, stream);
} HM_API_CATCH("hm_merkle_witness_bn256_dev")

int hm_poseidon_witness_bn256_dev(uint64_t handle, uint32_t log_n, size_t m, const void* d_msgs, void* d_advice, void* d_instance,
                                  void* stream) try {
  const char* who = "hm_poseidon_witness_bn256_dev";
  if (!d_msgs || !d_advice || !d_instance) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (int rc = witness_aligned(who, {d_msgs, d_advice, d_instance}, nullptr)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  uint32_t n_advice = 0;
  if (int rc = witness_args(who, *ctx, handle, 0, 0, log_n, m, false, &s, &n_advice)) return rc;
  return poseidon_witness_run(*s, log_n, m, (const uint32_t*)d_msgs, (uint32_t*)d_advice, (uint32_t*)d_instance, (hipStream_t)stream);
} HM_API_CATCH("hm_poseidon_witness_bn256_dev")

// The host forms: the inputs (at 64-byte boundaries, `in_end` bytes in all), the columns and the instance share one staging buffer;
// `launch` gets the buffer and the device addresses of the columns and the instance.
using WitnessLaunch = std::function<int(uint8_t*, uint32_t*, uint32_t*)>;
static int witness_host(const char* who, DeviceCtx& ctx, uint32_t n_advice, uint32_t log_n, size_t m, const HostIn* in, size_t n_in,
                        size_t in_end, size_t inst_bytes, uint64_t* advice, uint64_t* instance, const WitnessLaunch& launch) {
  const size_t col_bytes = (size_t)32 << log_n;
  if (m > WITNESS_HOST_MAX_BYTES / ((size_t)n_advice * col_bytes))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the columns exceed 256 MiB; use the device form");
  const size_t adv_bytes = m * n_advice * col_bytes;
  const HostOut out[2] = {{instance, inst_bytes, in_end + adv_bytes, true}, {advice, adv_bytes, in_end, false}};
  return host_round_trip(who, ctx, "witness", in_end + adv_bytes + inst_bytes, in, n_in, out, 2,
                         [&](uint8_t* d) { return launch(d, (uint32_t*)(d + in_end), (uint32_t*)(d + in_end + adv_bytes)); });
}

// the host forms of the two path circuits (never with a built tree)
static int merkle_witness_host(const char* who, uint32_t E, uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const uint64_t* leaves,
                               const uint64_t* siblings, const uint64_t* indices, const uint64_t* assets_sum, uint64_t* advice,
                               uint64_t* instance) {
  if (!leaves || !siblings || !indices || (E == 2 && !assets_sum) || !advice || !instance)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  uint32_t n_advice = 0;
  if (int rc = witness_args(who, *ctx, handle, E, depth, log_n, m, false, &s, &n_advice)) return rc;
  if (m == 0) return HM_OK;
  const size_t leaf_bytes = m * E * 32, sib_bytes = leaf_bytes * depth, sib_at = pad64(leaf_bytes), idx_at = sib_at + pad64(sib_bytes);
  const HostIn in[3] = {{leaves, leaf_bytes, 0}, {siblings, sib_bytes, sib_at}, {indices, m * 8, idx_at}};
  return witness_host(who, *ctx, n_advice, log_n, m, in, 3, idx_at + pad64(m * 8), m * (E == 2 ? 128 : 64), advice, instance,
                      [&](uint8_t* d, uint32_t* d_adv, uint32_t* d_inst) {
                        return merkle_witness_run(E, *s, depth, log_n, m, (const uint32_t*)d, (const uint32_t*)(d + sib_at),
                                                  (const uint64_t*)(d + idx_at), assets_sum, nullptr, d_adv, d_inst, nullptr);
                      });
}

int hm_merkle_sum_witness_bn256(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const uint64_t* leaves,
                                const uint64_t* siblings, const uint64_t* indices, const uint64_t* assets_sum, uint64_t* advice,
                                uint64_t* instance) try {
  return merkle_witness_host("hm_merkle_sum_witness_bn256", 2, handle, depth, log_n, m, leaves, siblings, indices, assets_sum, advice, instance);
} HM_API_CATCH("hm_merkle_sum_witness_bn256")

int hm_merkle_witness_bn256(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const uint64_t* leaves, const uint64_t* siblings,
                            const uint64_t* indices, uint64_t* advice, uint64_t* instance) try {
  return merkle_witness_host("hm_merkle_witness_bn256", 1, handle, depth, log_n, m, leaves, siblings, indices, nullptr, advice, instance);
} HM_API_CATCH("hm_merkle_witness_bn256")

int hm_poseidon_witness_bn256(uint64_t handle, uint32_t log_n, size_t m, const uint64_t* msgs, uint64_t* advice, uint64_t* instance) try {
  if (!msgs || !advice || !instance) return hm_fail(HM_ERR_BAD_ARG, "hm_poseidon_witness_bn256: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  uint32_t n_advice = 0;
  if (int rc = witness_args("hm_poseidon_witness_bn256", *ctx, handle, 0, 0, log_n, m, false, &s, &n_advice)) return rc;
  const HostIn in{msgs, m * 128, 0};
  return witness_host("hm_poseidon_witness_bn256", *ctx, n_advice, log_n, m, &in, 1, m * 128, m * 32, advice, instance,
                      [&](uint8_t* d, uint32_t* d_adv, uint32_t* d_inst) {
                        return poseidon_witness_run(*s, log_n, m, (const uint32_t*)d, d_adv, d_inst, nullptr);
                      });
} HM_API_CATCH("hm_poseidon_witness_bn256")

// ---- a built tree updated in place, and the roots of many paths (poseidon.inc: merkle_update_*, merkle_root_lane) -----------------
static int merkle_update_dev(const char* who, uint64_t handle, uint32_t width, uint32_t depth, void* d_nodes, const uint64_t* d_indices,
                             const void* d_new_leaves, size_t m, uint32_t* d_counts_or_null, void* stream) {
  const std::string w(who);
  if (m && (!d_nodes || !d_indices || !d_new_leaves)) return hm_fail(HM_ERR_BAD_ARG, w + ": null argument");
  if (depth == 0 || depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, w + ": depth must be 1 .. 30");
  if (m > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, w + ": m > 2^31");
  if (int rc = witness_aligned(who, {d_nodes, d_new_leaves}, d_indices)) return rc;
  if ((uintptr_t)d_counts_or_null & 3u) return hm_fail(HM_ERR_BAD_ARG, w + ": d_counts is not 4-byte aligned");
  const size_t elem_bytes = width == 5 ? 64 : 32;
  if (m && ranges_overlap(d_new_leaves, m * elem_bytes, d_nodes, (((size_t)2 << depth) - 1) * elem_bytes))
    return hm_fail(HM_ERR_BAD_ARG, w + ": d_new_leaves overlaps d_nodes");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = nullptr;
  if (int rc = merkle_spec(who, *ctx, handle, width, &s)) return rc;
  return merkle_update_run(*s, (uint32_t*)d_nodes, depth, d_indices, (const uint32_t*)d_new_leaves, m, d_counts_or_null, (hipStream_t)stream);
}

int hm_merkle_sum_tree_update_dev(uint64_t handle, uint32_t depth, void* d_nodes, const uint64_t* d_indices, const void* d_new_leaves,
                                  size_t m, uint32_t* d_counts_or_null, void* stream) try {
  return merkle_update_dev("hm_merkle_sum_tree_update_dev", handle, 5, depth, d_nodes, d_indices, d_new_leaves, m, d_counts_or_null, stream);
} HM_API_CATCH("hm_merkle_sum_tree_update_dev")

int hm_merkle_tree_update_dev(uint64_t handle, uint32_t depth, void* d_nodes, const uint64_t* d_indices, const void* d_new_leaves, size_t m,
                              uint32_t* d_counts_or_null, void* stream) try {
  return merkle_update_dev("hm_merkle_tree_update_dev", handle, 3, depth, d_nodes, d_indices, d_new_leaves, m, d_counts_or_null, stream);
} HM_API_CATCH("hm_merkle_tree_update_dev")

// what both forms of the roots refuse before anything else
static int merkle_roots_args(const char* who, uint32_t depth, size_t m, const void* leaves, const void* siblings, const void* indices,
                             const void* roots) {
  if (m && (!leaves || !siblings || !indices || !roots)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (depth == 0 || depth > MERKLE_MAX_DEPTH) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": depth must be 1 .. 30");
  if (m > POSEIDON_MAX_N) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": m > 2^31");
  return HM_OK;
}

int hm_merkle_roots_bn256_dev(uint64_t handle, uint32_t depth, size_t m, const void* d_leaves, const void* d_siblings,
                              const uint64_t* d_indices, void* d_roots, void* stream) try {
  const char* who = "hm_merkle_roots_bn256_dev";
  if (int rc = merkle_roots_args(who, depth, m, d_leaves, d_siblings, d_indices, d_roots)) return rc;
  if (int rc = witness_aligned(who, {d_leaves, d_siblings, d_roots}, d_indices)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = find_poseidon(*ctx, handle);
  if (!s) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown spec handle");
  return merkle_roots_run(*s, depth, m, (const uint32_t*)d_leaves, (const uint32_t*)d_siblings, d_indices, (uint32_t*)d_roots,
                          (hipStream_t)stream);
} HM_API_CATCH("hm_merkle_roots_bn256_dev")

int hm_merkle_roots_bn256(uint64_t handle, uint32_t depth, size_t m, const uint64_t* leaves, const uint64_t* siblings,
                          const uint64_t* indices, uint64_t* roots) try {
  const char* who = "hm_merkle_roots_bn256";
  if (int rc = merkle_roots_args(who, depth, m, leaves, siblings, indices, roots)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PoseidonSpec* s = find_poseidon(*ctx, handle);
  if (!s) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown spec handle");
  if (m == 0) return HM_OK;
  const size_t elem_bytes = s->width == 5 ? 64 : 32;
  const size_t leaf_bytes = m * elem_bytes, sib_bytes = leaf_bytes * depth, idx_at = leaf_bytes + sib_bytes, roots_at = idx_at + pad64(m * 8);
  const HostIn in[3] = {{leaves, leaf_bytes, 0}, {siblings, sib_bytes, leaf_bytes}, {indices, m * 8, idx_at}};
  const HostOut out{roots, leaf_bytes, roots_at, false};
  return host_round_trip(who, *ctx, "poseidon", roots_at + leaf_bytes, in, 3, &out, 1, [&](uint8_t* d) {
    return merkle_roots_run(*s, depth, m, (const uint32_t*)d, (const uint32_t*)(d + leaf_bytes), (const uint64_t*)(d + idx_at),
                            (uint32_t*)(d + roots_at), nullptr);
  });
} HM_API_CATCH("hm_merkle_roots_bn256")

// ---- the range-check circuit's witness (range.inc: range_witness_lane) ---------------------------------------------------------------
// what the layout and both forms of the witness refuse; -> n_advice and the rows of the table
static int range_witness_layout(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* n_advice,
                                uint32_t* table_rows) {
  const std::string w(who);
  if (max_bits == 0 || max_bits > 16) return hm_fail(HM_ERR_BAD_ARG, w + ": max_bits must be 1 .. 16");
  if (acc_cols == 0 || (uint64_t)max_bits * acc_cols > 253)
    return hm_fail(HM_ERR_BAD_ARG, w + ": acc_cols must be at least 1 and max_bits * acc_cols at most 253");
  if (log_n > WITNESS_MAX_LOG_N) return hm_fail(HM_ERR_BAD_ARG, w + ": log_n > 24");
  if (rows == 0) return hm_fail(HM_ERR_BAD_ARG, w + ": rows must be at least 1");
  const uint64_t need = rows > (1u << max_bits) ? rows : (1u << max_bits);
  if (((uint64_t)1 << log_n) < need + 6)
    return hm_fail(HM_ERR_BAD_ARG, w + ": the circuit needs " + std::to_string(need) + " rows, 2^log_n - 6 is fewer");
  *n_advice = 1 + acc_cols;
  *table_rows = 1u << max_bits;
  return HM_OK;
}

int hm_range_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                            uint32_t* out_table_rows) try {
  if (!out_n_advice || !out_table_rows) return hm_fail(HM_ERR_BAD_ARG, "hm_range_witness_layout: null argument");
  uint32_t n_advice = 0, table_rows = 0;
  if (int rc = range_witness_layout("hm_range_witness_layout", max_bits, acc_cols, log_n, rows, &n_advice, &table_rows)) return rc;
  *out_n_advice = n_advice;
  *out_table_rows = table_rows;
  return HM_OK;
} HM_API_CATCH("hm_range_witness_layout")

static int range_witness_args(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows,
                              const void* values, const void* advice, uint32_t* n_advice) {
  if (!values || !advice) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (m == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": m must be at least 1");
  uint32_t table_rows = 0;
  if (int rc = range_witness_layout(who, max_bits, acc_cols, log_n, rows, n_advice, &table_rows)) return rc;
  if (m > (POSEIDON_MAX_N >> log_n)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": more than 2^31 rows");
  return HM_OK;
}

int hm_range_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                  void* d_advice, uint32_t* d_over_or_null, void* stream) try {
  const char* who = "hm_range_witness_bn256_fr_dev";
  uint32_t n_advice = 0;
  if (int rc = range_witness_args(who, max_bits, acc_cols, log_n, m, rows, d_values, d_advice, &n_advice)) return rc;
  if (int rc = witness_aligned(who, {d_values, d_advice}, nullptr)) return rc;
  if ((uintptr_t)d_over_or_null & 3u) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_over is not 4-byte aligned");
  if (ranges_overlap(d_values, m * rows * 32, d_advice, m * n_advice * ((size_t)32 << log_n)))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_values overlaps d_advice");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return range_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d_values, (uint32_t*)d_advice, d_over_or_null,
                           (hipStream_t)stream);
} HM_API_CATCH("hm_range_witness_bn256_fr_dev")

int hm_range_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* values,
                              uint64_t* advice, uint32_t* over_or_null) try {
  const char* who = "hm_range_witness_bn256_fr";
  uint32_t n_advice = 0;
  if (int rc = range_witness_args(who, max_bits, acc_cols, log_n, m, rows, values, advice, &n_advice)) return rc;
  const size_t col_bytes = (size_t)32 << log_n;
  if (m > WITNESS_HOST_MAX_BYTES / ((size_t)n_advice * col_bytes))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the columns exceed 256 MiB; use the device form");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const size_t in_bytes = pad64(m * rows * 32), adv_bytes = m * n_advice * col_bytes, over_bytes = m * sizeof(uint32_t);
  const HostIn in{values, m * rows * 32, 0};
  const HostOut out[2] = {{over_or_null, over_or_null ? over_bytes : 0, in_bytes + adv_bytes, true}, {advice, adv_bytes, in_bytes, false}};
  return host_round_trip(who, *ctx, "witness", in_bytes + adv_bytes + over_bytes, &in, 1, out, 2, [&](uint8_t* d) {
    return range_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d, (uint32_t*)(d + in_bytes),
                             (uint32_t*)(d + in_bytes + adv_bytes), nullptr);
  });
} HM_API_CATCH("hm_range_witness_bn256_fr")

// ---- the sorted-column circuit's witness (sorted.inc: sorted_witness_lane) and the argsort of an id column -----------------------------
// what the layout and both forms of the witness refuse: the range check's limits, and max_bits * acc_cols + log_n <= 253, without
// which two ids of one column could agree mod r although every gap is in range
static int sorted_witness_layout(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* n_advice,
                                 uint32_t* table_rows) {
  if (int rc = range_witness_layout(who, max_bits, acc_cols, log_n, rows, n_advice, table_rows)) return rc;
  if ((uint64_t)max_bits * acc_cols + log_n > 253)
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": max_bits * acc_cols + log_n must be at most 253 (the gaps' sum must not wrap mod r)");
  return HM_OK;
}

int hm_sorted_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                             uint32_t* out_table_rows) try {
  if (!out_n_advice || !out_table_rows) return hm_fail(HM_ERR_BAD_ARG, "hm_sorted_witness_layout: null argument");
  uint32_t n_advice = 0, table_rows = 0;
  if (int rc = sorted_witness_layout("hm_sorted_witness_layout", max_bits, acc_cols, log_n, rows, &n_advice, &table_rows)) return rc;
  *out_n_advice = n_advice;
  *out_table_rows = table_rows;
  return HM_OK;
} HM_API_CATCH("hm_sorted_witness_layout")

static int sorted_witness_args(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows,
                               const void* ids, const void* advice, uint32_t* n_advice) {
  if (!ids || !advice) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (m == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": m must be at least 1");
  uint32_t table_rows = 0;
  if (int rc = sorted_witness_layout(who, max_bits, acc_cols, log_n, rows, n_advice, &table_rows)) return rc;
  if (m > (POSEIDON_MAX_N >> log_n)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": more than 2^31 rows");
  return HM_OK;
}

int hm_sorted_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_ids,
                                   void* d_advice, uint32_t* d_over_or_null, void* stream) try {
  const char* who = "hm_sorted_witness_bn256_fr_dev";
  uint32_t n_advice = 0;
  if (int rc = sorted_witness_args(who, max_bits, acc_cols, log_n, m, rows, d_ids, d_advice, &n_advice)) return rc;
  if (int rc = witness_aligned(who, {d_ids, d_advice}, nullptr)) return rc;
  if ((uintptr_t)d_over_or_null & 3u) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_over is not 4-byte aligned");
  if (ranges_overlap(d_ids, m * rows * 32, d_advice, m * n_advice * ((size_t)32 << log_n)))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_ids overlaps d_advice");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return sorted_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d_ids, (uint32_t*)d_advice, d_over_or_null,
                            (hipStream_t)stream);
} HM_API_CATCH("hm_sorted_witness_bn256_fr_dev")

int hm_sorted_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* ids,
                               uint64_t* advice, uint32_t* over_or_null) try {
  const char* who = "hm_sorted_witness_bn256_fr";
  uint32_t n_advice = 0;
  if (int rc = sorted_witness_args(who, max_bits, acc_cols, log_n, m, rows, ids, advice, &n_advice)) return rc;
  const size_t col_bytes = (size_t)32 << log_n;
  if (m > WITNESS_HOST_MAX_BYTES / ((size_t)n_advice * col_bytes))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the columns exceed 256 MiB; use the device form");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const size_t in_bytes = pad64(m * rows * 32), adv_bytes = m * n_advice * col_bytes, over_bytes = m * sizeof(uint32_t);
  const HostIn in{ids, m * rows * 32, 0};
  const HostOut out[2] = {{over_or_null, over_or_null ? over_bytes : 0, in_bytes + adv_bytes, true}, {advice, adv_bytes, in_bytes, false}};
  return host_round_trip(who, *ctx, "witness", in_bytes + adv_bytes + over_bytes, &in, 1, out, 2, [&](uint8_t* d) {
    return sorted_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d, (uint32_t*)(d + in_bytes),
                              (uint32_t*)(d + in_bytes + adv_bytes), nullptr);
  });
} HM_API_CATCH("hm_sorted_witness_bn256_fr")

int hm_fr_argsort_bn256_dev(const void* d_values, size_t n, uint64_t* d_perm, void* stream) try {
  const char* who = "hm_fr_argsort_bn256_dev";
  if (!d_values || !d_perm) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (n == 0 || n > ((size_t)1 << 26)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": n must be 1 .. 2^26");
  if (((uintptr_t)d_values & 15u) || ((uintptr_t)d_perm & 7u))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a device pointer is not aligned (d_values: 16, d_perm: 8)");
  if (ranges_overlap(d_values, n * 32, d_perm, n * 8)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_values overlaps d_perm");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_argsort_run((const uint32_t*)d_values, n, d_perm, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_argsort_bn256_dev")

// ---- the SafeAccumulator circuit's witness (accumulator.inc: accumulator_row) -----------------------------------------------------
// what the layout and both forms of the witness refuse; -> n_advice
static int accumulator_witness_layout(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* n_advice) {
  const std::string w(who);
  if (max_bits == 0 || max_bits > 4) return hm_fail(HM_ERR_BAD_ARG, w + ": max_bits must be 1 .. 4");
  if (acc_cols < 2 || (uint64_t)max_bits * acc_cols > 64)
    return hm_fail(HM_ERR_BAD_ARG, w + ": acc_cols must be at least 2 and max_bits * acc_cols at most 64");
  if (log_n > WITNESS_MAX_LOG_N) return hm_fail(HM_ERR_BAD_ARG, w + ": log_n > 24");
  if (rows == 0) return hm_fail(HM_ERR_BAD_ARG, w + ": rows must be at least 1");
  if (((uint64_t)1 << log_n) < (uint64_t)rows + 1 + 6)
    return hm_fail(HM_ERR_BAD_ARG, w + ": the circuit needs " + std::to_string((uint64_t)rows + 1) + " rows, 2^log_n - 6 is fewer");
  *n_advice = 2 + 2 * acc_cols;
  return HM_OK;
}

int hm_accumulator_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                                  uint32_t* out_used_rows) try {
  if (!out_n_advice || !out_used_rows) return hm_fail(HM_ERR_BAD_ARG, "hm_accumulator_witness_layout: null argument");
  uint32_t n_advice = 0;
  if (int rc = accumulator_witness_layout("hm_accumulator_witness_layout", max_bits, acc_cols, log_n, rows, &n_advice)) return rc;
  *out_n_advice = n_advice;
  *out_used_rows = rows + 1;
  return HM_OK;
} HM_API_CATCH("hm_accumulator_witness_layout")

static int accumulator_witness_args(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows,
                                    std::initializer_list<const void*> needed, uint32_t* n_advice) {
  for (const void* p : needed)
    if (!p) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (m == 0 || m > 65535) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": m must be 1 .. 65535");
  if (int rc = accumulator_witness_layout(who, max_bits, acc_cols, log_n, rows, n_advice)) return rc;
  if (m > (POSEIDON_MAX_N >> log_n)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": more than 2^31 rows");
  return HM_OK;
}

static int accumulator_witness_dev(const char* who, uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows,
                                   const void* d_values, const uint64_t* d_initial, void* d_advice, uint64_t* d_finals, uint32_t* d_over_or_null,
                                   void* stream, double* part_ms) {
  uint32_t n_advice = 0;
  if (int rc = accumulator_witness_args(who, max_bits, acc_cols, log_n, m, rows, {d_values, d_initial, d_advice, d_finals}, &n_advice)) return rc;
  if (int rc = witness_aligned(who, {d_values, d_advice}, nullptr)) return rc;
  if (((uintptr_t)d_initial | (uintptr_t)d_finals) & 7u) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_initial or d_finals is not 8-byte aligned");
  if ((uintptr_t)d_over_or_null & 3u) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_over is not 4-byte aligned");
  const size_t adv_bytes = m * n_advice * ((size_t)32 << log_n), limb_bytes = m * acc_cols * sizeof(uint64_t);
  if (ranges_overlap(d_values, m * rows * 32, d_advice, adv_bytes) || ranges_overlap(d_initial, limb_bytes, d_advice, adv_bytes) ||
      ranges_overlap(d_finals, limb_bytes, d_advice, adv_bytes) || ranges_overlap(d_finals, limb_bytes, d_values, m * rows * 32) ||
      ranges_overlap(d_finals, limb_bytes, d_initial, limb_bytes))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": an output overlaps an input or the other output");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  uint64_t inverses[15 * 4];
  host::fr_small_inverses((1u << max_bits) - 1, inverses);
  return accumulator_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d_values, d_initial, inverses, (uint32_t*)d_advice, d_finals,
                                 d_over_or_null, (hipStream_t)stream, part_ms);
}

int hm_accumulator_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                        const uint64_t* d_initial, void* d_advice, uint64_t* d_finals, uint32_t* d_over_or_null,
                                        void* stream) try {
  return accumulator_witness_dev("hm_accumulator_witness_bn256_fr_dev", max_bits, acc_cols, log_n, m, rows, d_values, d_initial, d_advice, d_finals,
                                 d_over_or_null, stream, nullptr);
} HM_API_CATCH("hm_accumulator_witness_bn256_fr_dev")

int hm_accumulator_witness_timed_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                              const uint64_t* d_initial, void* d_advice, uint64_t* d_finals, uint32_t* d_over_or_null,
                                              void* stream, double out_part_ms[4]) try {
  if (!out_part_ms) return hm_fail(HM_ERR_BAD_ARG, "hm_accumulator_witness_timed_bn256_fr_dev: null argument");
  return accumulator_witness_dev("hm_accumulator_witness_timed_bn256_fr_dev", max_bits, acc_cols, log_n, m, rows, d_values, d_initial, d_advice,
                                 d_finals, d_over_or_null, stream, out_part_ms);
} HM_API_CATCH("hm_accumulator_witness_timed_bn256_fr_dev")

int hm_accumulator_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* values,
                                    const uint64_t* initial, uint64_t* advice, uint64_t* finals, uint32_t* over_or_null) try {
  const char* who = "hm_accumulator_witness_bn256_fr";
  uint32_t n_advice = 0;
  if (int rc = accumulator_witness_args(who, max_bits, acc_cols, log_n, m, rows, {values, initial, advice, finals}, &n_advice)) return rc;
  const size_t col_bytes = (size_t)32 << log_n;
  if (m > WITNESS_HOST_MAX_BYTES / ((size_t)n_advice * col_bytes))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the columns exceed 256 MiB; use the device form");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  uint64_t inverses[15 * 4];
  host::fr_small_inverses((1u << max_bits) - 1, inverses);
  const size_t val_bytes = pad64(m * rows * 32), limb_bytes = pad64(m * acc_cols * sizeof(uint64_t)), adv_bytes = m * n_advice * col_bytes;
  const size_t adv_at = val_bytes + limb_bytes, fin_at = adv_at + adv_bytes, over_at = fin_at + limb_bytes;
  const HostIn in[2] = {{values, m * rows * 32, 0}, {initial, m * acc_cols * sizeof(uint64_t), val_bytes}};
  const HostOut out[3] = {{over_or_null, over_or_null ? m * sizeof(uint32_t) : 0, over_at, true},
                          {finals, m * acc_cols * sizeof(uint64_t), fin_at, true},
                          {advice, adv_bytes, adv_at, false}};
  return host_round_trip(who, *ctx, "witness", over_at + m * sizeof(uint32_t), in, 2, out, 3, [&](uint8_t* d) {
    return accumulator_witness_run(max_bits, acc_cols, log_n, m, rows, (const uint32_t*)d, (const uint64_t*)(d + val_bytes), inverses,
                                   (uint32_t*)(d + adv_at), (uint64_t*)(d + fin_at), (uint32_t*)(d + over_at), nullptr);
  });
} HM_API_CATCH("hm_accumulator_witness_bn256_fr")

}  // extern "C"
