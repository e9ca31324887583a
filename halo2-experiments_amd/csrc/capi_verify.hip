// capi_verify.hip -- the batch verifier's entry points of the C ABI: the proofs of a batch read slot by slot on the device and the
// column sums of their shared scalars (verify_read.inc), the per-proof terms of the opening checks (verify_terms.inc; the single- and
// the multi-circuit entry are one function, verify_terms_entry), the per-proof sums (verify_sums.inc), and the pairing
// product checks that end every verifier (pairing.inc), and Blake2b-512 with the proofs' transcripts on it (transcript.inc).
#include <hip/hip_runtime.h>

#include <string>

#include "g1.h"
#include "graph_lower.h"
#include "hm_internal.h"

namespace hm {
#include "verify_terms.inc"   // the plan's layout and its check (the kernels are in verify.hip)
#include "transcript.inc"     // the schedule's check (likewise)
}
using namespace hm;

extern "C" {

static constexpr size_t VERIFY_MAX_PROOFS = (size_t)1 << 24;
static constexpr uint32_t VERIFY_MAX_SLOTS = 1u << 16;
static constexpr size_t PAIRING_MAX_CHECKS = (size_t)1 << 20, PAIRING_MAX_PAIRS = (size_t)1 << 24;

int hm_verify_read_proofs_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                              uint32_t points, uint32_t scalars, void* d_points_xy, void* d_tail_xy, void* d_y_bytes, void* d_scalars,
                              uint32_t* d_bad, void* stream) try {
  const std::string who = "hm_verify_read_proofs_dev";
  if (!d_proofs || !d_slot_table || !d_points_xy || !d_tail_xy || !d_y_bytes || !d_scalars || !d_bad)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^24");
  if (slots == 0 || slots > VERIFY_MAX_SLOTS || (uint64_t)points + scalars != slots || own_points > points)
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= slots <= 2^16, points + scalars == slots and own_points <= points");
  if (((uintptr_t)d_proofs | (uintptr_t)d_points_xy | (uintptr_t)d_tail_xy | (uintptr_t)d_y_bytes | (uintptr_t)d_scalars) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_slot_table | (uintptr_t)d_bad) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_slot_table / d_bad is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return verify_read_run((const uint32_t*)d_proofs, n_proofs, d_slot_table, slots, own_points, points, scalars, (uint32_t*)d_points_xy,
                         (uint32_t*)d_tail_xy, (uint32_t*)d_y_bytes, (uint32_t*)d_scalars, d_bad, (hipStream_t)stream);
} HM_API_CATCH("hm_verify_read_proofs_dev")

int hm_verify_column_sum_dev(const void* d_rows, size_t n_rows, uint32_t columns, size_t lo, size_t hi, void* d_out, void* stream) try {
  const std::string who = "hm_verify_column_sum_dev";
  if (!d_rows || !d_out) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (columns == 0 || columns > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= columns <= 2^16");
  if (n_rows > VERIFY_MAX_PROOFS || lo > hi || hi > n_rows) return hm_fail(HM_ERR_BAD_ARG, who + ": need lo <= hi <= n_rows <= 2^24");
  if (((uintptr_t)d_rows | (uintptr_t)d_out) & 15u) return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return verify_colsum_run((const uint32_t*)d_rows, columns, lo, hi, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_verify_column_sum_dev")

// ---- the per-proof terms (verify_terms.inc, verify.hip): ONE entry behind the three of the ABI ----------------------------------------
// road: VT_MULTI, proofs of `circuits` circuits each (a circuits of 0 is the caller's mistake there, so it cannot stand for "single");
// VT_SINGLE, single-circuit SHPLONK proofs, and VT_GWC, single-circuit GWC proofs (d_h2_r is then d_w_left and d_h2_l is given the
// same pointer, which nothing reads): `circuits` is not looked at.  proof_bits: log2 of the most proofs a call takes.  The checks keep
// their order.
enum VtRoad { VT_SINGLE, VT_MULTI, VT_GWC };
static int verify_terms_entry(const std::string& who, uint32_t circuits, VtRoad road, unsigned proof_bits, uint64_t graph, const uint32_t* plan,
                              size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs, const void* d_records,
                              const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared, void* d_h2_r,
                              void* d_h2_l, void* stream) {
  if (!plan || !d_records || !d_scalars || !d_instance || !d_bad || !d_own || !d_shared || !d_h2_r || !d_h2_l)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  const bool multi = road == VT_MULTI;
  if (multi && (circuits == 0 || circuits > VM_MAX_CIRCUITS)) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= circuits <= 64");
  if (n_proofs == 0 || n_proofs > ((size_t)1 << proof_bits))
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^" + std::to_string(proof_bits));
  if (n_plan_words > ((size_t)1 << 24)) return hm_fail(HM_ERR_BAD_ARG, who + ": the plan is longer than 2^24 words");
  if (n_columns == 0 || n_columns > GE_MAX_COLUMNS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 .. 256 columns");
  if (((uintptr_t)d_records | (uintptr_t)d_scalars | (uintptr_t)d_instance | (uintptr_t)d_own | (uintptr_t)d_shared | (uintptr_t)d_h2_r |
       (uintptr_t)d_h2_l | (uintptr_t)d_bad) & 3u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 4-byte aligned");
  if (const char* why = multi            ? vtm_plan_problem(plan, n_plan_words, n_columns, circuits)
                        : road == VT_GWC ? vg_plan_problem(plan, n_plan_words, n_columns)
                                         : vt_plan_problem(plan, n_plan_words, n_columns))
    return hm_fail(HM_ERR_BAD_ARG, why);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  GraphProgram* g = nullptr;
  for (auto& have : ctx->graphs)
    if (have->handle == graph) g = have.get();
  if (!g) return hm_fail(HM_ERR_BAD_ARG, who + ": unknown program handle");
  const uint32_t *records = (const uint32_t*)d_records, *evals = (const uint32_t*)d_scalars, *inst = (const uint32_t*)d_instance;
  uint32_t *own = (uint32_t*)d_own, *shared = (uint32_t*)d_shared, *h2r = (uint32_t*)d_h2_r, *h2l = (uint32_t*)d_h2_l;
  if (multi)
    return verify_terms_multi_run(*ctx, *g, plan, n_plan_words, n_columns, n_dynamic, n_proofs, circuits, records, evals, inst, d_bad, own, shared,
                                  h2r, h2l, (hipStream_t)stream);
  if (road == VT_GWC)
    return verify_terms_gwc_run(*ctx, *g, plan, n_plan_words, n_columns, n_dynamic, n_proofs, records, evals, inst, d_bad, own, shared, h2r,
                                (hipStream_t)stream);
  return verify_terms_run(*ctx, *g, plan, n_plan_words, n_columns, n_dynamic, n_proofs, records, evals, inst, d_bad, own, shared, h2r, h2l,
                          (hipStream_t)stream);
}

int hm_verify_terms_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                        const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared,
                        void* d_h2_r, void* d_h2_l, void* stream) try {
  return verify_terms_entry("hm_verify_terms_dev", 0, VT_SINGLE, 20, graph, plan, n_plan_words, n_columns, n_dynamic, n_proofs, d_records, d_scalars,
                            d_instance, d_bad, d_own, d_shared, d_h2_r, d_h2_l, stream);
} HM_API_CATCH("hm_verify_terms_dev")

int hm_verify_terms_multi_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                              uint32_t circuits, const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad,
                              void* d_own, void* d_shared, void* d_h2_r, void* d_h2_l, void* stream) try {
  return verify_terms_entry("hm_verify_terms_multi_dev", circuits, VT_MULTI, 16, graph, plan, n_plan_words, n_columns, n_dynamic, n_proofs, d_records,
                            d_scalars, d_instance, d_bad, d_own, d_shared, d_h2_r, d_h2_l, stream);
} HM_API_CATCH("hm_verify_terms_multi_dev")

int hm_verify_terms_gwc_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                            const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared,
                            void* d_w_left, void* stream) try {
  return verify_terms_entry("hm_verify_terms_gwc_dev", 0, VT_GWC, 20, graph, plan, n_plan_words, n_columns, n_dynamic, n_proofs, d_records,
                            d_scalars, d_instance, d_bad, d_own, d_shared, d_w_left, d_w_left, stream);
} HM_API_CATCH("hm_verify_terms_gwc_dev")

// ---- the per-proof sums (verify_sums.inc, verify.hip) -------------------------------------------------------------------------------
int hm_verify_proof_sums_dev(const void* d_bases_xy, size_t n_proofs, uint32_t own_points, uint32_t shared_points, const void* d_own,
                             const void* d_shared, const void* d_h2_r, const void* d_h2_l, const uint32_t* d_bad, void* d_pairs_xy,
                             void* stream) try {
  const std::string who = "hm_verify_proof_sums_dev";
  if (!d_bases_xy || !d_own || !d_shared || !d_h2_r || !d_h2_l || !d_bad || !d_pairs_xy) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > PAIRING_MAX_CHECKS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^20");
  if ((uint64_t)own_points + shared_points == 0 || (uint64_t)own_points + shared_points > VERIFY_MAX_SLOTS)
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= own_points + shared_points <= 2^16");
  if (((uintptr_t)d_bases_xy | (uintptr_t)d_own | (uintptr_t)d_shared | (uintptr_t)d_h2_r | (uintptr_t)d_h2_l | (uintptr_t)d_pairs_xy) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if ((uintptr_t)d_bad & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_bad is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return verify_sums_run((const uint32_t*)d_bases_xy, n_proofs, own_points, shared_points, (const uint32_t*)d_own, (const uint32_t*)d_shared,
                         (const uint32_t*)d_h2_r, (const uint32_t*)d_h2_l, d_bad, (uint32_t*)d_pairs_xy, (hipStream_t)stream);
} HM_API_CATCH("hm_verify_proof_sums_dev")

// ---- Blake2b-512 and the transcripts of a batch (transcript.inc, lookup.hip) ----------------------------------------------------------
int hm_blake2b512_dev(const void* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, const uint8_t* personal16, void* d_out,
                      void* stream) try {
  const std::string who = "hm_blake2b512_dev";
  if (!d_msgs || !d_lens || !d_out) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n == 0 || n > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n <= 2^24");
  if (stride == 0 || stride > 0xffffffffull) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= stride < 2^32");
  if (((uintptr_t)d_lens | (uintptr_t)d_out) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_lens / d_out is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return blake2b_run((const uint8_t*)d_msgs, stride, d_lens, n, personal16, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_blake2b512_dev")

int hm_verify_transcript_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t points,
                             const void* d_y_bytes, const void* d_preamble, const uint32_t* d_preamble_counts, uint32_t preamble_stride,
                             const uint32_t* schedule, size_t n_schedule_pairs, uint32_t* d_bad_in_out, void* d_records,
                             uint32_t record_elems, void* stream) try {
  const std::string who = "hm_verify_transcript_dev";
  if (!d_proofs || !d_slot_table || !d_y_bytes || !d_preamble || !d_preamble_counts || !schedule || !d_bad_in_out || !d_records)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^24");
  if (slots == 0 || slots > VERIFY_MAX_SLOTS || points > slots) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= slots <= 2^16 and points <= slots");
  if (preamble_stride == 0 || preamble_stride > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= preamble_stride <= 2^16");
  if (record_elems == 0 || record_elems > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= record_elems <= 2^16");
  if (n_schedule_pairs == 0 || n_schedule_pairs > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_schedule_pairs <= 2^16");
  if (((uintptr_t)d_proofs | (uintptr_t)d_y_bytes | (uintptr_t)d_preamble | (uintptr_t)d_records) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_slot_table | (uintptr_t)d_preamble_counts | (uintptr_t)d_bad_in_out) & 3u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": d_slot_table / d_preamble_counts / d_bad_in_out is not 4-byte aligned");
  if (const char* why = tr_schedule_problem(schedule, n_schedule_pairs, slots, record_elems)) return hm_fail(HM_ERR_BAD_ARG, why);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_transcript_run(*ctx, (const uint32_t*)d_proofs, n_proofs, d_slot_table, slots, points, (const uint32_t*)d_y_bytes,
                               (const uint32_t*)d_preamble, d_preamble_counts, preamble_stride, schedule, n_schedule_pairs, d_bad_in_out,
                               (uint32_t*)d_records, record_elems, (hipStream_t)stream);
} HM_API_CATCH("hm_verify_transcript_dev")

// ---- the EVM encoding: Keccak-256, the uncompressed read and the transcripts of a batch (keccak.inc) ---------------------------------
int hm_keccak256_dev(const void* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, void* d_out, void* stream) try {
  const std::string who = "hm_keccak256_dev";
  if (!d_msgs || !d_lens || !d_out) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n == 0 || n > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n <= 2^24");
  if (stride == 0 || stride > 0xffffffffull) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= stride < 2^32");
  if (((uintptr_t)d_lens | (uintptr_t)d_out) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_lens / d_out is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return keccak256_run((const uint8_t*)d_msgs, stride, d_lens, n, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_keccak256_dev")

int hm_verify_read_proofs_evm_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                                  uint32_t scalars, void* d_points_xy, void* d_tail_xy, void* d_scalars, uint32_t* d_bad, void* stream) try {
  const std::string who = "hm_verify_read_proofs_evm_dev";
  if (!d_proofs || !d_slot_table || !d_points_xy || !d_tail_xy || !d_scalars || !d_bad) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^24");
  if (slots == 0 || slots > VERIFY_MAX_SLOTS || 2 * (uint64_t)own_points + scalars > slots)
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= slots <= 2^16 and 2 own_points + scalars <= slots");
  if (((uintptr_t)d_proofs | (uintptr_t)d_points_xy | (uintptr_t)d_tail_xy | (uintptr_t)d_scalars) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_slot_table | (uintptr_t)d_bad) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_slot_table / d_bad is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return verify_read_evm_run((const uint32_t*)d_proofs, n_proofs, d_slot_table, slots, own_points, scalars, (uint32_t*)d_points_xy,
                             (uint32_t*)d_tail_xy, (uint32_t*)d_scalars, d_bad, (hipStream_t)stream);
} HM_API_CATCH("hm_verify_read_proofs_evm_dev")

int hm_verify_transcript_evm_dev(const void* d_proofs, size_t n_proofs, uint32_t slots, const void* d_preamble,
                                 const uint32_t* d_preamble_counts, uint32_t preamble_stride, const uint32_t* schedule,
                                 size_t n_schedule_pairs, uint32_t* d_bad_in_out, void* d_records, uint32_t record_elems, void* stream) try {
  const std::string who = "hm_verify_transcript_evm_dev";
  if (!d_proofs || !d_preamble || !d_preamble_counts || !schedule || !d_bad_in_out || !d_records)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > VERIFY_MAX_PROOFS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^24");
  if (slots == 0 || slots > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= slots <= 2^16");
  if (preamble_stride == 0 || preamble_stride > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= preamble_stride <= 2^16");
  if (record_elems == 0 || record_elems > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= record_elems <= 2^16");
  if (n_schedule_pairs == 0 || n_schedule_pairs > VERIFY_MAX_SLOTS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_schedule_pairs <= 2^16");
  if (((uintptr_t)d_proofs | (uintptr_t)d_preamble | (uintptr_t)d_records) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_preamble_counts | (uintptr_t)d_bad_in_out) & 3u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": d_preamble_counts / d_bad_in_out is not 4-byte aligned");
  if (const char* why = tr_schedule_problem(schedule, n_schedule_pairs, slots, record_elems)) return hm_fail(HM_ERR_BAD_ARG, why);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return verify_transcript_evm_run(*ctx, (const uint32_t*)d_proofs, n_proofs, slots, (const uint32_t*)d_preamble, d_preamble_counts,
                                   preamble_stride, schedule, n_schedule_pairs, d_bad_in_out, (uint32_t*)d_records, record_elems,
                                   (hipStream_t)stream);
} HM_API_CATCH("hm_verify_transcript_evm_dev")

// ---- pairing product checks (pairing.inc, lookup.hip) ------------------------------------------------------------------------------
size_t hm_pairing_work_bytes(size_t n_pairs, size_t n_checks) {
  if (n_checks == 0 || n_checks > PAIRING_MAX_CHECKS || n_pairs > PAIRING_MAX_PAIRS) return 0;
  return pairing_work_words(n_pairs, n_checks) * sizeof(uint32_t);
}

int hm_pairing_check_bn256_dev(const void* d_g1_xy, const void* d_g2_xy, size_t n_pairs, const uint32_t* d_offsets, size_t n_checks,
                               void* d_gt, uint32_t* d_status, void* d_work, size_t work_bytes, void* stream) try {
  const std::string who = "hm_pairing_check_bn256_dev";
  if (!d_g1_xy || !d_g2_xy || !d_offsets || !d_status || !d_work) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_checks == 0 || n_checks > PAIRING_MAX_CHECKS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_checks <= 2^20");
  if (n_pairs > PAIRING_MAX_PAIRS) return hm_fail(HM_ERR_BAD_ARG, who + ": need n_pairs <= 2^24");
  if (work_bytes < hm_pairing_work_bytes(n_pairs, n_checks)) return hm_fail(HM_ERR_BAD_ARG, who + ": the workspace is shorter than hm_pairing_work_bytes");
  if (((uintptr_t)d_g1_xy | (uintptr_t)d_g2_xy | (uintptr_t)d_gt | (uintptr_t)d_work) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_offsets | (uintptr_t)d_status) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_offsets / d_status is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return pairing_check_run((const uint32_t*)d_g1_xy, (const uint32_t*)d_g2_xy, n_pairs, d_offsets, n_checks, (uint32_t*)d_gt, d_status,
                           (uint32_t*)d_work, (hipStream_t)stream);
} HM_API_CATCH("hm_pairing_check_bn256_dev")

}  // extern "C"
