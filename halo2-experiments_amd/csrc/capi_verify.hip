// capi_verify.hip -- the batch verifier's entry points of the C ABI: the proofs of a batch read slot by slot on the device and the
// column sums of their shared scalars (verify_read.inc), and the per-proof terms of the opening checks (verify_terms.inc).
#include <hip/hip_runtime.h>

#include <string>

#include "g1.h"
#include "graph_lower.h"
#include "hm_internal.h"

namespace hm {
#include "verify_terms.inc"   // the plan's layout and its check (the kernels are in lookup.hip)
}
using namespace hm;

extern "C" {

static constexpr size_t VERIFY_MAX_PROOFS = (size_t)1 << 24;
static constexpr uint32_t VERIFY_MAX_SLOTS = 1u << 16;

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

int hm_verify_terms_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                        const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared,
                        void* d_h2_r, void* d_h2_l, void* stream) try {
  const std::string who = "hm_verify_terms_dev";
  if (!plan || !d_records || !d_scalars || !d_instance || !d_bad || !d_own || !d_shared || !d_h2_r || !d_h2_l)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_proofs == 0 || n_proofs > ((size_t)1 << 20)) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_proofs <= 2^20");
  if (n_plan_words > ((size_t)1 << 24)) return hm_fail(HM_ERR_BAD_ARG, who + ": the plan is longer than 2^24 words");
  if (n_columns == 0 || n_columns > GE_MAX_COLUMNS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 .. 256 columns");
  if (((uintptr_t)d_records | (uintptr_t)d_scalars | (uintptr_t)d_instance | (uintptr_t)d_own | (uintptr_t)d_shared | (uintptr_t)d_h2_r |
       (uintptr_t)d_h2_l | (uintptr_t)d_bad) & 3u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 4-byte aligned");
  if (const char* why = vt_plan_problem(plan, n_plan_words, n_columns)) return hm_fail(HM_ERR_BAD_ARG, why);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  GraphProgram* g = nullptr;
  for (auto& have : ctx->graphs)
    if (have->handle == graph) g = have.get();
  if (!g) return hm_fail(HM_ERR_BAD_ARG, who + ": unknown program handle");
  return verify_terms_run(*ctx, *g, plan, n_plan_words, n_columns, n_dynamic, n_proofs, (const uint32_t*)d_records, (const uint32_t*)d_scalars,
                          (const uint32_t*)d_instance, d_bad, (uint32_t*)d_own, (uint32_t*)d_shared, (uint32_t*)d_h2_r, (uint32_t*)d_h2_l,
                          (hipStream_t)stream);
} HM_API_CATCH("hm_verify_terms_dev")

}  // extern "C"
