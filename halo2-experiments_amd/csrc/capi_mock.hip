// capi_mock.hip -- the witness checker's entry points of the C ABI: the gates, the copy constraints and the lookups of a batch of
// witnesses checked on the device (mock.hip), failures appended to the caller's record buffer.
#include <hip/hip_runtime.h>

#include <string>

#include "graph_lower.h"
#include "hm_internal.h"

using namespace hm;

extern "C" {

// what the three entries refuse before anything else
static int mock_args(const std::string& who, const void* const* bases, const uint64_t* strides, const uint32_t* rows, size_t n_columns,
                     uint32_t k, size_t m, uint32_t user_base, const void* d_records, size_t cap, const void* d_counter,
                     const void* d_user_flags, const uint64_t* out_total) {
  if (!bases || !strides || !rows || !d_records || !d_counter || !d_user_flags || !out_total)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_columns == 0 || n_columns > GE_MAX_COLUMNS) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 .. 256 columns");
  if (k > 30) return hm_fail(HM_ERR_BAD_ARG, who + ": k > 30");
  if (m == 0 || m > ((size_t)1 << 31) || (uint64_t)m + user_base > ((uint64_t)1 << 32))
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= m <= 2^31 users");
  if (cap == 0) return hm_fail(HM_ERR_BAD_ARG, who + ": a record buffer of capacity 0");
  if (((uintptr_t)d_records & 7u) || ((uintptr_t)d_counter & 7u))
    return hm_fail(HM_ERR_BAD_ARG, who + ": d_records / d_counter is not 8-byte aligned");
  for (size_t i = 0; i < n_columns; ++i) {
    if (!bases[i]) return hm_fail(HM_ERR_BAD_ARG, who + ": null column pointer");
    if (((uintptr_t)bases[i] & 15u) || (strides[i] & 3u)) return hm_fail(HM_ERR_BAD_ARG, who + ": a column is not 16-byte aligned");
    if (rows[i] > ((uint64_t)1 << k)) return hm_fail(HM_ERR_BAD_ARG, who + ": a column holds more than 2^k rows");
  }
  return HM_OK;
}

// the small read-back that ends every call: the counter as it stands behind this call's launches
static int mock_total(uint64_t* d_counter, uint64_t* out_total, hipStream_t stream) {
  uint64_t total = 0;
  HM_HIP_CHECK(hipMemcpyAsync(&total, d_counter, sizeof total, hipMemcpyDeviceToHost, stream));
  HM_HIP_CHECK(hipStreamSynchronize(stream));
  *out_total = total;
  return HM_OK;
}

static GraphProgram* mock_program(DeviceCtx& ctx, uint64_t handle) {
  for (auto& g : ctx.graphs)
    if (g->handle == handle) return g.get();
  return nullptr;
}

int hm_mock_gates_dev(uint64_t graph, const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows,
                      size_t n_columns, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t k, uint32_t usable_rows, size_t m,
                      const uint64_t* d_lanes_or_null, size_t n_lanes, uint64_t* d_records, size_t cap, uint64_t* d_counter,
                      uint8_t* d_user_flags, uint64_t* out_total, void* stream) try {
  const std::string who = "hm_mock_gates_dev";
  if (int rc = mock_args(who, column_bases, column_strides, column_rows, n_columns, k, m, 0, d_records, cap, d_counter, d_user_flags, out_total))
    return rc;
  if (n_dynamic && !dynamic_constants) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (usable_rows == 0 || usable_rows > ((uint64_t)1 << k)) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= usable_rows <= 2^k");
  if ((uint64_t)m * usable_rows > ((uint64_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, who + ": m * usable_rows > 2^32");
  if (d_lanes_or_null && (((uintptr_t)d_lanes_or_null & 7u) || n_lanes == 0 || n_lanes > ((uint64_t)1 << 32)))
    return hm_fail(HM_ERR_BAD_ARG, who + ": the lane list is empty, longer than 2^32 or not 8-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  GraphProgram* g = mock_program(*ctx, graph);
  if (!g) return hm_fail(HM_ERR_NOT_FOUND, who + ": unknown program handle");
  const MockTable table{column_bases, column_strides, column_rows, n_columns};
  const MockSink sink{d_records, cap, d_counter, d_user_flags};
  if (int rc = mock_program_run(*ctx, *g, table, dynamic_constants, n_dynamic, k, usable_rows, m, 0, d_lanes_or_null, n_lanes, nullptr, sink,
                                (hipStream_t)stream))
    return rc;
  return mock_total(d_counter, out_total, (hipStream_t)stream);
} HM_API_CATCH("hm_mock_gates_dev")

int hm_mock_copies_dev(const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows, size_t n_columns,
                       const uint32_t* permutation_columns, size_t n_permutation, const uint32_t* d_copies, size_t n_copies, uint32_t k,
                       size_t m, uint64_t* d_records, size_t cap, uint64_t* d_counter, uint8_t* d_user_flags, uint64_t* out_total,
                       void* stream) try {
  const std::string who = "hm_mock_copies_dev";
  if (int rc = mock_args(who, column_bases, column_strides, column_rows, n_columns, k, m, 0, d_records, cap, d_counter, d_user_flags, out_total))
    return rc;
  if (!permutation_columns || !d_copies) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_permutation == 0 || n_permutation > GE_MAX_COLUMNS || ((uint64_t)n_permutation << k) > ((uint64_t)1 << 32))
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 .. 256 permutation columns and columns * 2^k <= 2^32");
  for (size_t j = 0; j < n_permutation; ++j)
    if (permutation_columns[j] >= n_columns) return hm_fail(HM_ERR_BAD_ARG, who + ": a permutation column is not in the table");
  if ((uintptr_t)d_copies & 7u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_copies is not 8-byte aligned");
  if (n_copies == 0 || n_copies > ((size_t)1 << 30) || (uint64_t)m * n_copies > ((uint64_t)1 << 40))
    return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_copies <= 2^30 and m * n_copies <= 2^40");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const MockTable table{column_bases, column_strides, column_rows, n_columns};
  const MockSink sink{d_records, cap, d_counter, d_user_flags};
  if (int rc = mock_copies_run(*ctx, table, permutation_columns, n_permutation, d_copies, n_copies, k, m, sink, (hipStream_t)stream)) return rc;
  return mock_total(d_counter, out_total, (hipStream_t)stream);
} HM_API_CATCH("hm_mock_copies_dev")

int hm_mock_lookup_dev(uint64_t graph, const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows,
                       size_t n_columns, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t k, uint32_t usable_rows, size_t m,
                       uint32_t user_base, const void* d_table_values, uint64_t* d_records, size_t cap, uint64_t* d_counter,
                       uint8_t* d_user_flags, uint64_t* out_total, void* stream) try {
  const std::string who = "hm_mock_lookup_dev";
  if (int rc = mock_args(who, column_bases, column_strides, column_rows, n_columns, k, m, user_base, d_records, cap, d_counter, d_user_flags,
                         out_total))
    return rc;
  if ((n_dynamic && !dynamic_constants) || !d_table_values) return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if ((uintptr_t)d_table_values & 15u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_table_values is not 16-byte aligned");
  if (usable_rows == 0 || usable_rows > ((uint64_t)1 << k)) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= usable_rows <= 2^k");
  if ((uint64_t)m * usable_rows > ((uint64_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, who + ": m * usable_rows > 2^32");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  GraphProgram* g = mock_program(*ctx, graph);
  if (!g) return hm_fail(HM_ERR_NOT_FOUND, who + ": unknown program handle");
  const MockTable table{column_bases, column_strides, column_rows, n_columns};
  const MockSink sink{d_records, cap, d_counter, d_user_flags};
  if (int rc = mock_program_run(*ctx, *g, table, dynamic_constants, n_dynamic, k, usable_rows, m, user_base, nullptr, 0,
                                (const uint32_t*)d_table_values, sink, (hipStream_t)stream))
    return rc;
  return mock_total(d_counter, out_total, (hipStream_t)stream);
} HM_API_CATCH("hm_mock_lookup_dev")

}  // extern "C"
