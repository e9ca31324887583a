// capi_g1.hip -- the G1 entry points of the C ABI outside the MSM: fixed-base multiples, best_fft over G1 (g1_fft.hip), all KZG openings
// of a polynomial (g1_fft.hip), the pairing operands of ledger openings (ledger.hip) and the SRS point encodings (g1_codec.hip).
#include <hip/hip_runtime.h>

#include <string>

#include "hm_internal.h"

using namespace hm;

extern "C" {

int hm_g1_fixed_base_mul_dev(const void* d_scalars, size_t n, const uint64_t base_xy[8], void* d_out_xy, void* stream) try {
  if ((n && (!d_scalars || !d_out_xy)) || !base_xy) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_fixed_base_mul_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return g1_fixed_base_mul_run(*ctx, (const uint32_t*)d_scalars, n, base_xy, (uint32_t*)d_out_xy, (hipStream_t)stream);
} HM_API_CATCH("hm_g1_fixed_base_mul_dev")

int hm_g1_fft_bn256_dev(void* d_points_xy, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale, void* stream) try {
  if (!d_points_xy || !omega) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_fft_bn256_dev: null argument");
  if (log_n > 24) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_fft_bn256_dev: log_n > 24");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return g1_fft_run(*ctx, (uint32_t*)d_points_xy, 16, omega, log_n, scale, (hipStream_t)stream);
} HM_API_CATCH("hm_g1_fft_bn256_dev")

int hm_g1_fft_bn256(uint64_t* points_xyz, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale) try {
  if (!points_xyz || !omega) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_fft_bn256: null argument");
  if (log_n > 24) return hm_fail(HM_ERR_BAD_ARG, "hm_g1_fft_bn256: log_n > 24");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const size_t bytes = ((size_t)96) << log_n;
  const HostIn in{points_xyz, bytes, 0};
  const HostOut out{points_xyz, bytes, 0, false};
  return host_round_trip("hm_g1_fft_bn256", *ctx, "g1_fft", bytes, &in, 1, &out, 1,
                         [&](uint8_t* d) { return g1_fft_run(*ctx, (uint32_t*)d, 24, omega, log_n, scale, nullptr); });
} HM_API_CATCH("hm_g1_fft_bn256")

// ---- all KZG openings of a polynomial on its domain (g1_fft.hip) ---------------------------------------------------------------
int hm_kzg_open_table_bn256_dev(const void* d_g_xy, uint32_t log_n, void* d_table_xy, void* stream) try {
  if (!d_g_xy || !d_table_xy) return hm_fail(HM_ERR_BAD_ARG, "hm_kzg_open_table_bn256_dev: null argument");
  if (log_n > 23) return hm_fail(HM_ERR_BAD_ARG, "hm_kzg_open_table_bn256_dev: log_n > 23");
  if (ranges_overlap(d_g_xy, (size_t)64 << log_n, d_table_xy, (size_t)128 << log_n))
    return hm_fail(HM_ERR_BAD_ARG, "hm_kzg_open_table_bn256_dev: the table overlaps the points");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return kzg_open_table_run(*ctx, (const uint32_t*)d_g_xy, log_n, (uint32_t*)d_table_xy, (hipStream_t)stream);
} HM_API_CATCH("hm_kzg_open_table_bn256_dev")

static int kzg_open_all_entry(const char* who, const void* d_table_xy, const void* d_coeffs, uint32_t log_n, size_t count, void* d_proofs_xy,
                              double* part_ms, void* stream) {
  if (!d_table_xy || (count && (!d_coeffs || !d_proofs_xy))) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (log_n > 23) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": log_n > 23");
  if (count > 65535) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": count > 65535");
  const size_t n = (size_t)1 << log_n;
  if (count && (ranges_overlap(d_proofs_xy, count * n * 64, d_table_xy, n * 128) || ranges_overlap(d_proofs_xy, count * n * 64, d_coeffs, count * n * 32)))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the proofs overlap an input");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return kzg_open_all_run(*ctx, (const uint32_t*)d_table_xy, (const uint32_t*)d_coeffs, log_n, count, (uint32_t*)d_proofs_xy,
                          (hipStream_t)stream, part_ms);
}

int hm_kzg_open_all_bn256_dev(const void* d_table_xy, const void* d_coeffs, uint32_t log_n, size_t count, void* d_proofs_xy,
                              void* stream) try {
  return kzg_open_all_entry("hm_kzg_open_all_bn256_dev", d_table_xy, d_coeffs, log_n, count, d_proofs_xy, nullptr, stream);
} HM_API_CATCH("hm_kzg_open_all_bn256_dev")

int hm_kzg_open_all_timed_bn256_dev(const void* d_table_xy, const void* d_coeffs, uint32_t log_n, size_t count, void* d_proofs_xy,
                                    double out_part_ms[7], void* stream) try {
  if (!out_part_ms || count == 0) return hm_fail(HM_ERR_BAD_ARG, "hm_kzg_open_all_timed_bn256_dev: null argument or no polynomial");
  return kzg_open_all_entry("hm_kzg_open_all_timed_bn256_dev", d_table_xy, d_coeffs, log_n, count, d_proofs_xy, out_part_ms, stream);
} HM_API_CATCH("hm_kzg_open_all_timed_bn256_dev")

// ---- ledger openings: every user's pairing operands (ledger.hip) ---------------------------------------------------------------
int hm_kzg_ledger_pairs_bn256_dev(const void* d_openings_xy, const uint32_t* d_indices, const void* d_ids, const void* d_balances,
                                  const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8], uint32_t log_n,
                                  uint32_t assets, size_t n_users, void* d_g1_xy, uint32_t* d_flags, void* stream) try {
  const std::string who = "hm_kzg_ledger_pairs_bn256_dev";
  if (!d_openings_xy || !d_indices || !d_ids || (assets && !d_balances) || !gamma || !omega || !c_gamma || !d_g1_xy || !d_flags)
    return hm_fail(HM_ERR_BAD_ARG, who + ": null argument");
  if (n_users == 0 || n_users > ((size_t)1 << 20)) return hm_fail(HM_ERR_BAD_ARG, who + ": need 1 <= n_users <= 2^20");
  if (log_n > 28) return hm_fail(HM_ERR_BAD_ARG, who + ": log_n > 28");
  if (assets > (1u << 16)) return hm_fail(HM_ERR_BAD_ARG, who + ": assets > 2^16");
  if (const char* problem = kzg_ledger_words_problem(gamma, omega, c_gamma)) return hm_fail(HM_ERR_BAD_ARG, who + ": " + problem);
  if (((uintptr_t)d_openings_xy | (uintptr_t)d_ids | (uintptr_t)d_balances | (uintptr_t)d_g1_xy) & 15u)
    return hm_fail(HM_ERR_BAD_ARG, who + ": a buffer is not 16-byte aligned");
  if (((uintptr_t)d_indices | (uintptr_t)d_flags) & 3u) return hm_fail(HM_ERR_BAD_ARG, who + ": d_indices / d_flags is not 4-byte aligned");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return kzg_ledger_pairs_run((const uint32_t*)d_openings_xy, d_indices, (const uint32_t*)d_ids, (const uint32_t*)d_balances, gamma, omega,
                              c_gamma, log_n, assets, n_users, (uint32_t*)d_g1_xy, d_flags, (hipStream_t)stream);
} HM_API_CATCH("hm_kzg_ledger_pairs_bn256_dev")

// ---- SRS point encodings (g1_codec.inc) --------------------------------------------------------------------------------------
static constexpr size_t G1_CODEC_MAX_N = (size_t)1 << 30;

static int g1_codec_args(const char* who, size_t n, const void* in, const void* out, bool has_out, const uint64_t* first_invalid,
                         bool has_flag) {
  if ((n && (!in || (has_out && !out))) || (has_flag && !first_invalid)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (n > G1_CODEC_MAX_N) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": n > 2^30");
  return HM_OK;
}

int hm_g1_compress_bn256_dev(const void* d_points_xy, size_t n, void* d_out32, void* stream) try {
  if (int rc = g1_codec_args("hm_g1_compress_bn256_dev", n, d_points_xy, d_out32, true, nullptr, false)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return g1_compress_run((const uint32_t*)d_points_xy, n, (uint32_t*)d_out32, (hipStream_t)stream);
} HM_API_CATCH("hm_g1_compress_bn256_dev")

int hm_g1_decompress_bn256_dev(const void* d_in32, size_t n, void* d_points_xy, uint64_t* out_first_invalid, void* stream) try {
  if (int rc = g1_codec_args("hm_g1_decompress_bn256_dev", n, d_in32, d_points_xy, true, out_first_invalid, true)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return g1_decompress_run((const uint32_t*)d_in32, n, (uint32_t*)d_points_xy, out_first_invalid, (hipStream_t)stream);
} HM_API_CATCH("hm_g1_decompress_bn256_dev")

int hm_g1_check_bn256_dev(const void* d_points_xy, size_t n, uint64_t* out_first_invalid, void* stream) try {
  if (int rc = g1_codec_args("hm_g1_check_bn256_dev", n, d_points_xy, nullptr, false, out_first_invalid, true)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return g1_check_run((const uint32_t*)d_points_xy, n, out_first_invalid, (hipStream_t)stream);
} HM_API_CATCH("hm_g1_check_bn256_dev")

// Host forms: input and output share one staging buffer (input first); the caller's output is written only by the last copy.
int hm_g1_compress_bn256(const uint64_t* points_xy, size_t n, uint8_t* out32) try {
  if (int rc = g1_codec_args("hm_g1_compress_bn256", n, points_xy, out32, true, nullptr, false)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (n == 0) return HM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const HostIn in{points_xy, n * 64, 0};
  const HostOut out{out32, n * 32, n * 64, false};
  return host_round_trip("hm_g1_compress_bn256", *ctx, "g1_codec", n * 96, &in, 1, &out, 1,
                         [&](uint8_t* d) { return g1_compress_run((const uint32_t*)d, n, (uint32_t*)(d + n * 64), nullptr); });
} HM_API_CATCH("hm_g1_compress_bn256")

int hm_g1_decompress_bn256(const uint8_t* in32, size_t n, uint64_t* points_xy, uint64_t* out_first_invalid) try {
  if (int rc = g1_codec_args("hm_g1_decompress_bn256", n, in32, points_xy, true, out_first_invalid, true)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  *out_first_invalid = n;
  if (n == 0) return HM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const HostIn in{in32, n * 32, 0};
  const HostOut out{points_xy, n * 64, n * 32, false};
  // HM_ERR_INVALID_DATA comes back from the launch: the caller's array is untouched
  return host_round_trip("hm_g1_decompress_bn256", *ctx, "g1_codec", n * 96, &in, 1, &out, 1, [&](uint8_t* d) {
    return g1_decompress_run((const uint32_t*)d, n, (uint32_t*)(d + n * 32), out_first_invalid, nullptr);
  });
} HM_API_CATCH("hm_g1_decompress_bn256")

int hm_g1_check_bn256(const uint64_t* points_xy, size_t n, uint64_t* out_first_invalid) try {
  if (int rc = g1_codec_args("hm_g1_check_bn256", n, points_xy, nullptr, false, out_first_invalid, true)) return rc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  *out_first_invalid = n;
  if (n == 0) return HM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const HostIn in{points_xy, n * 64, 0};
  return host_round_trip("hm_g1_check_bn256", *ctx, "g1_codec", n * 64, &in, 1, nullptr, 0,
                         [&](uint8_t* d) { return g1_check_run((const uint32_t*)d, n, out_first_invalid, nullptr); });
} HM_API_CATCH("hm_g1_check_bn256")

}  // extern "C"
