// capi_poly.hip -- the field-side entry points of the C ABI: NTT and evaluation-domain forms, polynomial and vector steps, the lookup
// argument's columns, the hm_graph_* programs and the quotient entry points.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "graph_lower.h"
#include "hm_internal.h"
#include "host_fr.h"

using namespace hm;

extern "C" {

static void count_vector(DeviceCtx& ctx, int kind, uint64_t calls, uint64_t elements) {   // ctx.mu held
  ctx.calls.vector_calls[kind] += calls;
  ctx.calls.vector_elements[kind] += elements;
}

static void count_ntt(DeviceCtx& ctx, uint32_t log_n, size_t batch) {
  ctx.calls.ntt_calls += batch;
  ctx.calls.ntt_elements += (uint64_t)batch << log_n;
  ctx.calls.ntt_by_log[log_n & 31] += batch;
}
// the three spans of a host form's round trip (host_round_trip)
static void count_ntt_spans(DeviceCtx& ctx, const HostSpans& t) {
  ctx.calls.ntt_h2d_us += t.h2d_us;
  ctx.calls.ntt_device_us += t.device_us;
  ctx.calls.ntt_d2h_us += t.d2h_us;
}

// ---- the NTT entries: each states its call (ntt_plan.inc: NttCall) and its pointers; ntt_entry does the rest ----
static NttCall ntt_call(uint32_t log_n, uint64_t batch, uint32_t fused) {
  NttCall c{};
  c.log_n = log_n, c.batch = batch, c.fused = fused;
  return c;
}
static NttPointers ntt_pointers(void* d_a, const uint64_t* omega, const uint64_t* scale = nullptr, const uint64_t* coset = nullptr,
                                const uint64_t* post3 = nullptr) {
  NttPointers p;
  p.d_a = (uint32_t*)d_a, p.omega = omega, p.scale = scale, p.coset = coset, p.post3 = post3;
  return p;
}
// what needs neither a device nor the context: null arguments, then ntt_check_call's refusals under the entry's name
static int ntt_refuse(const char* who, bool null_argument, const NttCall& bound) {
  if (null_argument) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (const char* why = ntt_check_call(bound)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": " + why);
  return HM_OK;
}
// every device-pointer NTT entry: the refusals, the context and its lock, ntt_run, the call counter
static int ntt_entry(const char* who, bool null_argument, const NttCall& call, const NttPointers& p, void* stream) {
  if (const int refused = ntt_refuse(who, null_argument, ntt_bind(call, p))) return refused;
  if (ntt_call_arrays(call) == 0) return HM_OK;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = ntt_run(*ctx, call, p, (hipStream_t)stream);
  if (rc == HM_OK) count_ntt(*ctx, call.log_n, (size_t)ntt_call_arrays(call));
  return rc;
}
// every host-pointer NTT entry, one array: the refusals, the context and its lock, the round trip through ctx.io with `launch` on
// the staging buffer between the copies, the counters.  The caller's arrays are written by the download alone.
static int ntt_host_entry(const char* who, bool null_argument, const NttCall& call, size_t staging_bytes, const HostIn& in, const HostOut& out,
                          const std::function<int(DeviceCtx&, uint8_t*)>& launch) {
  NttCall staged = call;                     // the arrays will lie in the staging buffer: aligned, the extending form's two apart
  staged.in_place = call.log_z == 0;
  if (const int refused = ntt_refuse(who, null_argument, staged)) return refused;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostSpans t;
  const int rc = host_round_trip(who, *ctx, nullptr, staging_bytes, &in, 1, &out, 1, [&](uint8_t* d) { return launch(*ctx, d); }, &t);
  if (rc != HM_OK) return rc;
  count_ntt(*ctx, call.log_n, 1);
  count_ntt_spans(*ctx, t);
  return HM_OK;
}

int hm_ntt_bn256_fr_dev(void* d_a, const uint64_t omega[4], uint32_t log_n, void* stream) try {
  return ntt_entry("hm_ntt_bn256_fr_dev", !d_a || !omega, ntt_call(log_n, 1, 0), ntt_pointers(d_a, omega), stream);
} HM_API_CATCH("hm_ntt_bn256_fr_dev")

int hm_ntt_batch_bn256_fr_dev(void* d_a, size_t batch, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale,
                              const uint64_t* coset, void* stream) try {
  return ntt_entry("hm_ntt_batch_bn256_fr_dev", (batch && !d_a) || !omega,
                   ntt_call(log_n, batch, (scale ? NTT_F_SCALE : 0u) | (coset ? NTT_F_COSET3 : 0u)), ntt_pointers(d_a, omega, scale, coset), stream);
} HM_API_CATCH("hm_ntt_batch_bn256_fr_dev")

int hm_ifft_bn256_fr_dev(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void* stream) try {
  return ntt_entry("hm_ifft_bn256_fr_dev", !d_a || !omega_inv || !divisor, ntt_call(log_n, 1, NTT_F_SCALE), ntt_pointers(d_a, omega_inv, divisor),
                   stream);
} HM_API_CATCH("hm_ifft_bn256_fr_dev")

int hm_coset_ntt_bn256_fr_dev(void* d_a, const uint64_t omega[4], uint32_t log_n, const uint64_t coset[12], void* stream) try {
  return ntt_entry("hm_coset_ntt_bn256_fr_dev", !d_a || !omega || !coset, ntt_call(log_n, 1, NTT_F_COSET3), ntt_pointers(d_a, omega, nullptr, coset),
                   stream);
} HM_API_CATCH("hm_coset_ntt_bn256_fr_dev")

int hm_extended_to_coeff_bn256_fr_dev(void* d_a, size_t batch, const uint64_t extended_omega_inv[4], uint32_t log_ext,
                                      const uint64_t divisor[4], const uint64_t coset_inv[12], void* stream) try {
  return ntt_entry("hm_extended_to_coeff_bn256_fr_dev", (batch && !d_a) || !extended_omega_inv || !divisor || !coset_inv,
                   ntt_call(log_ext, batch, NTT_F_SCALE | NTT_F_POST3), ntt_pointers(d_a, extended_omega_inv, divisor, nullptr, coset_inv), stream);
} HM_API_CATCH("hm_extended_to_coeff_bn256_fr_dev")

// EvaluationDomain::coeff_to_extended as a call: the extending form where the plan has it (the zero part of the padded arrays is then
// neither written nor read), else -- small or un-extended domains -- the ordinary in-place transform of the materialised arrays.
static NttCall extended_call(uint64_t batch, uint32_t log_n, uint32_t log_ext, bool coset) {
  NttCall c = ntt_call(log_ext, batch, coset ? NTT_F_COSET3 : 0u);
  c.log_z = log_ext - log_n;                                   // log_n > log_ext wraps: refused as longer than the transform
  if (c.log_z <= log_ext && !ntt_extending_applies(log_ext, c.log_z)) c.log_z = 0;
  return c;
}
// ctx.mu is held by the caller, who has checked `call` (extended_call's) against these pointers.
static int coeff_to_extended_locked(DeviceCtx& ctx, const NttCall& call, const void* d_coeffs, void* d_ext, uint32_t log_n,
                                    const uint64_t extended_omega[4], const uint64_t* coset, hipStream_t stream) {
  NttPointers p = ntt_pointers(d_ext, extended_omega, nullptr, coset);
  if (call.log_z) {
    p.d_in = (const uint32_t*)d_coeffs;
  } else if (d_coeffs != d_ext || log_n != call.log_n) {
    const size_t row_in = (size_t)32 << log_n, row_out = (size_t)32 << call.log_n;
    if (log_n != call.log_n) HM_HIP_CHECK(hipMemsetAsync(d_ext, 0, row_out * call.batch, stream));
    HM_HIP_CHECK(hipMemcpy2DAsync(d_ext, row_out, d_coeffs, row_in, row_in, call.batch, hipMemcpyDeviceToDevice, stream));
  }
  return ntt_run(ctx, call, p, stream);
}

int hm_coeff_to_extended_bn256_fr_dev(const void* d_coeffs, void* d_ext, size_t batch, const uint64_t extended_omega[4],
                                      uint32_t log_n, uint32_t log_ext, const uint64_t* coset, void* stream) try {
  const NttCall call = extended_call(batch, log_n, log_ext, coset != nullptr);
  const char* who = "hm_coeff_to_extended_bn256_fr_dev";
  NttPointers at = ntt_pointers(d_ext, extended_omega);
  if (call.log_z) at.d_in = (const uint32_t*)d_coeffs;
  if (const int refused = ntt_refuse(who, (batch && (!d_coeffs || !d_ext)) || !extended_omega, ntt_bind(call, at))) return refused;
  if (batch == 0) return HM_OK;
  // Without the extending form the padded arrays are materialised at d_ext first (the transform itself is in place there): d_coeffs is
  // held to the same alignment, and an overlapping d_coeffs would not survive the padding (d_ext == d_coeffs with nothing to pad is
  // the in-place transform).
  if (!call.log_z && (d_coeffs != d_ext || log_n != log_ext)) {
    if ((uintptr_t)d_coeffs & 15) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a data pointer is not 16-byte aligned");
    if (ranges_overlap(d_coeffs, ((size_t)32 << log_n) * batch, d_ext, ((size_t)32 << log_ext) * batch))
      return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": output partially overlaps the coefficients");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = coeff_to_extended_locked(*ctx, call, d_coeffs, d_ext, log_n, extended_omega, coset, (hipStream_t)stream);
  if (rc == HM_OK) count_ntt(*ctx, log_ext, batch);
  return rc;
} HM_API_CATCH("hm_coeff_to_extended_bn256_fr_dev")

int hm_coeff_to_coset_bn256_fr_dev(const void* d_coeffs, void* d_out, size_t batch, const uint64_t omega[4], uint32_t log_n,
                                   const uint64_t shift[4], int columns_internal, void* stream) try {
  NttPointers p = ntt_pointers(d_out, omega);
  if (d_coeffs != d_out) p.d_in = (const uint32_t*)d_coeffs;
  p.shifts = shift, p.internal = columns_internal != 0;
  return ntt_entry("hm_coeff_to_coset_bn256_fr_dev", (batch && (!d_coeffs || !d_out)) || !omega || !shift, ntt_call(log_n, batch, NTT_F_IN_TABLE), p,
                   stream);
} HM_API_CATCH("hm_coeff_to_coset_bn256_fr_dev")

int hm_coeff_to_cosets_bn256_fr_dev(const void* d_coeffs, void* d_out, size_t batch, const uint64_t omega[4], uint32_t log_n,
                                    const uint64_t* shifts, size_t count, int columns_internal, void* stream) try {
  NttCall call = ntt_call(log_n, batch, NTT_F_IN_TABLES);
  call.fwd_cosets = count > NTT_COSETS_MAX ? NTT_COSETS_MAX + 1 : (uint32_t)count;
  NttPointers p = ntt_pointers(d_out, omega);
  p.d_in = (const uint32_t*)d_coeffs, p.shifts = shifts, p.internal = columns_internal != 0;
  return ntt_entry("hm_coeff_to_cosets_bn256_fr_dev", (batch && count && (!d_coeffs || !d_out)) || !omega || (count && !shifts), call, p, stream);
} HM_API_CATCH("hm_coeff_to_cosets_bn256_fr_dev")

int hm_coset_to_coeff_bn256_fr_dev(void* d_a, size_t batch, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4],
                                   const uint64_t shift_inv[4], void* stream) try {
  NttPointers p = ntt_pointers(d_a, omega_inv, divisor);
  p.shifts = shift_inv;
  return ntt_entry("hm_coset_to_coeff_bn256_fr_dev", (batch && !d_a) || !omega_inv || !divisor || !shift_inv,
                   ntt_call(log_n, batch, NTT_F_SCALE | NTT_F_OUT_TABLE), p, stream);
} HM_API_CATCH("hm_coset_to_coeff_bn256_fr_dev")

int hm_cosets_to_coeff_bn256_fr_dev(void* d_a, size_t count, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4],
                                    const uint64_t* shift_invs, void* stream) try {
  NttCall call = ntt_call(log_n, 1, NTT_F_SCALE | NTT_F_OUT_TABLES);
  call.inv_cosets = count > NTT_COSETS_MAX ? NTT_COSETS_MAX + 1 : (uint32_t)count;
  NttPointers p = ntt_pointers(d_a, omega_inv, divisor);
  p.shifts = shift_invs;
  return ntt_entry("hm_cosets_to_coeff_bn256_fr_dev", (count && (!d_a || !shift_invs)) || !omega_inv || !divisor, call, p, stream);
} HM_API_CATCH("hm_cosets_to_coeff_bn256_fr_dev")

// Host-pointer forms: only what upstream's arrays really hold crosses PCIe -- the 2^log_n coefficients up (never the zero padding),
// the first `keep` coefficients down (never the part extended_to_coeff truncates).
int hm_ntt_bn256_fr(uint64_t* a, const uint64_t omega[4], uint32_t log_n) try {
  const NttCall call = ntt_call(log_n, 1, 0);
  const size_t bytes = (size_t)32 << (log_n & 31);
  return ntt_host_entry("hm_ntt_bn256_fr", !a || !omega, call, bytes, HostIn{a, bytes, 0}, HostOut{a, bytes, 0, false},
                        [&](DeviceCtx& ctx, uint8_t* d) { return ntt_run(ctx, call, ntt_pointers(d, omega), nullptr); });
} HM_API_CATCH("hm_ntt_bn256_fr")

int hm_coeff_to_extended_bn256_fr(const uint64_t* coeffs, uint64_t* ext, const uint64_t extended_omega[4], uint32_t log_n,
                                  uint32_t log_ext, const uint64_t* coset) try {
  const NttCall call = extended_call(1, log_n, log_ext, coset != nullptr);
  const size_t bytes_in = (size_t)32 << (log_n & 31), bytes_out = (size_t)32 << (log_ext & 31);
  // staging: [the extended array][the coefficients].  `ext` is written by the download alone (it may be the very allocation `coeffs`
  // lives in: the input has been uploaded whole).  It is normally a FRESH allocation (the new Vec of the result): its first-touch page
  // faults are taken by xfer_prefault's threads, under the transform, or by the lanes' copying threads.
  return ntt_host_entry("hm_coeff_to_extended_bn256_fr", !coeffs || !ext || !extended_omega, call, bytes_out + bytes_in,
                        HostIn{coeffs, bytes_in, bytes_out}, HostOut{ext, bytes_out, 0, false}, [&](DeviceCtx& ctx, uint8_t* d) {
                          const int rc = coeff_to_extended_locked(ctx, call, d + bytes_out, d, log_n, extended_omega, coset, nullptr);
                          if (rc == HM_OK && xfer_mode(ext, bytes_out) == 0) xfer_prefault(ext, bytes_out);   // direct copies only
                          return rc;
                        });
} HM_API_CATCH("hm_coeff_to_extended_bn256_fr")

int hm_extended_to_coeff_bn256_fr(uint64_t* a, size_t keep, const uint64_t extended_omega_inv[4], uint32_t log_ext,
                                  const uint64_t divisor[4], const uint64_t coset_inv[12]) try {
  const char* who = "hm_extended_to_coeff_bn256_fr";
  if (!a || !extended_omega_inv || !divisor || !coset_inv) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (log_ext <= NTT_LOG_N_MAX && keep > ((size_t)1 << log_ext)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": keep exceeds 2^log_ext");
  const NttCall call = ntt_call(log_ext, 1, NTT_F_SCALE | NTT_F_POST3);
  const size_t bytes = (size_t)32 << (log_ext & 31);
  return ntt_host_entry(who, false, call, bytes, HostIn{a, bytes, 0}, HostOut{a, keep * 32, 0, false},      // the truncated part is never downloaded
                        [&](DeviceCtx& ctx, uint8_t* d) { return ntt_run(ctx, call, ntt_pointers(d, extended_omega_inv, divisor, nullptr, coset_inv), nullptr); });
} HM_API_CATCH("hm_extended_to_coeff_bn256_fr")

int hm_eval_polynomial_bn256_fr_dev(const void* d_polys, size_t n, const uint32_t* poly_index, const uint64_t* points, size_t count,
                                    uint64_t* out, void* stream) try {
  if ((count && (!points || !out)) || (count && n && !d_polys))
    return hm_fail(HM_ERR_BAD_ARG, "hm_eval_polynomial_bn256_fr_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_EVAL_POLYNOMIAL, count, (uint64_t)count * n);
  return fr_eval_polynomial_run(*ctx, (const uint32_t*)d_polys, n, poly_index, points, count, out, (hipStream_t)stream);
} HM_API_CATCH("hm_eval_polynomial_bn256_fr_dev")

int hm_kate_division_bn256_fr_dev(const void* d_poly, size_t n, const uint64_t z[4], void* d_quotient, void* stream) try {
  if (!z || (n >= 2 && (!d_poly || !d_quotient))) return hm_fail(HM_ERR_BAD_ARG, "hm_kate_division_bn256_fr_dev: null argument");
  if (n >= 2) {
    const char *a = (const char*)d_poly, *q = (const char*)d_quotient;
    if (q < a + n * 32 && a < q + (n - 1) * 32)
      return hm_fail(HM_ERR_BAD_ARG, "hm_kate_division_bn256_fr_dev: quotient overlaps the polynomial");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_KATE_DIVISION, 1, n);
  return fr_kate_division_run(*ctx, (const uint32_t*)d_poly, n, z, (uint32_t*)d_quotient, (hipStream_t)stream);
} HM_API_CATCH("hm_kate_division_bn256_fr_dev")

int hm_fr_grand_product_dev(const void* d_factors, size_t n, const uint64_t start[4], void* d_out, void* stream) try {
  if (!start || (n && (!d_factors || !d_out))) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_grand_product_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_GRAND_PRODUCT, 1, n);
  return fr_grand_product_run(*ctx, (const uint32_t*)d_factors, n, start, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_grand_product_dev")

int hm_kate_division_batch_bn256_fr_dev(const void* const* d_polys, size_t n, const uint64_t* z, void* const* d_quotients, size_t count,
                                        void* stream) try {
  if (count == 0) return HM_OK;
  if (!z || !d_polys || !d_quotients) return hm_fail(HM_ERR_BAD_ARG, "hm_kate_division_batch_bn256_fr_dev: null argument");
  if (n >= 2) {
    for (size_t j = 0; j < count; ++j)
      if (!d_polys[j] || !d_quotients[j]) return hm_fail(HM_ERR_BAD_ARG, "hm_kate_division_batch_bn256_fr_dev: null device pointer");
    for (size_t j = 0; j < count; ++j)
      for (size_t i = 0; i < count; ++i)
        if (ranges_overlap(d_quotients[j], (n - 1) * 32, d_polys[i], n * 32) ||
            (i != j && ranges_overlap(d_quotients[j], (n - 1) * 32, d_quotients[i], (n - 1) * 32)))
          return hm_fail(HM_ERR_BAD_ARG, "hm_kate_division_batch_bn256_fr_dev: a quotient overlaps another array of the call");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_KATE_DIVISION, count, (uint64_t)count * n);
  return fr_kate_division_batch_run(*ctx, d_polys, n, z, d_quotients, count, (hipStream_t)stream);
} HM_API_CATCH("hm_kate_division_batch_bn256_fr_dev")

int hm_fr_grand_product_batch_dev(const void* const* d_factors, size_t n, const uint64_t start[4], size_t chain_row, void* const* d_out,
                                  size_t count, void* stream) try {
  if (count == 0) return HM_OK;
  if (!start || !d_factors || !d_out) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_grand_product_batch_dev: null argument");
  if (n) {
    for (size_t j = 0; j < count; ++j)
      if (!d_factors[j] || !d_out[j]) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_grand_product_batch_dev: null device pointer");
    for (size_t j = 0; j < count; ++j)
      for (size_t i = 0; i < count; ++i)
        if (i != j && (ranges_overlap(d_out[j], n * 32, d_factors[i], n * 32) || ranges_overlap(d_out[j], n * 32, d_out[i], n * 32)))
          return hm_fail(HM_ERR_BAD_ARG, "hm_fr_grand_product_batch_dev: an output overlaps another column of the call");
    for (size_t j = 0; j < count; ++j)
      if (d_out[j] != d_factors[j] && ranges_overlap(d_out[j], n * 32, d_factors[j], n * 32))
        return hm_fail(HM_ERR_BAD_ARG, "hm_fr_grand_product_batch_dev: an output partially overlaps its factors");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_GRAND_PRODUCT, count, (uint64_t)count * n);
  return fr_grand_product_batch_run(*ctx, d_factors, n, start, chain_row < n ? chain_row : n, d_out, count, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_grand_product_batch_dev")

int hm_fr_batch_invert_dev(void* d_values, size_t n, void* stream) try {
  if (n && !d_values) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_batch_invert_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    count_vector(*ctx, HM_STAT_BATCH_INVERT, 1, n);
  }
  return fr_batch_invert_run((uint32_t*)d_values, n, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_batch_invert_dev")

int hm_fr_linear_combination_dev(const void* const* d_polys, const uint64_t* coeffs, size_t count, size_t n, void* d_out,
                                 void* stream) try {
  if ((n && !d_out) || (count && (!d_polys || !coeffs))) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_linear_combination_dev: null argument");
  if (n)
    for (size_t j = 0; j < count; ++j)
      if (!d_polys[j]) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_linear_combination_dev: null polynomial");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, 1, (uint64_t)count * n);
  }
  return fr_linear_combination_run(d_polys, coeffs, count, n, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_linear_combination_dev")

int hm_shplonk_set_quotient_bn256_fr_dev(const void* const* d_polys, const uint64_t* weights, size_t m, size_t n, const uint64_t* points,
                                         size_t t, const uint64_t scale[4], void* d_out, int accumulate, void* stream) try {
  const char* who = "hm_shplonk_set_quotient_bn256_fr_dev";
  if (!d_polys || !weights || !points || !scale || !d_out) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (m == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": no polynomial");
  if (t == 0 || t > (size_t)HM_SHPLONK_MAX_POINTS) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": need 1 <= t <= HM_SHPLONK_MAX_POINTS");
  if (n < t + 1 || n > ((size_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": need t + 1 <= n <= 2^32");
  if ((uintptr_t)d_out & 15) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the output is not 16-byte aligned");
  for (size_t j = 0; j < m; ++j)
    if (!d_polys[j] || ((uintptr_t)d_polys[j] & 15)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a null or misaligned polynomial");
  for (size_t a = 0; a < t; ++a)
    for (size_t b = a + 1; b < t; ++b)
      if (host::fr_eq(host::fr_load(points + a * 4), host::fr_load(points + b * 4)))
        return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": two equal points");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, 1, (uint64_t)m * n);
    count_vector(*ctx, HM_STAT_KATE_DIVISION, t, (uint64_t)t * n);
  }
  return fr_shplonk_set_quotient_run(d_polys, weights, m, n, points, (uint32_t)t, scale, (uint32_t*)d_out, accumulate != 0, (hipStream_t)stream);
} HM_API_CATCH("hm_shplonk_set_quotient_bn256_fr_dev")

int hm_fr_linear_combination_batch_dev(const void* const* d_polys, const uint64_t* coeffs, size_t count, size_t n, void* const* d_outs,
                                       size_t proofs, void* stream) try {
  const char* who = "hm_fr_linear_combination_batch_dev";
  if ((proofs && !d_outs) || (proofs && count && (!d_polys || !coeffs))) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (n) {
    for (size_t b = 0; b < proofs; ++b)
      if (!d_outs[b]) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null output");
    for (size_t j = 0; j < proofs * count; ++j)
      if (!d_polys[j]) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null polynomial");
    if (const char* why = fr_batch_alias_check(d_polys, count, d_outs, proofs)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": " + why);
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, proofs, (uint64_t)proofs * count * n);
  }
  return fr_linear_combination_batch_run(d_polys, coeffs, count, n, d_outs, proofs, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_linear_combination_batch_dev")

int hm_shplonk_set_quotient_batch_bn256_fr_dev(const void* const* d_polys, const uint64_t* weights, size_t m, size_t n, const uint64_t* points,
                                               size_t t, const uint64_t* scales, void* const* d_outs, int accumulate, size_t proofs,
                                               void* stream) try {
  const char* who = "hm_shplonk_set_quotient_batch_bn256_fr_dev";
  if (!d_polys || !weights || !points || !scales || !d_outs) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (proofs == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": no proof");
  if (m == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": no polynomial");
  if (t == 0 || t > (size_t)HM_SHPLONK_MAX_POINTS) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": need 1 <= t <= HM_SHPLONK_MAX_POINTS");
  if (n < t + 1 || n > ((size_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": need t + 1 <= n <= 2^32");
  for (size_t b = 0; b < proofs; ++b) {
    if (!d_outs[b] || ((uintptr_t)d_outs[b] & 15)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a null or misaligned output");
    for (size_t j = 0; j < m; ++j)
      if (!d_polys[b * m + j] || ((uintptr_t)d_polys[b * m + j] & 15))
        return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a null or misaligned polynomial");
    for (size_t a = 0; a < t; ++a)
      for (size_t c = a + 1; c < t; ++c)
        if (host::fr_eq(host::fr_load(points + (b * t + a) * 4), host::fr_load(points + (b * t + c) * 4)))
          return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": two equal points");
  }
  if (const char* why = fr_batch_alias_check(d_polys, m, d_outs, proofs)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": " + why);
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, proofs, (uint64_t)proofs * m * n);
    count_vector(*ctx, HM_STAT_KATE_DIVISION, proofs * t, (uint64_t)proofs * t * n);
  }
  return fr_shplonk_set_quotient_batch_run(d_polys, weights, m, n, points, (uint32_t)t, scales, d_outs, accumulate != 0, proofs, (hipStream_t)stream);
} HM_API_CATCH("hm_shplonk_set_quotient_batch_bn256_fr_dev")

int hm_lookup_permute_bn256_fr_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input,
                                   void* d_permuted_table, void* stream) try {
  if (rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table))
    return hm_fail(HM_ERR_BAD_ARG, "hm_lookup_permute_bn256_fr_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_LOOKUP_PERMUTE, 1, rows);
  return lookup_permute_run(*ctx, &d_input, &d_table, 1, rows, &d_permuted_input, &d_permuted_table, nullptr, (hipStream_t)stream);
} HM_API_CATCH("hm_lookup_permute_bn256_fr_dev")

int hm_lookup_permute_batch_bn256_fr_dev(const void* const* d_inputs, const void* const* d_tables, size_t count, size_t rows,
                                         void* const* d_permuted_inputs, void* const* d_permuted_tables, int* missing, void* stream) try {
  if (count && (!d_inputs || !d_tables || !d_permuted_inputs || !d_permuted_tables))
    return hm_fail(HM_ERR_BAD_ARG, "hm_lookup_permute_batch_bn256_fr_dev: null argument");
  if (rows)
    for (size_t p = 0; p < count; ++p)
      if (!d_inputs[p] || !d_tables[p] || !d_permuted_inputs[p] || !d_permuted_tables[p])
        return hm_fail(HM_ERR_BAD_ARG, "hm_lookup_permute_batch_bn256_fr_dev: null column");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  count_vector(*ctx, HM_STAT_LOOKUP_PERMUTE, count, (uint64_t)count * rows);
  return lookup_permute_run(*ctx, d_inputs, d_tables, count, rows, d_permuted_inputs, d_permuted_tables, missing, (hipStream_t)stream);
} HM_API_CATCH("hm_lookup_permute_batch_bn256_fr_dev")

int hm_logup_multiplicities_bn256_fr_dev(const void* const* d_tables, const void* const* d_inputs, const uint32_t* input_counts, size_t count,
                                         size_t rows, void* const* d_m, int* missing, void* stream) try {
  const std::string who = "hm_logup_multiplicities_bn256_fr_dev: ";
  if (count == 0) return HM_OK;
  if (!d_tables || !d_inputs || !input_counts || !d_m) return hm_fail(HM_ERR_BAD_ARG, who + "null argument");
  if (rows == 0 || rows >= ((size_t)1 << 31)) return hm_fail(HM_ERR_BAD_ARG, who + "need 1 <= rows < 2^31");
  const size_t bytes = rows * 32;
  size_t total = 0;
  for (size_t a = 0; a < count; ++a) {
    if (input_counts[a] == 0) return hm_fail(HM_ERR_BAD_ARG, who + "an argument without an input column");
    if ((uint64_t)input_counts[a] * rows >= ((uint64_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, who + "need c * rows < 2^32 (the counters are 32-bit)");
    total += input_counts[a];
  }
  auto usable = [](const void* p) { return p && ((uintptr_t)p & 15) == 0; };
  for (size_t a = 0; a < count; ++a)
    if (!usable(d_tables[a]) || !usable(d_m[a])) return hm_fail(HM_ERR_BAD_ARG, who + "a null or misaligned column");
  for (size_t j = 0; j < total; ++j)
    if (!usable(d_inputs[j])) return hm_fail(HM_ERR_BAD_ARG, who + "a null or misaligned input column");
  for (size_t a = 0; a < count; ++a) {
    for (size_t b = 0; b < count; ++b)
      if (ranges_overlap(d_m[a], bytes, d_tables[b], bytes) || (a != b && ranges_overlap(d_m[a], bytes, d_m[b], bytes)))
        return hm_fail(HM_ERR_BAD_ARG, who + "an output overlaps another column of the call");
    for (size_t j = 0; j < total; ++j)
      if (ranges_overlap(d_m[a], bytes, d_inputs[j], bytes)) return hm_fail(HM_ERR_BAD_ARG, who + "an output overlaps an input column");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return logup_multiplicities_run(d_tables, d_inputs, input_counts, count, rows, d_m, missing, (hipStream_t)stream);
} HM_API_CATCH("hm_logup_multiplicities_bn256_fr_dev")

int hm_fr_grand_sum_batch_dev(const void* const* d_terms, size_t n, void* const* d_out, size_t count, void* stream) try {
  const std::string who = "hm_fr_grand_sum_batch_dev: ";
  if (count == 0) return HM_OK;
  if (!d_terms || !d_out) return hm_fail(HM_ERR_BAD_ARG, who + "null argument");
  if (n == 0 || n >= ((size_t)1 << 32)) return hm_fail(HM_ERR_BAD_ARG, who + "need 1 <= n < 2^32");
  if (count > 65535) return hm_fail(HM_ERR_BAD_ARG, who + "at most 65535 columns per call");
  for (size_t j = 0; j < count; ++j)
    if (!d_terms[j] || !d_out[j] || (((uintptr_t)d_terms[j] | (uintptr_t)d_out[j]) & 15)) return hm_fail(HM_ERR_BAD_ARG, who + "a null or misaligned column");
  for (size_t j = 0; j < count; ++j) {
    for (size_t i = 0; i < count; ++i)
      if (i != j && (ranges_overlap(d_out[j], n * 32, d_terms[i], n * 32) || ranges_overlap(d_out[j], n * 32, d_out[i], n * 32)))
        return hm_fail(HM_ERR_BAD_ARG, who + "an output overlaps another column of the call");
    if (d_out[j] != d_terms[j] && ranges_overlap(d_out[j], n * 32, d_terms[j], n * 32))
      return hm_fail(HM_ERR_BAD_ARG, who + "an output partially overlaps its terms");
  }
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_grand_sum_batch_run(d_terms, n, d_out, count, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_grand_sum_batch_dev")

int hm_fr_mul_periodic_dev(void* d_a, size_t n, const uint64_t* pattern, uint32_t period, void* stream) try {
  if ((n && !d_a) || !pattern) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_mul_periodic_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_mul_periodic_run((uint32_t*)d_a, n, pattern, period, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_mul_periodic_dev")

int hm_fr_powers_dev(void* d_out, size_t n, const uint64_t x[4], void* stream) try {
  if ((n && !d_out) || !x) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_powers_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_powers_run((uint32_t*)d_out, n, x, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_powers_dev")

int hm_graph_create(const uint32_t* calcs, size_t n_calc, const uint64_t* constants, size_t n_const, size_t n_dynamic,
                    const int32_t* rotations, size_t n_rot, size_t n_columns, uint32_t n_intermediates, uint64_t* out_handle) try {
  if (!out_handle || (n_calc && !calcs) || (n_const && !constants) || (n_rot && !rotations))
    return hm_fail(HM_ERR_BAD_ARG, "hm_graph_create: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return graph_create(*ctx, calcs, n_calc, constants, n_const, n_dynamic, rotations, n_rot, n_columns, n_intermediates, out_handle);
} HM_API_CATCH("hm_graph_create")

// every hm_graph_evaluate*_dev: null arguments, the context and its lock, the program, the call counter, graph_run
static int graph_entry(const char* who, uint64_t handle, const GraphCall& c, void* stream) {
  if (!c.d_values || (c.n_columns && (!c.bases || (c.kind != GRAPH_SINGLE && !c.strides))) || (c.n_dyn && !c.dyn_ext))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (auto& g : ctx->graphs)
    if (g->handle == handle) {
      const bool countable = c.kind == GRAPH_SINGLE ? c.log_size < 40 : c.log_size < 32 && c.units < (1ull << 32);
      count_vector(*ctx, HM_STAT_GRAPH_EVALUATE, 1, countable ? ((uint64_t)c.segments << c.log_size) * c.units : 0);
      return graph_run(*ctx, *g, c, (hipStream_t)stream);
    }
  return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown program handle");
}

int hm_graph_evaluate_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                          size_t n_dynamic, uint32_t log_size, void* d_values, void* stream) try {
  return graph_entry("hm_graph_evaluate_dev", handle,
                     {GRAPH_SINGLE, n_columns, 1, n_dynamic, log_size, 1, 0, d_values, 0, d_columns, nullptr, dynamic_constants}, stream);
} HM_API_CATCH("hm_graph_evaluate_dev")

int hm_graph_evaluate_flags_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                                size_t n_dynamic, uint32_t log_size, void* d_values, uint32_t flags, void* stream) try {
  return graph_entry("hm_graph_evaluate_flags_dev", handle,
                     {GRAPH_SINGLE, n_columns, 1, n_dynamic, log_size, 1, flags, d_values, 0, d_columns, nullptr, dynamic_constants}, stream);
} HM_API_CATCH("hm_graph_evaluate_flags_dev")

int hm_graph_evaluate_segments_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                                   size_t n_dynamic, uint32_t log_segment, uint32_t segments, void* d_values, uint32_t flags, void* stream) try {
  return graph_entry("hm_graph_evaluate_segments_dev", handle,
                     {GRAPH_SINGLE, n_columns, 1, n_dynamic, log_segment, segments, flags, d_values, 0, d_columns, nullptr, dynamic_constants}, stream);
} HM_API_CATCH("hm_graph_evaluate_segments_dev")

int hm_graph_evaluate_circuits_dev(uint64_t handle, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                                   size_t circuits, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_size, uint32_t segments,
                                   void* d_values, uint32_t flags, void* stream) try {
  return graph_entry("hm_graph_evaluate_circuits_dev", handle,
                     {GRAPH_CIRCUITS, n_columns, circuits, n_dynamic, log_size, segments, flags, d_values, 0, column_bases, column_strides, dynamic_constants},
                     stream);
} HM_API_CATCH("hm_graph_evaluate_circuits_dev")

int hm_graph_evaluate_proofs_dev(uint64_t handle, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                                 size_t proofs, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_size, uint32_t segments,
                                 void* d_values, uint64_t values_stride, uint32_t flags, void* stream) try {
  return graph_entry("hm_graph_evaluate_proofs_dev", handle,
                     {GRAPH_PROOFS, n_columns, proofs, n_dynamic, log_size, segments, flags, d_values, values_stride, column_bases, column_strides,
                      dynamic_constants},
                     stream);
} HM_API_CATCH("hm_graph_evaluate_proofs_dev")

// ---------------------------------------------------------------------------------------------
// The quotient h(X) of a proof in ONE call, from coefficient arrays: every column onto `count` cosets of the n-th roots
// (hm_coeff_to_cosets), the numerator program over count segments of n rows (hm_graph_evaluate_segments), the inverse
// transforms (hm_cosets_to_coeff), and the recombination with the vanishing division on its matrix -- what upstream's
// evaluate_h + divide_by_vanishing_poly + extended_to_coeff make of the extended arrays.
// ---------------------------------------------------------------------------------------------
// host side of the recombination: u_c = shift_c^n, V^-1 (Gauss-Jordan) with 1 / (u_c - 1) on column c -> rows of 4 * count words
static int quotient_matrix(const char* who, const uint64_t* shifts, size_t count, uint32_t log_n, std::vector<std::vector<uint64_t>>* rows) {
  std::vector<host::Fr4> u(count);
  for (size_t c = 0; c < count; ++c) {
    host::Fr4 x = host::fr_load(shifts + 4 * c);
    if (host::fr_is_zero(x)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a coset shift is zero");
    for (uint32_t b = 0; b < log_n; ++b) x = host::fr_mul(x, x);
    u[c] = x;
    if (host::fr_eq(u[c], host::FR_ONE)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a coset lies in the n-th roots (X^n - 1 vanishes on it)");
    for (size_t b = 0; b < c; ++b)
      if (host::fr_eq(u[b], u[c])) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": two shifts name the same coset");
  }
  const host::Fr4 zero = {{0, 0, 0, 0}};
  std::vector<std::vector<host::Fr4>> m(count, std::vector<host::Fr4>(2 * count, zero));      // [V | I] -> [I | V^-1]
  for (size_t a = 0; a < count; ++a) {
    host::Fr4 p = host::FR_ONE;
    for (size_t t = 0; t < count; ++t) { m[a][t] = p; p = host::fr_mul(p, u[a]); }
    m[a][count + a] = host::FR_ONE;
  }
  for (size_t col = 0; col < count; ++col) {
    size_t piv = col;
    while (piv < count && host::fr_is_zero(m[piv][col])) ++piv;
    if (piv == count) return hm_fail(HM_ERR_INTERNAL, std::string(who) + ": singular coset matrix");
    std::swap(m[col], m[piv]);
    const host::Fr4 inv = host::fr_inv(m[col][col]);
    for (auto& v : m[col]) v = host::fr_mul(v, inv);
    for (size_t row = 0; row < count; ++row) {
      if (row == col || host::fr_is_zero(m[row][col])) continue;
      const host::Fr4 f = m[row][col];
      for (size_t c2 = 0; c2 < 2 * count; ++c2) m[row][c2] = host::fr_sub(m[row][c2], host::fr_mul(f, m[col][c2]));
    }
  }
  rows->assign(count, std::vector<uint64_t>(4 * count));
  for (size_t c = 0; c < count; ++c) {
    const host::Fr4 tinv = host::fr_inv(host::fr_sub(u[c], host::FR_ONE));
    for (size_t t = 0; t < count; ++t) {
      const host::Fr4 v = host::fr_mul(m[t][count + c], tinv);
      std::memcpy(&(*rows)[t][4 * c], v.l, 32);
    }
  }
  return HM_OK;
}

// steps 1 - 3 on this device: the columns onto `count` cosets, the numerator over count segments, the inverse transforms ->
// d_partials (count x n).  ctx.mu held.
static int quotient_partials(const char* who, DeviceCtx& ctx, uint64_t program, const void* const* d_coeff_columns, const void* const* d_on_cosets,
                             size_t n_columns, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_n, const uint64_t omega[4],
                             const uint64_t* shifts, size_t count, void* d_partials, hipStream_t st) {
  std::vector<size_t> todo;
  for (size_t i = 0; i < n_columns; ++i) {
    if (d_on_cosets && d_on_cosets[i]) continue;
    if (!d_coeff_columns || !d_coeff_columns[i]) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a column has neither coefficients nor coset values");
    todo.push_back(i);
  }
  const uint64_t n = 1ull << log_n;
  std::vector<host::Fr4> shift_inv(count);
  for (size_t c = 0; c < count; ++c) {
    const host::Fr4 x = host::fr_load(shifts + 4 * c);
    if (host::fr_is_zero(x)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a coset shift is zero");
    shift_inv[c] = host::fr_inv(x);
  }
  const host::Fr4 zero = {{0, 0, 0, 0}};
  host::Fr4 nn = host::FR_ONE;                                               // n = 2^log_n in Montgomery form: 1 doubled log_n times
  for (uint32_t b = 0; b < log_n; ++b) nn = host::fr_sub(nn, host::fr_sub(zero, nn));
  const host::Fr4 n_inv = host::fr_inv(nn);
  const host::Fr4 om_inv = host::fr_inv(host::fr_load(omega));
  GraphProgram* g = nullptr;
  for (auto& gp : ctx.graphs)
    if (gp->handle == program) g = gp.get();
  if (!g) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": unknown program handle");
  if (n_columns != g->n_columns) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": the program was built for another number of columns");
  const size_t row = (size_t)n * 32;
  const size_t T = todo.size();
  std::vector<const void*> cols(n_columns);
  // The transforms and the numerator below take the stream's slot again (aux_scope nests on one stream) and use its other buffers.
  return aux_scope(ctx, st, [&](AuxSlot& slot) -> int {
    // work: [the columns to transform, side by side: T x n] [those columns on the cosets: T x count x n]
    uint8_t* work = (uint8_t*)aux_buffer(slot, AuxBuf::work, row * (T + T * count) + 32, who);
    if (!work) return HM_ERR_HIP;
    uint8_t* contig = work;
    uint8_t* on_cosets = contig + row * T;
    int rc = HM_OK;
    if (T) {
      for (size_t j = 0; j < T; ++j)
        HM_HIP_CHECK(hipMemcpyAsync(contig + row * j, d_coeff_columns[todo[j]], row, hipMemcpyDeviceToDevice, st));
      NttCall onto = ntt_call(log_n, T, NTT_F_IN_TABLES);
      onto.fwd_cosets = (uint32_t)count;
      NttPointers p = ntt_pointers(on_cosets, omega);
      p.d_in = (const uint32_t*)contig, p.shifts = shifts, p.internal = true;
      rc = ntt_run(ctx, onto, p, st);
      if (rc != HM_OK) return rc;
      count_ntt(ctx, log_n, T * count);
    }
    for (size_t i = 0; i < n_columns; ++i) cols[i] = d_on_cosets ? d_on_cosets[i] : nullptr;
    for (size_t j = 0; j < T; ++j) cols[todo[j]] = on_cosets + row * count * j;
    HM_HIP_CHECK(hipMemsetAsync(d_partials, 0, row * count, st));                // PreviousValue: upstream starts h at zero
    rc = graph_run(ctx, *g, {GRAPH_SINGLE, n_columns, 1, n_dynamic, log_n, (uint32_t)count, HM_GRAPH_COLUMNS_INTERNAL, d_partials, 0, cols.data(), nullptr,
                             dynamic_constants}, st);
    if (rc != HM_OK) return rc;
    count_vector(ctx, HM_STAT_GRAPH_EVALUATE, 1, (uint64_t)count << log_n);
    NttCall back = ntt_call(log_n, 1, NTT_F_SCALE | NTT_F_OUT_TABLES);
    back.inv_cosets = (uint32_t)count;
    NttPointers q = ntt_pointers(d_partials, om_inv.l, n_inv.l);
    q.shifts = shift_inv[0].l;
    rc = ntt_run(ctx, back, q, st);
    if (rc == HM_OK) count_ntt(ctx, log_n, count);
    return rc;
  });
}

static int quotient_check_args(const char* who, const void* out, const uint64_t* omega, const uint64_t* shifts, size_t n_columns,
                               const void* const* d_coeff_columns, const void* const* d_on_cosets, size_t n_dynamic,
                               const uint64_t* dynamic_constants, uint32_t log_n, size_t count) {
  if (!out || !omega || !shifts || (n_columns && !d_coeff_columns && !d_on_cosets) || (n_dynamic && !dynamic_constants))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (log_n > 28 || log_n == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": log_n must be in 1 .. 28");
  if (count == 0 || count > 16) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": 1 .. 16 cosets per call");
  if (n_columns == 0 || n_columns * count > 65535) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": columns x cosets must be in 1 .. 65535");
  return HM_OK;
}

int hm_quotient_partials_bn256_fr_dev(uint64_t program, const void* const* d_coeff_columns, const void* const* d_on_cosets, size_t n_columns,
                                      const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_n, const uint64_t omega[4],
                                      const uint64_t* shifts, size_t count, void* d_partials, void* stream) try {
  const char* who = "hm_quotient_partials_bn256_fr_dev";
  const int arc = quotient_check_args(who, d_partials, omega, shifts, n_columns, d_coeff_columns, d_on_cosets, n_dynamic, dynamic_constants, log_n, count);
  if (arc != HM_OK) return arc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return quotient_partials(who, *ctx, program, d_coeff_columns, d_on_cosets, n_columns, dynamic_constants, n_dynamic, log_n, omega, shifts, count,
                           d_partials, (hipStream_t)stream);
} HM_API_CATCH("hm_quotient_partials_bn256_fr_dev")

int hm_quotient_combine_bn256_fr_dev(const void* const* d_partials, const uint64_t* shifts, size_t count, uint32_t log_n, size_t pieces, void* d_h,
                                     void* stream) try {
  const char* who = "hm_quotient_combine_bn256_fr_dev";
  if (!d_partials || !shifts || !d_h) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (log_n > 28 || log_n == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": log_n must be in 1 .. 28");
  if (count == 0 || count > 64 || pieces == 0 || pieces > count) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": 1 <= pieces <= cosets <= 64");
  for (size_t c = 0; c < count; ++c) {
    if (!d_partials[c]) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null partial");
    // piece t is written before piece t + 1 reads EVERY partial again: h must not share memory with any of them
    if (ranges_overlap(d_h, ((size_t)32 << log_n) * pieces, d_partials[c], (size_t)32 << log_n))
      return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_h overlaps a partial (recombining in place is not supported)");
  }
  std::vector<std::vector<uint64_t>> rows;
  const int mrc = quotient_matrix(who, shifts, count, log_n, &rows);
  if (mrc != HM_OK) return mrc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const uint64_t n = 1ull << log_n;
  for (size_t t = 0; t < pieces; ++t) {
    const int rc = fr_linear_combination_run(d_partials, rows[t].data(), count, n, (uint32_t*)((uint8_t*)d_h + (size_t)n * 32 * t), (hipStream_t)stream);
    if (rc != HM_OK) return rc;
  }
  count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, pieces, (uint64_t)pieces * count * n);
  return HM_OK;
} HM_API_CATCH("hm_quotient_combine_bn256_fr_dev")

int hm_quotient_by_cosets_bn256_fr_dev(uint64_t program, const void* const* d_coeff_columns, const void* const* d_on_cosets, size_t n_columns,
                                       const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_n, const uint64_t omega[4],
                                       const uint64_t* shifts, size_t count, size_t pieces, void* d_h, void* stream) try {
  const char* who = "hm_quotient_by_cosets_bn256_fr_dev";
  const int arc = quotient_check_args(who, d_h, omega, shifts, n_columns, d_coeff_columns, d_on_cosets, n_dynamic, dynamic_constants, log_n, count);
  if (arc != HM_OK) return arc;
  if (pieces == 0 || pieces > count) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": 1 <= pieces <= cosets <= 16");
  std::vector<std::vector<uint64_t>> rows;
  const int mrc = quotient_matrix(who, shifts, count, log_n, &rows);
  if (mrc != HM_OK) return mrc;
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n = 1ull << log_n;
  const size_t row = (size_t)n * 32;
  std::vector<const void*> parts(count);
  // the partials live in the stream's NTT scratch slot? no: that is the transforms' ping-pong buffer.  They get the tail of a
  // buffer of their own (AuxSlot::table is the scans' scratch: free between calls on this stream)
  return aux_scope(*ctx, st, [&](AuxSlot& slot) -> int {
    uint8_t* parts_buf = (uint8_t*)aux_buffer(slot, AuxBuf::table, row * count, who);
    if (!parts_buf) return HM_ERR_HIP;
    int rc = quotient_partials(who, *ctx, program, d_coeff_columns, d_on_cosets, n_columns, dynamic_constants, n_dynamic, log_n, omega, shifts, count,
                               parts_buf, st);
    if (rc != HM_OK) return rc;
    for (size_t c = 0; c < count; ++c) parts[c] = parts_buf + row * c;
    for (size_t t = 0; t < pieces; ++t) {
      rc = fr_linear_combination_run(parts.data(), rows[t].data(), count, n, (uint32_t*)((uint8_t*)d_h + row * t), st);
      if (rc != HM_OK) return rc;
    }
    count_vector(*ctx, HM_STAT_LINEAR_COMBINATION, pieces, (uint64_t)pieces * count * n);
    return HM_OK;
  });
} HM_API_CATCH("hm_quotient_by_cosets_bn256_fr_dev")

int hm_graph_destroy(uint64_t handle) try {
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (size_t i = 0; i < ctx->graphs.size(); ++i)
    if (ctx->graphs[i]->handle == handle) {
      (void)hipDeviceSynchronize();          // a launch may still read the program (rare call: once per circuit)
      graph_release(*ctx->graphs[i]);
      ctx->graphs.erase(ctx->graphs.begin() + i);
      return HM_OK;
    }
  return hm_fail(HM_ERR_NOT_FOUND, "hm_graph_destroy: unknown program handle");
} HM_API_CATCH("hm_graph_destroy")

int hm_fr_dot_bn256_dev(const void* d_a, const void* d_b, size_t n, uint64_t out[4], void* stream) try {
  if (!out || (n && (!d_a || !d_b))) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_dot_bn256_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return fr_dot_run(*ctx, (const uint32_t*)d_a, (const uint32_t*)d_b, n, out, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_dot_bn256_dev")

int hm_fr_affine_sequence_dev(void* d_out, size_t n, const uint64_t a[4], const uint64_t b[4], void* stream) try {
  if ((n && !d_out) || !a || !b) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_affine_sequence_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_affine_sequence_run((uint32_t*)d_out, n, a, b, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_affine_sequence_dev")

int hm_fr_random_dev(void* d_out, size_t n, uint64_t seed, void* stream) try {
  if (n && !d_out) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_random_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return fr_random_run((uint32_t*)d_out, n, seed, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_random_dev")

int hm_fr_scale_dev(void* d_a, size_t n, const uint64_t c[4], void* stream) try {
  if ((n && !d_a) || !c) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_scale_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (n == 0) return HM_OK;
  return fr_scale_run((uint32_t*)d_a, c, n, (hipStream_t)stream);     // the constant travels by value: no shared state
} HM_API_CATCH("hm_fr_scale_dev")

int hm_fr_distribute_powers_dev(void* d_a, size_t n, const uint64_t c3[12], void* stream) try {
  if ((n && !d_a) || !c3) return hm_fail(HM_ERR_BAD_ARG, "hm_fr_distribute_powers_dev: null argument");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  if (n == 0) return HM_OK;
  return fr_mul_pattern3_run((uint32_t*)d_a, c3, n, (hipStream_t)stream);
} HM_API_CATCH("hm_fr_distribute_powers_dev")

}  // extern "C"
