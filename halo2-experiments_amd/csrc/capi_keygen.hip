// capi_keygen.hip -- the keygen entry points of the C ABI: the permutation argument's sigma mapping assembled from copy constraints
// and its columns (keygen.inc, polyops.hip).
#include <hip/hip_runtime.h>

#include <string>

#include "hm_internal.h"

using namespace hm;

extern "C" {

// what both entries refuse before anything else: -> cells = columns * 2^k
static int perm_shape(const char* who, uint32_t columns, uint32_t k, uint64_t* cells) {
  if (columns == 0) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": columns must be at least 1");
  if (k > 32 || ((uint64_t)columns << k) > ((uint64_t)1 << 32))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": columns * 2^k > 2^32");
  *cells = (uint64_t)columns << k;
  return HM_OK;
}

int hm_permutation_assemble_dev(const uint32_t* d_copies, size_t m, uint32_t columns, uint32_t k, uint32_t* d_sigma_cells,
                                uint32_t* d_dropped_or_null, void* stream) try {
  const char* who = "hm_permutation_assemble_dev";
  uint64_t cells = 0;
  if (int rc = perm_shape(who, columns, k, &cells)) return rc;
  if (m > ((size_t)1 << 30)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": 2 m > 2^31");
  if (!d_sigma_cells || (m && !d_copies)) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (((uintptr_t)d_copies & 7u) || ((uintptr_t)d_sigma_cells & 3u) || ((uintptr_t)d_dropped_or_null & 3u))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a device pointer is not 4-byte aligned (d_copies: 8)");
  if (m && ranges_overlap(d_copies, m * 8, d_sigma_cells, (size_t)cells * 4))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_copies overlaps d_sigma_cells");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return perm_assemble_run(d_copies, m, columns, k, d_sigma_cells, d_dropped_or_null, (hipStream_t)stream);
} HM_API_CATCH("hm_permutation_assemble_dev")

int hm_permutation_columns_bn256_fr_dev(const uint32_t* d_sigma_cells, uint32_t columns, uint32_t k, const uint64_t omega[4],
                                        const uint64_t delta[4], void* d_out, void* stream) try {
  const char* who = "hm_permutation_columns_bn256_fr_dev";
  uint64_t cells = 0;
  if (int rc = perm_shape(who, columns, k, &cells)) return rc;
  if (!d_sigma_cells || !omega || !delta || !d_out) return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (((uintptr_t)d_sigma_cells & 3u) || ((uintptr_t)d_out & 15u))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a device pointer is not 16-byte aligned (d_sigma_cells: 4)");
  if (ranges_overlap(d_sigma_cells, (size_t)cells * 4, d_out, (size_t)cells * 32))
    return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": d_sigma_cells overlaps d_out");
  DeviceCtx* ctx = ctx_for_current_device();
  if (!ctx) return HM_ERR_NO_DEVICE;
  return perm_columns_run(d_sigma_cells, columns, k, omega, delta, (uint32_t*)d_out, (hipStream_t)stream);
} HM_API_CATCH("hm_permutation_columns_bn256_fr_dev")

}  // extern "C"
