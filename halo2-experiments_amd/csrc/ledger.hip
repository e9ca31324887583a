// ledger.hip -- the device side of verify_ledger_users (ledger.py): the kernel and the driver
//   kzg_ledger_pairs_run      every user's pair (pi, -R) of its ledger opening check, one lane per user (ledger.inc)
// The per-lane functions stand in ledger.inc: host_check.cpp compiles them too.
#include <hip/hip_runtime.h>

#include <string>

#include "fq_inverse.h"
#include "g1_mul.h"
#include "hm_internal.h"

namespace hm {

#include "g1_codec.inc"      // g1_check_one
#include "verify_sums.inc"   // vs_load_base, vs_store_acc, vs_finish
#include "ledger.inc"

constexpr int LD_THREADS = 64;             // one wavefront per workgroup: a lane is a user, and no lane talks to another

__global__ __launch_bounds__(LD_THREADS) void kzg_ledger_pairs_kernel(LdShared s, const uint32_t* __restrict__ openings,
                                                                     const uint32_t* __restrict__ indices, const uint32_t* __restrict__ ids,
                                                                     const uint32_t* __restrict__ balances, uint64_t users,
                                                                     uint32_t* __restrict__ rows, uint32_t* __restrict__ flags) {
  const uint64_t b = (uint64_t)blockIdx.x * LD_THREADS + threadIdx.x;
  if (b >= users) return;
  flags[b] = ld_pair(s, openings + b * 16, indices[b], ids + b * 8, balances + b * s.assets * 8, rows + b * 2 * VS_ROW_WORDS);
}

static bool words_below(const uint64_t* w, const uint32_t (&mod32)[8]) {
  for (int j = 3; j >= 0; --j) {
    const uint64_t m = ((uint64_t)mod32[2 * j + 1] << 32) | mod32[2 * j];
    if (w[j] != m) return w[j] < m;
  }
  return false;
}

// what is wrong with the three host word arrays of a call, or null: read by the entry point before it asks for a device
const char* kzg_ledger_words_problem(const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8]) {
  if (!words_below(gamma, FrParams::MOD32) || !words_below(omega, FrParams::MOD32)) return "gamma or omega is not below r";
  if (!words_below(c_gamma, FqParams::MOD32) || !words_below(c_gamma + 4, FqParams::MOD32)) return "a coordinate of c_gamma is not below p";
  return nullptr;
}

// the arguments were checked by the caller (capi_g1.hip): one launch, asynchronous on `stream`
int kzg_ledger_pairs_run(const uint32_t* d_openings, const uint32_t* d_indices, const uint32_t* d_ids, const uint32_t* d_balances,
                         const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8], uint32_t log_n, uint32_t assets,
                         size_t users, uint32_t* d_g1, uint32_t* d_flags, hipStream_t stream) {
  LdShared s;
  for (int j = 0; j < 4; ++j) {
    s.gamma[2 * j] = (uint32_t)gamma[j], s.gamma[2 * j + 1] = (uint32_t)(gamma[j] >> 32);
    s.omega[2 * j] = (uint32_t)omega[j], s.omega[2 * j + 1] = (uint32_t)(omega[j] >> 32);
  }
  for (int j = 0; j < 8; ++j) s.c_gamma[2 * j] = (uint32_t)c_gamma[j], s.c_gamma[2 * j + 1] = (uint32_t)(c_gamma[j] >> 32);
  s.k = log_n;
  s.assets = assets;
  const uint32_t blocks = (uint32_t)((users + LD_THREADS - 1) / LD_THREADS);
  hipLaunchKernelGGL(kzg_ledger_pairs_kernel, dim3(blocks), dim3(LD_THREADS), 0, stream, s, d_openings, d_indices, d_ids, d_balances,
                     (uint64_t)users, d_g1, d_flags);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

}  // namespace hm
