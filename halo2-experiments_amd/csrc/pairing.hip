// pairing.hip -- batched pairing product checks on BN256: the two kernels, pairing_work_words and
// pairing_check_run.  The tower, the Miller lane and the final exponentiation are in pairing.inc, which host_check.cpp compiles too.
#include <hip/hip_runtime.h>

#include "g1.h"
#include "hm_internal.h"

namespace hm {

#include "pairing.inc"

constexpr int PF_THREADS = 64;

__global__ __launch_bounds__(PF_THREADS) void pairing_miller_kernel(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                                    uint64_t n_pairs, uint32_t* __restrict__ slots,
                                                                    uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * PF_THREADS + threadIdx.x;
  if (i >= n_pairs) return;
  uint32_t p[16], q[32];
  {
    const uint4* s = reinterpret_cast<const uint4*>(g1 + i * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 v = s[k];
      p[4 * k] = v.x, p[4 * k + 1] = v.y, p[4 * k + 2] = v.z, p[4 * k + 3] = v.w;
    }
    const uint4* t = reinterpret_cast<const uint4*>(g2 + i * 32);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = t[k];
      q[4 * k] = v.x, q[4 * k + 1] = v.y, q[4 * k + 2] = v.z, q[4 * k + 3] = v.w;
    }
  }
  flags[i] = pf_miller_lane(p, q, PfLane{slots + i, (size_t)n_pairs});
}

__global__ __launch_bounds__(PF_THREADS) void pairing_finish_kernel(const uint32_t* __restrict__ offsets, uint64_t n_pairs, uint64_t n_checks,
                                                                    uint32_t* __restrict__ pair_slots, const uint32_t* __restrict__ flags,
                                                                    uint32_t* __restrict__ check_slots, uint32_t* __restrict__ gt,
                                                                    uint32_t* __restrict__ status) {
  const uint64_t c = (uint64_t)blockIdx.x * PF_THREADS + threadIdx.x;
  if (c >= n_checks) return;
  status[c] = pf_finish_lane(offsets[c], offsets[c + 1], n_pairs, PfLane{pair_slots, (size_t)n_pairs}, flags,
                             PfLane{check_slots + c, (size_t)n_checks}, gt ? gt + c * PF_WORDS : nullptr);
}

// words of the workspace: the pairs' slots, their flags, the checks' slots
size_t pairing_work_words(size_t n_pairs, size_t n_checks) {
  return (size_t)PF_PAIR_SLOTS * PF_WORDS * n_pairs + n_pairs + (size_t)PF_CHECK_SLOTS * PF_WORDS * n_checks;
}

int pairing_check_run(const uint32_t* d_g1, const uint32_t* d_g2, size_t n_pairs, const uint32_t* d_offsets, size_t n_checks, uint32_t* d_gt,
                      uint32_t* d_status, uint32_t* d_work, hipStream_t stream) {
  uint32_t* pair_slots = d_work;
  uint32_t* flags = pair_slots + (size_t)PF_PAIR_SLOTS * PF_WORDS * n_pairs;
  uint32_t* check_slots = flags + n_pairs;
  if (n_pairs) {
    pairing_miller_kernel<<<(unsigned)((n_pairs + PF_THREADS - 1) / PF_THREADS), PF_THREADS, 0, stream>>>(d_g1, d_g2, n_pairs, pair_slots, flags);
    HM_HIP_CHECK(hipGetLastError());
  }
  pairing_finish_kernel<<<(unsigned)((n_checks + PF_THREADS - 1) / PF_THREADS), PF_THREADS, 0, stream>>>(d_offsets, n_pairs, n_checks, pair_slots,
                                                                                                       flags, check_slots, d_gt, d_status);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

}  // namespace hm
