// range.hip -- the witness of the OverflowCheckV2 range-check circuit on the device: the kernel and
// range_witness_run.  The lane function is in range.inc, which host_check.cpp compiles too.
#include <hip/hip_runtime.h>

#include "g1.h"
#include "hm_internal.h"

namespace hm {

#include "poseidon.inc"   // ps_get_words / ps_put_words
#include "range.inc"

constexpr int RANGE_THREADS = 256;

__global__ __launch_bounds__(RANGE_THREADS) void range_witness_kernel(const RangeArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * RANGE_THREADS + threadIdx.x;
  if (idx >= a.lanes) return;                              // lanes is a multiple of 2^log_n: with log_n >= 6 whole waves leave
  const bool over = range_witness_lane(a, idx);
  if (!a.over) return;
  if (a.log_n >= 6) {                                      // a wave lies inside one circuit: one add per wave that has any
    const uint64_t votes = __ballot(over);
    if (votes && (threadIdx.x & 63) == 0) atomicAdd(a.over + (idx >> a.log_n), (uint32_t)__popcll(votes));
  } else if (over) {
    atomicAdd(a.over + (idx >> a.log_n), 1u);
  }
}

// the arguments were checked by the caller (capi_hash.hip: range_witness_args)
int range_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_values,
                      uint32_t* d_advice, uint32_t* d_over, hipStream_t stream) {
  RangeArgs a;
  a.values = d_values;
  a.advice = d_advice;
  a.over = d_over;
  a.lanes = (uint64_t)m << log_n;
  a.max_bits = max_bits;
  a.acc_cols = acc_cols;
  a.log_n = log_n;
  a.rows = rows;
  if (d_over) HM_HIP_CHECK(hipMemsetAsync(d_over, 0, m * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(range_witness_kernel, dim3((uint32_t)((a.lanes + RANGE_THREADS - 1) / RANGE_THREADS)), dim3(RANGE_THREADS), 0, stream, a);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

}  // namespace hm
