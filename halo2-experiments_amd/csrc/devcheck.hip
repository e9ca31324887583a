// devcheck.hip -- libhm_devcheck.so: the op tables of unit_ops.h on the device, one lane per case (tests/test_unit_ops_gpu.py).
// Test-only: it includes the arithmetic headers and nothing else of the library, and is never linked into libhalo2_mi355x.so.
// This is the device compile of ff29.h / g1.h as the kernels see it (HM_PIN is the inline-asm pin here), op by op.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/halo2_mi355x.h"
#include "unit_ops.h"

using namespace hm;

namespace {

constexpr int kBlock = 64;   // one wave per block: every op is a long straight-line chain, occupancy does not matter here

template <class F>
__global__ __launch_bounds__(kBlock) void field_ops_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    unit::field_op<F>(op, in + i * unit::FIELD_IN_WORDS, out + i * unit::FIELD_OUT_WORDS);
}

__global__ __launch_bounds__(kBlock) void curve_ops_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    unit::curve_op(op, in + i * unit::CURVE_IN_WORDS, out + i * unit::CURVE_OUT_WORDS);
}

// d_in: n input records, d_out: n output records, both device memory and 16-byte aligned
int check_args(const void* d_in, const void* d_out, size_t n) {
  if (!d_in || !d_out) return HM_ERR_BAD_ARG;
  if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return HM_ERR_BAD_ARG;
  if (n > ((size_t)1 << 24)) return HM_ERR_BAD_ARG;
  return HM_OK;
}
unsigned grid_for(size_t n) {
  const size_t blocks = (n + kBlock - 1) / kBlock;
  return (unsigned)(blocks < 4096 ? blocks : 4096);   // grid-stride beyond
}

}  // namespace

extern "C" {

// field: 0 = Fq, 1 = Fr; op: unit::FieldOp.  Asynchronous on `stream`; the output records must be zeroed by the caller.
int dc_field_ops(int field, int op, const uint32_t* d_in, uint32_t* d_out, size_t n, void* stream) {
  if (field != 0 && field != 1) return HM_ERR_BAD_ARG;
  if (op < 0 || op >= unit::UF_OP_END || (op > unit::UF_TO_EXT && op < unit::UF_SUB_3_29)) return HM_ERR_BAD_ARG;
  if (int rc = check_args(d_in, d_out, n)) return rc;
  if (n == 0) return HM_OK;
  if (field == 0)
    field_ops_kernel<FqParams><<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(op, d_in, d_out, n);
  else
    field_ops_kernel<FrParams><<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(op, d_in, d_out, n);
  return hipGetLastError() == hipSuccess ? HM_OK : HM_ERR_HIP;
}

// op: unit::CurveOp
int dc_curve_ops(int op, const uint32_t* d_in, uint32_t* d_out, size_t n, void* stream) {
  if (op < 0 || op >= unit::UC_OP_END) return HM_ERR_BAD_ARG;
  if (int rc = check_args(d_in, d_out, n)) return rc;
  if (n == 0) return HM_OK;
  curve_ops_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(op, d_in, d_out, n);
  return hipGetLastError() == hipSuccess ? HM_OK : HM_ERR_HIP;
}

}  // extern "C"
