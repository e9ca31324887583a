// g1_codec.hip -- the SRS point encodings of ParamsKZG::read / write on the device: the kernels and the
// drivers g1_compress_run, g1_decompress_run and g1_check_run.  The formats and the per-point functions are in g1_codec.inc, which
// host_check.cpp compiles too.
#include <hip/hip_runtime.h>

#include <string>

#include "hm_internal.h"
#include "msm_dev.h"

namespace hm {

#include "g1_codec.inc"

__global__ __launch_bounds__(ACC_THREADS) void g1_compress_kernel(const uint32_t* __restrict__ xy, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(xy + i * 16);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const uint32_t wy[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  uint32_t v[8];
  g1_compress_one(wx, wy, v);
  uint4* o = reinterpret_cast<uint4*>(out + i * 8);
  o[0] = make_uint4(v[0], v[1], v[2], v[3]);
  o[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// invalid entries -> (0, 0) and atomicMin(first_bad, i)
__global__ __launch_bounds__(ACC_THREADS) void g1_decompress_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ xy, size_t n,
                                                                    unsigned long long* __restrict__ first_bad) {
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(in + i * 8);
  const uint4 a = q[0], b = q[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t ox[8], oy[8];
  if (!g1_decompress_one(w, ox, oy)) atomicMin(first_bad, (unsigned long long)i);
  uint4* o = reinterpret_cast<uint4*>(xy + i * 16);
  o[0] = make_uint4(ox[0], ox[1], ox[2], ox[3]);
  o[1] = make_uint4(ox[4], ox[5], ox[6], ox[7]);
  o[2] = make_uint4(oy[0], oy[1], oy[2], oy[3]);
  o[3] = make_uint4(oy[4], oy[5], oy[6], oy[7]);
}

__global__ __launch_bounds__(ACC_THREADS) void g1_check_kernel(const uint32_t* __restrict__ xy, size_t n,
                                                               unsigned long long* __restrict__ first_bad) {
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(xy + i * 16);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const uint32_t wy[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  if (!g1_check_one(wx, wy)) atomicMin(first_bad, (unsigned long long)i);
}

// SRS point encodings (g1_codec.inc).  Compression is asynchronous on `stream`.
int g1_compress_run(const uint32_t* d_xy, size_t n, uint32_t* d_out32, hipStream_t stream) {
  if (n == 0) return HM_OK;
  hipLaunchKernelGGL(g1_compress_kernel, dim3((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0, stream, d_xy,
                     d_out32, n);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// The validating kernels lower one device word (allocated per call, stream-ordered, all ones) to the smallest invalid index; this waits for
// `stream`, reads it back and answers HM_ERR_INVALID_DATA with *first_invalid set, or HM_OK with *first_invalid = n.
template <class Launch>
static int g1_codec_validating_run(const char* who, size_t n, uint64_t* first_invalid, hipStream_t stream, Launch launch) {
  *first_invalid = n;
  if (n == 0) return HM_OK;
  unsigned long long bad = ~0ull;
  int rc = stream_scratch(who, sizeof(bad), stream, [&](uint8_t* mem) -> int {
    unsigned long long* flag = (unsigned long long*)mem;
    int rc = HM_OK;
    const hipError_t me = hipMemsetAsync(flag, 0xff, sizeof(bad), stream);
    if (me != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": hipMemsetAsync: " + hipGetErrorString(me));
    if (rc == HM_OK) {
      launch(dim3((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS)), flag);
      if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": kernel launch failed");
    }
    if (rc == HM_OK) {
      const hipError_t ce = hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, stream);
      if (ce != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": reading the flag: " + hipGetErrorString(ce));
    }
    return rc;
  });
  const hipError_t se = hipStreamSynchronize(stream);
  if (rc == HM_OK && se != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(se));
  if (rc == HM_OK && bad < n) {
    *first_invalid = bad;
    rc = hm_fail(HM_ERR_INVALID_DATA, std::string(who) + ": invalid point at index " + std::to_string(bad));
  }
  return rc;
}

int g1_decompress_run(const uint32_t* d_in32, size_t n, uint32_t* d_xy, uint64_t* first_invalid, hipStream_t stream) {
  return g1_codec_validating_run("g1_decompress", n, first_invalid, stream, [&](dim3 grid, unsigned long long* flag) {
    hipLaunchKernelGGL(g1_decompress_kernel, grid, dim3(ACC_THREADS), 0, stream, d_in32, d_xy, n, flag);
  });
}

int g1_check_run(const uint32_t* d_xy, size_t n, uint64_t* first_invalid, hipStream_t stream) {
  return g1_codec_validating_run("g1_check", n, first_invalid, stream, [&](dim3 grid, unsigned long long* flag) {
    hipLaunchKernelGGL(g1_check_kernel, grid, dim3(ACC_THREADS), 0, stream, d_xy, n, flag);
  });
}

}  // namespace hm
