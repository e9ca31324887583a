// keygen.hip -- keygen's permutation assembly on the device: the kernels of the union, the keys and the links,
// and perm_assemble_run.  The plan, the key packing and the link rule are in keygen.inc, which host_check.cpp compiles too; the sort
// is the Merkle update's network (poseidon.hip: merkle_update_sort).
#include <hip/hip_runtime.h>

#include <string>

#include "ff29.h"
#include "hm_internal.h"

namespace hm {

#include "keygen.inc"

constexpr int PS_THREADS = 256;      // lanes per workgroup, as in poseidon.hip, whose sort runs between these kernels

__global__ __launch_bounds__(PS_THREADS) void perm_identity_kernel(uint32_t* __restrict__ cells_out, uint64_t cells) {
  const uint64_t c = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (c < cells) cells_out[c] = (uint32_t)c;
}

// The parent words are read and written by lanes of every XCD while the kernel runs: device-scope accesses throughout.  A stale
// word is still an ancestor (pointers only go down), and a hook is decided by the compare-and-swap alone.
__device__ __forceinline__ uint32_t perm_parent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t perm_find_halving(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = perm_parent(parent, x);
    if (p == x) return x;
    const uint32_t g = perm_parent(parent, p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

__global__ __launch_bounds__(PS_THREADS) void perm_union_kernel(const uint2* __restrict__ copies, uint64_t m, uint64_t cells,
                                                                uint32_t* parent) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= m) return;
  const uint2 pair = copies[t];
  if (pair.x >= cells || pair.y >= cells) return;
  uint32_t a = perm_find_halving(parent, pair.x), b = perm_find_halving(parent, pair.y);
  while (a != b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) break;
    a = perm_find_halving(parent, seen);        // hi was hooked meanwhile: go on from where it points
    b = perm_find_halving(parent, lo);
  }
}

// after the union has finished: plain reads, nothing is written to the forest
__global__ __launch_bounds__(PS_THREADS) void perm_keys_kernel(const uint32_t* __restrict__ copies, uint64_t m, uint64_t n_pow2,
                                                               uint64_t cells, const uint32_t* __restrict__ parent,
                                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ dropped) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= n_pow2) return;
  uint64_t key = PERM_PAD;
  if (t < 2 * m) {
    const uint32_t cell = copies[t], other = copies[t ^ 1];
    if (cell < cells && other < cells) {
      uint32_t r = cell;
      for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
      key = perm_key(r, cell);
    } else if (dropped && !(t & 1)) {
      atomicAdd(dropped, 1u);
    }
  }
  keys[t] = key;
}

__global__ __launch_bounds__(PS_THREADS) void perm_link_kernel(const uint64_t* __restrict__ keys, uint64_t entries, uint64_t n_pow2,
                                                               uint32_t* __restrict__ sigma_cells) {
  const uint64_t p = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (p >= entries) return;
  uint32_t cell, target;
  if (perm_link(keys[p], p + 1 < n_pow2 ? keys[p + 1] : PERM_PAD, cell, target)) sigma_cells[cell] = target;
}

static int perm_assemble_launch(const uint32_t* d_copies, uint64_t m, uint64_t cells, uint32_t* d_sigma_cells, uint32_t* d_dropped,
                                uint64_t* d_keys, uint64_t n_pow2, hipStream_t stream) {
  const auto blocks = [](uint64_t lanes) { return dim3((unsigned)((lanes + PS_THREADS - 1) / PS_THREADS)); };
  hipLaunchKernelGGL(perm_union_kernel, blocks(m), dim3(PS_THREADS), 0, stream, (const uint2*)d_copies, m, cells, d_sigma_cells);
  hipLaunchKernelGGL(perm_keys_kernel, blocks(n_pow2), dim3(PS_THREADS), 0, stream, d_copies, m, n_pow2, cells,
                     (const uint32_t*)d_sigma_cells, d_keys, d_dropped);
  if (int rc = merkle_update_sort(d_keys, n_pow2, stream)) return rc;
  hipLaunchKernelGGL(perm_link_kernel, blocks(2 * m), dim3(PS_THREADS), 0, stream, (const uint64_t*)d_keys, 2 * m, n_pow2, d_sigma_cells);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// A fixed chain of launches: identity, union, keys, the sort's stages, links.  Nothing comes back to the host; the keys are
// stream-ordered scratch, as merkle_update_run's.
int perm_assemble_run(const uint32_t* d_copies, size_t m, uint32_t columns, uint32_t k, uint32_t* d_sigma_cells, uint32_t* d_dropped,
                      hipStream_t stream) {
  const uint64_t cells = (uint64_t)columns << k;
  if (d_dropped) HM_HIP_CHECK(hipMemsetAsync(d_dropped, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(perm_identity_kernel, dim3((unsigned)((cells + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, stream,
                     d_sigma_cells, cells);
  HM_HIP_CHECK(hipGetLastError());
  if (m == 0) return HM_OK;
  uint64_t n_pow2 = 2;
  while (n_pow2 < 2 * (uint64_t)m) n_pow2 <<= 1;
  return stream_scratch("permutation_assemble", (size_t)n_pow2 * 8, stream, [&](uint8_t* keys) -> int {
    return perm_assemble_launch(d_copies, m, cells, d_sigma_cells, d_dropped, (uint64_t*)keys, n_pow2, stream);
  });
}

}  // namespace hm
