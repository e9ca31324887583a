// sorted.hip -- the sorted-column circuit's witness and the argsort that brings an id column into its order, on the device
// (DESIGN.md section 32): the kernels, sorted_witness_run and fr_argsort_run.  The lane function and the record order are in
// sorted.inc, which host_check.cpp compiles too.
//
// The argsort carries a 32-bit row with every 256-bit key (lookup.hip's sort is keys-only and stays as it is):
//   1  records   Montgomery words -> canonical integers (one product by 2^-256, range.inc: range_plain) beside their rows, padded to a
//                power of two with all-ones keys, which sort behind every field element
//   2  sort      bitonic network on (key, row): stages with a partner inside a tile of SRT_TILE records run in LDS, structure of
//                arrays; the others are one launch per stage
//   3  rows      the sorted rows of the first n records, widened to 64 bits
// No two records are equal (the row breaks ties), so the result is a function of the input alone.
#include <hip/hip_runtime.h>

#include <string>

#include "g1.h"
#include "hm_internal.h"

namespace hm {

#include "poseidon.inc"   // ps_get_words / ps_put_words
#include "range.inc"      // range_plain / range_limb_ext
#include "sorted.inc"

constexpr int SRT_THREADS = 256;
// records per LDS tile: 1024 x 9 words = 36 KiB, so four workgroups (16 waves) share a CU's 160 KiB
constexpr uint32_t SRT_TILE_LOG = 10, SRT_TILE = 1u << SRT_TILE_LOG;

__global__ __launch_bounds__(SRT_THREADS) void sorted_witness_kernel(const SortedArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
  if (idx >= a.lanes) return;                              // lanes is a multiple of 2^log_n: with log_n >= 6 whole waves leave
  const bool over = sorted_witness_lane(a, idx);
  if (!a.over) return;
  if (a.log_n >= 6) {                                      // a wave lies inside one circuit: one add per wave that has any
    const uint64_t votes = __ballot(over);
    if (votes && (threadIdx.x & 63) == 0) atomicAdd(a.over + (idx >> a.log_n), (uint32_t)__popcll(votes));
  } else if (over) {
    atomicAdd(a.over + (idx >> a.log_n), 1u);
  }
}

// the arguments were checked by the caller (capi_hash.hip: sorted_witness_args)
int sorted_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_ids,
                       uint32_t* d_advice, uint32_t* d_over, hipStream_t stream) {
  SortedArgs a;
  a.ids = d_ids;
  a.advice = d_advice;
  a.over = d_over;
  a.lanes = (uint64_t)m << log_n;
  a.max_bits = max_bits;
  a.acc_cols = acc_cols;
  a.log_n = log_n;
  a.rows = rows;
  if (d_over) HM_HIP_CHECK(hipMemsetAsync(d_over, 0, m * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(sorted_witness_kernel, dim3((uint32_t)((a.lanes + SRT_THREADS - 1) / SRT_THREADS)), dim3(SRT_THREADS), 0, stream, a);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// ---- the argsort ------------------------------------------------------------------------------------------------------------------------
// keys: n_pow2 x 8 words, rows: n_pow2 words; record i < n is (the canonical integer of element i, i), the others (all ones, i)
__global__ __launch_bounds__(SRT_THREADS) void srt_records_kernel(const uint32_t* __restrict__ values, uint64_t n, uint64_t n_pow2,
                                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
  if (i >= n_pow2) return;
  uint32_t p[8] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
  if (i < n) {
    uint32_t w[8];
    ps_get_words(values + i * 8, w);
    range_plain(w, p);
  }
  ps_put_words(keys + i * 8, p);
  rows[i] = (uint32_t)i;
}

__device__ __forceinline__ void srt_load(const uint32_t* keys, const uint32_t* rows, uint64_t i, uint32_t (&r)[9]) {
  uint32_t w[8];
  ps_get_words(keys + i * 8, w);
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = w[k];
  r[8] = rows[i];
}
__device__ __forceinline__ void srt_store(uint32_t* keys, uint32_t* rows, uint64_t i, const uint32_t (&r)[9]) {
  const uint32_t w[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
  ps_put_words(keys + i * 8, w);
  rows[i] = r[8];
}

// one compare-exchange stage with partner distance j >= SRT_TILE of the phase of length k: one lane per pair
__global__ __launch_bounds__(SRT_THREADS) void srt_global_kernel(uint32_t* keys, uint32_t* rows, uint64_t n_pow2, uint64_t k, uint64_t j) {
  const uint64_t t = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
  if (t >= n_pow2 / 2) return;
  const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  uint32_t a[9], b[9];
  srt_load(keys, rows, i, a);
  srt_load(keys, rows, l, b);
  const bool asc = (i & k) == 0;
  if (asc ? sorted_record_less(b, a) : sorted_record_less(a, b)) {
    srt_store(keys, rows, i, b);
    srt_store(keys, rows, l, a);
  }
}

// every stage with partner distance < SRT_TILE of the phases k_first .. k_last (k_first = 2: the whole sort of a tile), for one tile
// in LDS: word w of record e at lds[w][e], so the lanes of a wave read neighbouring words of one array
__global__ __launch_bounds__(SRT_THREADS) void srt_tile_kernel(uint32_t* keys, uint32_t* rows, uint64_t n_pow2, uint64_t k_first,
                                                               uint64_t k_last) {
  __shared__ uint32_t lds[9][SRT_TILE];
  const uint64_t base = (uint64_t)blockIdx.x * SRT_TILE;
  const uint32_t tile = n_pow2 < SRT_TILE ? (uint32_t)n_pow2 : SRT_TILE;
  for (uint32_t e = threadIdx.x; e < tile; e += SRT_THREADS) {
    uint32_t r[9];
    srt_load(keys, rows, base + e, r);
#pragma unroll
    for (int w = 0; w < 9; ++w) lds[w][e] = r[w];
  }
  __syncthreads();
  for (uint64_t k = k_first; k <= k_last; k <<= 1) {
    uint32_t j = (uint32_t)(k / 2 < tile ? k / 2 : tile / 2);
    for (; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < tile / 2; t += SRT_THREADS) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        uint32_t a[9], b[9];
#pragma unroll
        for (int w = 0; w < 9; ++w) {
          a[w] = lds[w][i];
          b[w] = lds[w][l];
        }
        const bool asc = ((base + i) & k) == 0;
        if (asc ? sorted_record_less(b, a) : sorted_record_less(a, b)) {
#pragma unroll
          for (int w = 0; w < 9; ++w) {
            lds[w][i] = b[w];
            lds[w][l] = a[w];
          }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t e = threadIdx.x; e < tile; e += SRT_THREADS) {
    uint32_t r[9];
#pragma unroll
    for (int w = 0; w < 9; ++w) r[w] = lds[w][e];
    srt_store(keys, rows, base + e, r);
  }
}

__global__ __launch_bounds__(SRT_THREADS) void srt_rows_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint64_t* __restrict__ perm) {
  const uint64_t i = (uint64_t)blockIdx.x * SRT_THREADS + threadIdx.x;
  if (i < n) perm[i] = rows[i];
}

// d_perm may be null: the caller reads the sorted records themselves (logup.hip: the general-key multiplicities)
int fr_sort_records_run(const uint32_t* d_values, uint64_t n, uint64_t n_pow2, uint32_t* d_keys, uint32_t* d_rows, uint64_t* d_perm,
                        hipStream_t stream) {
  const auto blocks = [](uint64_t lanes) { return dim3((unsigned)((lanes + SRT_THREADS - 1) / SRT_THREADS)); };
  hipLaunchKernelGGL(srt_records_kernel, blocks(n_pow2), dim3(SRT_THREADS), 0, stream, d_values, n, n_pow2, d_keys, d_rows);
  if (n_pow2 >= 2) {
    const dim3 tiles((unsigned)((n_pow2 + SRT_TILE - 1) / SRT_TILE));
    const uint64_t in_tile = n_pow2 < SRT_TILE ? n_pow2 : (uint64_t)SRT_TILE;
    hipLaunchKernelGGL(srt_tile_kernel, tiles, dim3(SRT_THREADS), 0, stream, d_keys, d_rows, n_pow2, (uint64_t)2, in_tile);
    for (uint64_t k = (uint64_t)SRT_TILE * 2; k <= n_pow2; k <<= 1) {
      for (uint64_t j = k / 2; j >= SRT_TILE; j >>= 1)
        hipLaunchKernelGGL(srt_global_kernel, blocks(n_pow2 / 2), dim3(SRT_THREADS), 0, stream, d_keys, d_rows, n_pow2, k, j);
      hipLaunchKernelGGL(srt_tile_kernel, tiles, dim3(SRT_THREADS), 0, stream, d_keys, d_rows, n_pow2, k, k);
    }
  }
  if (d_perm) hipLaunchKernelGGL(srt_rows_kernel, blocks(n), dim3(SRT_THREADS), 0, stream, (const uint32_t*)d_rows, n, d_perm);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// A fixed chain of launches whatever the values; the records are stream-ordered scratch (36 bytes for each of the next power of two
// of n).  The arguments were checked by the caller (capi_hash.hip).
int fr_argsort_run(const uint32_t* d_values, size_t n, uint64_t* d_perm, hipStream_t stream) {
  uint64_t n_pow2 = 1;
  while (n_pow2 < (uint64_t)n) n_pow2 <<= 1;
  return stream_scratch("fr_argsort", (size_t)n_pow2 * 36, stream, [&](uint8_t* ws) -> int {
    uint32_t* keys = (uint32_t*)ws;
    return fr_sort_records_run(d_values, n, n_pow2, keys, keys + n_pow2 * 8, d_perm, stream);
  });
}

}  // namespace hm
