// logup.hip -- the logUp lookup argument on the device: the multiplicity column m of an argument and the
// running sums phi, the kernels and their drivers.  The per-lane functions are in logup.inc, which host_check.cpp compiles too.
//
// Multiplicities.  One argument = one table column and c input columns of `rows` live rows; m[i] = the number of (input, row) pairs
// whose value is the table's value on row i, if i is the FIRST table row holding that value, otherwise 0.  No column is sorted when
// the keys are small:
//   bits      the plain integers of every table value, OR-ed per wave into a few slots: the host picks the route by them
//   small keys (all below 2^bits, bits <= LU_COUNT_BITS), value bins, grid.y = argument:
//     first   first[v] = the least table row holding v                        (32-bit atomicMin, one per table row)
//     count   count[v] += the (input, row) pairs holding v                    (one atomicAdd per distinct value and wave)
//     write   m[i] = count[t[i]] if first[t[i]] = i, else 0                   (a lane per table row)
//   general keys, an argument after the other: the table as (key, row) records through sorted.hip's network, then
//     search  a lane per row finds the lower bound of each of its c keys and adds to the counter of that record's ROW (equal keys
//             stand by ascending row, so the lower bound is the first row); one atomicAdd per distinct record and wave
//     write   m[i] = counter[i]
// An input key outside the bins, in a bin no table row holds, or not among the records raises the argument's `missing` word.
// All atomics are vector atomics on 32-bit words.
//
// Running sums.  out[i] = sum_{j < i} terms[j] mod r, three plain launches with the column in grid.y, the shape of accumulator.hip's
// prefix sum: the block totals, their scan by one workgroup per column, the rows.  Shuffles inside a wave, the wave totals through
// LDS; no look-back, nothing polled, nothing atomic.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "g1.h"
#include "hm_internal.h"
#include "host_fr.h"
#include "mock_check.h"   // mock_key_cmp / mock_key_lower_bound: the order of the sorted keys

namespace hm {

#include "poseidon.inc"   // ps_get_words / ps_put_words
#include "range.inc"      // range_plain
#include "sorted.inc"     // sorted_sub_mod / sorted_const_words
#include "logup.inc"

constexpr int LU_THREADS = 256, LU_WAVES = LU_THREADS / 64;
static_assert(LU_THREADS == (int)LU_SCAN_ROWS, "a lane per row of the scan's block");
constexpr uint32_t LU_KB_SLOTS = 32, LU_KB_STRIDE = 16;      // the key-bit words: a 64-byte line per slot, as lookup.hip's
constexpr size_t LU_BIN_BUDGET = (size_t)256 << 20;          // bytes of value bins in flight: the arguments go in chunks under it

// one argument of a batch, in device memory
struct LuArg {
  const uint32_t* table;
  uint32_t* m;
  uint32_t first_input, c;                                    // its input columns: inputs[first_input .. first_input + c)
};

// counters[idx] += the number of lanes of the wave that are `on` with this idx: one atomic per distinct idx of the wave, so a column
// that holds one value does not hammer one counter.  Every lane of the wave must call.
__device__ __forceinline__ void lu_wave_add(uint32_t* counters, uint32_t idx, bool on) {
  uint64_t todo = __ballot(on);
  while (todo) {
    const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
    const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
    const uint64_t same = __ballot(on && idx == li) & todo;
    if ((threadIdx.x & 63) == leader) atomicAdd(counters + li, (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

__device__ __forceinline__ void lu_wave_flag(uint32_t* flag, bool bad) {
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// kbits slot (blockIdx.x % LU_KB_SLOTS): word 0 |= word 0 of the table keys, word 1 |= their words 1 .. 7
__global__ __launch_bounds__(LU_THREADS) void lu_bits_kernel(const LuArg* args, uint64_t rows, uint32_t* __restrict__ kbits) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  uint32_t lo_bits = 0, hi_bits = 0;
  if (i < rows) {
    uint32_t key[8];
    (void)lu_key(args[blockIdx.y].table + i * 8, 1u, key);
    lo_bits = key[0];
    hi_bits = key[1] | key[2] | key[3] | key[4] | key[5] | key[6] | key[7];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo_bits |= __shfl_xor(lo_bits, off, 64);
    hi_bits |= __shfl_xor(hi_bits, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    uint32_t* slot = kbits + (size_t)(blockIdx.x % LU_KB_SLOTS) * LU_KB_STRIDE;
    if (lo_bits) atomicOr(slot, lo_bits);
    if (hi_bits) atomicOr(slot + 1, hi_bits);
  }
}

// ---- small keys: bins[2 a nbins ..] = the counts of argument a, then its first rows ------------------------------------------------------
__global__ __launch_bounds__(LU_THREADS) void lu_first_kernel(const LuArg* args, uint64_t rows, uint32_t nbins, uint32_t* bins) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  if (i >= rows) return;
  uint32_t* first = bins + ((size_t)2 * blockIdx.y + 1) * nbins;
  uint32_t key[8];
  if (lu_key(args[blockIdx.y].table + i * 8, nbins, key)) atomicMin(first + key[0], (uint32_t)i);
}

__global__ __launch_bounds__(LU_THREADS) void lu_count_kernel(const LuArg* args, const uint32_t* const* inputs, uint64_t rows, uint32_t nbins,
                                                              uint32_t* bins, uint32_t* flags) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  const LuArg a = args[blockIdx.y];
  uint32_t* count = bins + (size_t)2 * blockIdx.y * nbins;
  const uint32_t* first = count + nbins;
  const bool live = i < rows;
  bool bad = false;
  for (uint32_t j = 0; j < a.c; ++j) {
    uint32_t key[8], bin = 0;
    bool ok = false;
    if (live) {
      ok = lu_key(inputs[a.first_input + j] + i * 8, nbins, key) && first[key[0]] != LU_NO_ROW;
      bin = ok ? key[0] : 0u;
      bad = bad || !ok;
    }
    lu_wave_add(count, bin, ok);
  }
  lu_wave_flag(flags + blockIdx.y, bad);
}

__global__ __launch_bounds__(LU_THREADS) void lu_write_small_kernel(const LuArg* args, uint64_t rows, uint32_t nbins, const uint32_t* bins,
                                                                    LuFr to_mont) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  if (i >= rows) return;
  const LuArg a = args[blockIdx.y];
  const uint32_t* count = bins + (size_t)2 * blockIdx.y * nbins;
  const uint32_t* first = count + nbins;
  uint32_t key[8], w[8];
  const bool in = lu_key(a.table + i * 8, nbins, key);
  const uint32_t mine = in && first[key[0]] == (uint32_t)i ? count[key[0]] : 0u;
  lu_count_ext(mine, to_mont, w);
  ps_put_words(a.m + i * 8, w);
}

// ---- general keys: ONE argument; keys / srows the table's sorted records, counters a word per table row --------------------------------
__global__ __launch_bounds__(LU_THREADS) void lu_search_kernel(const LuArg* arg, const uint32_t* const* inputs, uint64_t rows,
                                                               const uint32_t* __restrict__ keys, const uint32_t* __restrict__ srows,
                                                               uint32_t* counters, uint32_t* flag) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  const LuArg a = *arg;
  const bool live = i < rows;
  bool bad = false;
  for (uint32_t j = 0; j < a.c; ++j) {
    uint32_t row = 0;
    bool ok = false;
    if (live) {
      uint32_t key[8];
      (void)lu_key(inputs[a.first_input + j] + i * 8, 1u, key);
      const uint64_t at = lu_find(keys, rows, key);
      ok = at < rows;
      row = ok ? srows[at] : 0u;
      bad = bad || !ok;
    }
    lu_wave_add(counters, row, ok);
  }
  lu_wave_flag(flag, bad);
}

__global__ __launch_bounds__(LU_THREADS) void lu_write_general_kernel(const LuArg* arg, uint64_t rows, const uint32_t* __restrict__ counters,
                                                                      LuFr to_mont) {
  const uint64_t i = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  if (i >= rows) return;
  uint32_t w[8];
  lu_count_ext(counters[i], to_mont, w);
  ps_put_words(arg->m + i * 8, w);
}

// 1 <= rows < 2^31, every c >= 1 and c * rows < 2^32, no null pointer: checked by the caller
int logup_multiplicities_run(const void* const* d_tables, const void* const* d_inputs, const uint32_t* input_counts, size_t count, uint64_t rows,
                             void* const* d_m, int* missing, hipStream_t stream) {
  const char* who = "logup multiplicities";
  std::vector<LuArg> h_args(count);
  size_t total_inputs = 0;
  for (size_t a = 0; a < count; ++a) {
    h_args[a] = LuArg{(const uint32_t*)d_tables[a], (uint32_t*)d_m[a], (uint32_t)total_inputs, input_counts[a]};
    total_inputs += input_counts[a];
  }
  LuFr to_mont;
  {
    const host::Fr4 r2 = {{0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL}};   // 2^512 mod r as words = the element 2^256
    host::fr_to_internal9(r2, to_mont.l);
  }
  const size_t args_bytes = pad64(count * sizeof(LuArg)), in_bytes = pad64(total_inputs * sizeof(void*)), flag_bytes = pad64(count * 4);
  const size_t kb_bytes = pad64((size_t)LU_KB_SLOTS * LU_KB_STRIDE * 4);
  const uint32_t rb = (uint32_t)((rows + LU_THREADS - 1) / LU_THREADS);
  std::vector<uint32_t> h_flags(count, 0u);
  int rc = HM_OK;                                                    // the first failure, with its message
  auto fail = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == HM_OK) rc = hm_fail(HM_ERR_HIP, std::string(who) + ": " + what + ": " + hipGetErrorString(e));
    return e != hipSuccess;
  };
  const int scope_rc = stream_scratch(who, args_bytes + in_bytes + flag_bytes + kb_bytes, stream, [&](uint8_t* head) -> int {
    LuArg* args = (LuArg*)head;
    const uint32_t* const* inputs = (const uint32_t* const*)(head + args_bytes);
    uint32_t *flags = (uint32_t*)(head + args_bytes + in_bytes), *kbits = (uint32_t*)(head + args_bytes + in_bytes + flag_bytes);
    // pageable sources: the runtime has taken its copies when these return
    if (fail(hipMemcpyAsync(args, h_args.data(), count * sizeof(LuArg), hipMemcpyHostToDevice, stream), "upload")) return rc;
    if (fail(hipMemcpyAsync((void*)inputs, d_inputs, total_inputs * sizeof(void*), hipMemcpyHostToDevice, stream), "upload")) return rc;
    if (fail(hipMemsetAsync(flags, 0, flag_bytes + kb_bytes, stream), "memset")) return rc;
    for (size_t a0 = 0; a0 < count; a0 += 32768) {
      const uint32_t cnt = (uint32_t)(count - a0 < 32768 ? count - a0 : 32768);
      hipLaunchKernelGGL(lu_bits_kernel, dim3(rb, cnt), dim3(LU_THREADS), 0, stream, (const LuArg*)(args + a0), rows, kbits);
    }
    uint32_t h_bits[LU_KB_SLOTS * LU_KB_STRIDE];
    if (fail(hipMemcpyAsync(h_bits, kbits, sizeof h_bits, hipMemcpyDeviceToHost, stream), "key bits")) return rc;
    if (fail(hipStreamSynchronize(stream), "key bits")) return rc;
    uint32_t lo_or = 0, hi_or = 0;
    for (uint32_t s = 0; s < LU_KB_SLOTS; ++s) {
      lo_or |= h_bits[s * LU_KB_STRIDE];
      hi_or |= h_bits[s * LU_KB_STRIDE + 1];
    }
    uint32_t need = 1;
    while (need < 32 && (lo_or >> need) != 0) ++need;
    int work_rc;
    if (hi_or == 0 && need <= LU_COUNT_BITS) {
      const uint32_t nbins = 1u << need;
      const size_t per_arg = (size_t)2 * nbins * 4;
      size_t chunk = LU_BIN_BUDGET / per_arg;                  // >= 32 at 2^20 bins
      if (chunk > 32768) chunk = 32768;
      if (chunk > count) chunk = count;
      work_rc = stream_scratch(who, chunk * per_arg, stream, [&](uint8_t* work) -> int {
        uint32_t* bins = (uint32_t*)work;
        for (size_t a0 = 0; a0 < count; a0 += chunk) {
          const uint32_t cnt = (uint32_t)(count - a0 < chunk ? count - a0 : chunk);
          for (uint32_t a = 0; a < cnt; ++a)                        // the counts to 0, the first rows to LU_NO_ROW
            if (fail(hipMemsetAsync(bins + (size_t)2 * a * nbins, 0, (size_t)nbins * 4, stream), "memset") ||
                fail(hipMemsetAsync(bins + ((size_t)2 * a + 1) * nbins, 0xFF, (size_t)nbins * 4, stream), "memset"))
              return rc;
          const LuArg* part = args + a0;
          hipLaunchKernelGGL(lu_first_kernel, dim3(rb, cnt), dim3(LU_THREADS), 0, stream, part, rows, nbins, bins);
          hipLaunchKernelGGL(lu_count_kernel, dim3(rb, cnt), dim3(LU_THREADS), 0, stream, part, inputs, rows, nbins, bins, flags + a0);
          hipLaunchKernelGGL(lu_write_small_kernel, dim3(rb, cnt), dim3(LU_THREADS), 0, stream, part, rows, nbins, (const uint32_t*)bins, to_mont);
        }
        return HM_OK;
      });
    } else {
      if (rows > ((uint64_t)1 << 26))
        return hm_fail(HM_ERR_BAD_ARG, std::string(who) + ": a table with keys of 2^" + std::to_string(LU_COUNT_BITS) + " and above takes at most 2^26 rows");
      uint64_t n2 = 1;
      while (n2 < rows) n2 <<= 1;
      const size_t key_bytes = pad64((size_t)n2 * 32), row_bytes = pad64((size_t)n2 * 4), cnt_bytes = pad64((size_t)rows * 4);
      work_rc = stream_scratch(who, key_bytes + row_bytes + cnt_bytes, stream, [&](uint8_t* work) -> int {
        uint32_t *keys = (uint32_t*)work, *srows = (uint32_t*)(work + key_bytes), *counters = (uint32_t*)(work + key_bytes + row_bytes);
        for (size_t a = 0; a < count; ++a) {
          if (const int src = fr_sort_records_run(h_args[a].table, rows, n2, keys, srows, nullptr, stream)) return src;
          if (fail(hipMemsetAsync(counters, 0, (size_t)rows * 4, stream), "memset")) return rc;
          hipLaunchKernelGGL(lu_search_kernel, dim3(rb), dim3(LU_THREADS), 0, stream, (const LuArg*)(args + a), inputs, rows, (const uint32_t*)keys,
                             (const uint32_t*)srows, counters, flags + a);
          hipLaunchKernelGGL(lu_write_general_kernel, dim3(rb), dim3(LU_THREADS), 0, stream, (const LuArg*)(args + a), rows,
                             (const uint32_t*)counters, to_mont);
        }
        return HM_OK;
      });
    }
    if (work_rc != HM_OK) return work_rc;
    if (fail(hipGetLastError(), "launch")) return rc;
    if (fail(hipMemcpyAsync(h_flags.data(), flags, count * 4, hipMemcpyDeviceToHost, stream), "flags")) return rc;
    (void)fail(hipStreamSynchronize(stream), "flags");
    return rc;
  });
  if (scope_rc != HM_OK) return scope_rc;
  bool any = false;
  for (size_t a = 0; a < count; ++a) {
    if (missing) missing[a] = h_flags[a] ? 1 : 0;
    any = any || h_flags[a] != 0;
  }
  if (any) return hm_fail(HM_ERR_NOT_FOUND, std::string(who) + ": an input value is missing from the table (ConstraintSystemFailure)");
  return HM_OK;
}

// ---- the running sums --------------------------------------------------------------------------------------------------------------------
// inclusive scan over the block of the 8-word values; lds: LU_WAVES rows, free to be written.  Every lane of the block must call.
__device__ __forceinline__ void gs_block_scan(uint32_t (&v)[8], uint32_t (*lds)[8]) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = __shfl_up(v[k], d, 64);
    if (lane >= (uint32_t)d) lu_add_mod(v, o);
  }
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 8; ++k) lds[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < LU_WAVES - 1; ++w) {
    if ((uint32_t)w < wave) {
      uint32_t o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = lds[w][k];
      lu_add_mod(v, o);
    }
  }
}

__device__ __forceinline__ void gs_load(const uint32_t* column, uint64_t t, uint64_t n, uint32_t (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0;
  if (t < n) ps_get_words(column + t * 8, v);
}

// totals[c][b] = the sum of rows [b B, (b + 1) B) of column c
__global__ __launch_bounds__(LU_THREADS) void gs_reduce_kernel(const uint32_t* const* terms, uint64_t n, uint32_t* totals, uint32_t n_blocks) {
  __shared__ uint32_t lds[LU_WAVES][8];
  uint32_t v[8];
  gs_load(terms[blockIdx.y], (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x, n, v);
  gs_block_scan(v, lds);
  if (threadIdx.x == LU_THREADS - 1) ps_put_words(totals + ((size_t)blockIdx.y * n_blocks + blockIdx.x) * 8, v);
}

// per column: thread i takes per_thread consecutive totals, the block scans the threads' sums, thread i writes its totals back as the
// sum of everything before each
__global__ __launch_bounds__(LU_THREADS) void gs_scan_kernel(uint32_t* totals, uint32_t n_blocks, uint32_t per_thread) {
  __shared__ uint32_t lds[LU_WAVES][8];
  uint32_t* tot = totals + (size_t)blockIdx.x * n_blocks * 8;
  const uint64_t lo = (uint64_t)threadIdx.x * per_thread, hi = lo + per_thread < n_blocks ? lo + per_thread : n_blocks;
  uint32_t mine[8] = {0, 0, 0, 0, 0, 0, 0, 0}, run[8], w[8];
  for (uint64_t j = lo; j < hi; ++j) {
    ps_get_words(tot + j * 8, w);
    lu_add_mod(mine, w);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) run[k] = mine[k];
  gs_block_scan(run, lds);
  sorted_sub_mod(run, mine);                                  // exclusive: what stands before this thread's totals
  for (uint64_t j = lo; j < hi; ++j) {
    ps_get_words(tot + j * 8, w);
    ps_put_words(tot + j * 8, run);
    lu_add_mod(run, w);
  }
}

// out[t] = totals[c][b] + the rows of the block before t; a lane reads its term before it writes its row, so out[c] may be terms[c]
__global__ __launch_bounds__(LU_THREADS) void gs_rows_kernel(const uint32_t* const* terms, uint64_t n, const uint32_t* totals, uint32_t n_blocks,
                                                             uint32_t* const* out) {
  __shared__ uint32_t lds[LU_WAVES][8];
  const uint64_t t = (uint64_t)blockIdx.x * LU_THREADS + threadIdx.x;
  uint32_t v[8], s[8], base[8];
  gs_load(terms[blockIdx.y], t, n, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = v[k];
  gs_block_scan(s, lds);
  if (t >= n) return;
  sorted_sub_mod(s, v);
  ps_get_words(totals + ((size_t)blockIdx.y * n_blocks + blockIdx.x) * 8, base);
  lu_add_mod(s, base);
  ps_put_words(out[blockIdx.y] + t * 8, s);
}

// 1 <= n < 2^32 * LU_SCAN_ROWS, 1 <= count <= 65535, no null pointer, no overlap but out[c] == terms[c]: checked by the caller
int fr_grand_sum_batch_run(const void* const* d_terms, uint64_t n, void* const* d_out, size_t count, hipStream_t stream) {
  const uint32_t n_blocks = (uint32_t)((n + LU_THREADS - 1) / LU_THREADS);
  const uint32_t per_thread = (n_blocks + LU_THREADS - 1) / LU_THREADS;
  const size_t ptr_bytes = pad64(count * sizeof(void*)), tot_bytes = pad64(count * (size_t)n_blocks * 32);
  return stream_scratch("grand sum", 2 * ptr_bytes + tot_bytes, stream, [&](uint8_t* ws) -> int {
    const uint32_t* const* terms = (const uint32_t* const*)ws;
    uint32_t* const* out = (uint32_t* const*)(ws + ptr_bytes);
    uint32_t* totals = (uint32_t*)(ws + 2 * ptr_bytes);
    int rc = HM_OK;
    // pageable sources: the runtime has taken its copies when these return
    if (hipMemcpyAsync((void*)terms, d_terms, count * sizeof(void*), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync((void*)out, d_out, count * sizeof(void*), hipMemcpyHostToDevice, stream) != hipSuccess)
      rc = hm_fail(HM_ERR_HIP, "grand sum: upload failed");
    if (rc == HM_OK) {
      hipLaunchKernelGGL(gs_reduce_kernel, dim3(n_blocks, (uint32_t)count), dim3(LU_THREADS), 0, stream, terms, n, totals, n_blocks);
      hipLaunchKernelGGL(gs_scan_kernel, dim3((uint32_t)count), dim3(LU_THREADS), 0, stream, totals, n_blocks, per_thread);
      hipLaunchKernelGGL(gs_rows_kernel, dim3(n_blocks, (uint32_t)count), dim3(LU_THREADS), 0, stream, terms, n, (const uint32_t*)totals, n_blocks, out);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string("grand sum: ") + hipGetErrorString(e));
    }
    return rc;
  });
}

}  // namespace hm
