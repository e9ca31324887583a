// accumulator.hip -- the witness of the SafeAccumulator circuit on the device: the kernels and
// accumulator_witness_run.  The row function is in accumulator.inc, which host_check.cpp compiles too.
//
// The rows of a circuit depend on each other through S_{r-1}, a prefix sum of the values' low 64 bits (wrapping: W <= 64).  Four
// launches, each a plain grid with the circuit in blockIdx.y; no lane waits for another block, nothing is polled, nothing is atomic:
//   reduce   block (b, c) sums the values of table rows [b B, (b + 1) B) of circuit c into totals[c][b]
//   scan     one block per circuit: totals[c][b] <- S_0 + the totals before b; row 0's accumulate cells; the initial state's verdict
//   rows     block (b, c) reads its values again, scans them in the block (shuffles inside a wave, the wave totals through LDS),
//            and every lane writes its whole row from (S_{r-1}, v_r); the block's count of failing rows goes to counts[c][b]
//   count    one block per circuit: over[c] = the sum of its counts
#include <hip/hip_runtime.h>

#include "g1.h"
#include "hm_internal.h"

namespace hm {

#include "poseidon.inc"   // ps_get_words / ps_put_words
#include "range.inc"      // range_plain / range_limb_ext
#include "accumulator.inc"

constexpr int ACC_THREADS = 256, ACC_WAVES = ACC_THREADS / 64;

// inclusive scan over the block; lds: ACC_WAVES words, free to be written.  Every lane of the block must call.
__device__ __forceinline__ uint64_t acc_block_scan(uint64_t v, uint64_t* lds) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(inc, d);
    if (lane >= (uint32_t)d) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t before = 0;
#pragma unroll
  for (int w = 0; w < ACC_WAVES - 1; ++w) before += (uint32_t)w < wave ? lds[w] : 0;
  return before + inc;
}

// the low 64 bits of the value on table row t of circuit c (zero outside rows 1 .. rows)
__device__ __forceinline__ uint64_t acc_lane_value(const AccArgs& a, uint64_t c, uint64_t t, uint32_t (&w)[8], bool& big) {
  big = false;
  if (t == 0 || t > a.rows) return 0;
  ps_get_words(a.values + (c * a.rows + (t - 1)) * 8, w);
  return acc_value_low(w, a.max_bits, big);
}

__global__ __launch_bounds__(ACC_THREADS) void accumulator_reduce_kernel(const AccArgs a, uint64_t* totals, uint32_t n_blocks) {
  __shared__ uint64_t lds[ACC_WAVES];
  const uint64_t c = blockIdx.y, t = (uint64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  uint32_t w[8];
  bool big;
  const uint64_t sum = acc_block_scan(acc_lane_value(a, c, t, w, big), lds);
  if (threadIdx.x == ACC_THREADS - 1) totals[c * n_blocks + blockIdx.x] = sum;
}

// per circuit: thread i takes per_thread consecutive totals, the block scans the threads' sums, thread i writes its totals back as
// S_0 + everything before each
__global__ __launch_bounds__(ACC_THREADS) void accumulator_scan_kernel(const AccArgs a, uint64_t* totals, uint32_t n_blocks, uint32_t per_thread,
                                                                     uint32_t* counts) {
  __shared__ uint64_t lds[ACC_WAVES];
  const uint64_t c = blockIdx.x;
  uint64_t* tot = totals + c * n_blocks;
  const uint64_t lo = (uint64_t)threadIdx.x * per_thread, hi = lo + per_thread < n_blocks ? lo + per_thread : n_blocks;
  uint64_t mine = 0;
  for (uint64_t j = lo; j < hi; ++j) mine += tot[j];
  uint64_t s0;
  const bool bad = acc_initial_state(a, c, s0);             // acc_cols loads of a line every lane shares
  uint64_t run = s0 + acc_block_scan(mine, lds) - mine;
  for (uint64_t j = lo; j < hi; ++j) {
    const uint64_t v = tot[j];
    tot[j] = run;
    run += v;
  }
  if (threadIdx.x < a.acc_cols) acc_initial_cell(a, c, threadIdx.x);
  if (counts && threadIdx.x == 0) counts[c * (n_blocks + 1) + n_blocks] = bad ? 1u : 0u;
}

__global__ __launch_bounds__(ACC_THREADS) void accumulator_rows_kernel(const AccArgs a, const uint64_t* totals, uint32_t n_blocks, uint32_t* counts) {
  __shared__ uint64_t lds[ACC_WAVES];
  __shared__ uint32_t votes[ACC_WAVES];
  const uint64_t c = blockIdx.y, t = (uint64_t)blockIdx.x * ACC_THREADS + threadIdx.x, n = (uint64_t)1 << a.log_n;
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  const uint32_t n_cols = 2 + 2 * a.acc_cols;
  uint32_t* out = a.advice + c * n_cols * col_words + t * 8;
  if (blockIdx.x >= n_blocks) {                             // the whole block lies above the last value: rows of zeros
    if (t < n) acc_zero_cells(out, col_words, 0, n_cols);
    return;
  }
  uint32_t w[8];
  bool big;
  const uint64_t v = acc_lane_value(a, c, t, w, big);
  const uint64_t s_prev = (totals[c * n_blocks + blockIdx.x] + acc_block_scan(v, lds) - v) & acc_width_mask(a.max_bits * a.acc_cols);
  bool over = false;
  if (t == 0) {
    acc_zero_cells(out, col_words, 0, 2 + a.acc_cols);      // the accumulate cells of row 0 are the scan kernel's
  } else if (t <= a.rows) {
    uint64_t s_new;
    over = accumulator_row(a, out, s_prev, w, s_new);
    if (t == a.rows) acc_write_finals(a, c, s_new);
  } else if (t < n) {
    acc_zero_cells(out, col_words, 0, n_cols);
  }
  if (!counts) return;
  const uint64_t ballot = __ballot(over);
  if ((threadIdx.x & 63) == 0) votes[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < ACC_WAVES; ++i) sum += votes[i];
    counts[c * (n_blocks + 1) + blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(ACC_THREADS) void accumulator_count_kernel(const uint32_t* counts, uint32_t n_counts, uint32_t* over) {
  __shared__ uint64_t lds[ACC_WAVES];
  const uint32_t* mine = counts + (uint64_t)blockIdx.x * n_counts;
  uint64_t sum = 0;
  for (uint32_t j = threadIdx.x; j < n_counts; j += ACC_THREADS) sum += mine[j];
  sum = acc_block_scan(sum, lds);
  if (threadIdx.x == ACC_THREADS - 1) over[blockIdx.x] = (uint32_t)sum;
}

// the arguments were checked by the caller (capi_hash.hip: accumulator_witness_args); inverses_ext: host memory
int accumulator_witness_run(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* d_values,
                            const uint64_t* d_initial, const uint64_t* inverses_ext, uint32_t* d_advice, uint64_t* d_finals, uint32_t* d_over,
                            hipStream_t stream, double* part_ms) {
  const uint32_t n_blocks = rows / ACC_THREADS + 1;                        // the blocks that hold a table row 0 .. rows
  const uint32_t all_blocks = (uint32_t)((((uint64_t)1 << log_n) + ACC_THREADS - 1) / ACC_THREADS);
  const uint32_t per_thread = (n_blocks + ACC_THREADS - 1) / ACC_THREADS;
  const size_t inv_bytes = pad64((((size_t)1 << max_bits) - 1) * 32), tot_bytes = pad64(m * n_blocks * sizeof(uint64_t));
  const size_t cnt_bytes = d_over ? m * (n_blocks + 1) * sizeof(uint32_t) : 0;
  return stream_scratch("accumulator_witness", inv_bytes + tot_bytes + cnt_bytes, stream, [&](uint8_t* ws) -> int {
    int rc = HM_OK;
    hipEvent_t ev[5] = {};                                     // part_ms: events around the four launches (the call then waits for them)
    if (part_ms)
      for (hipEvent_t& e : ev)
        if (rc == HM_OK && hipEventCreate(&e) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "accumulator_witness: hipEventCreate failed");
    auto mark = [&](int i) {
      if (part_ms && rc == HM_OK && hipEventRecord(ev[i], stream) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "accumulator_witness: hipEventRecord failed");
    };
    // a pageable source: the runtime has taken its copy when this returns
    if (hipMemcpyAsync(ws, inverses_ext, (((size_t)1 << max_bits) - 1) * 32, hipMemcpyHostToDevice, stream) != hipSuccess)
      rc = hm_fail(HM_ERR_HIP, "accumulator_witness: upload failed");
    mark(0);
    if (rc == HM_OK) {
      AccArgs a;
      a.values = d_values;
      a.initial = d_initial;
      a.inverses = (const uint32_t*)ws;
      a.advice = d_advice;
      a.finals = d_finals;
      a.max_bits = max_bits;
      a.acc_cols = acc_cols;
      a.log_n = log_n;
      a.rows = rows;
      uint64_t* totals = (uint64_t*)(ws + inv_bytes);
      uint32_t* counts = d_over ? (uint32_t*)(ws + inv_bytes + tot_bytes) : nullptr;
      hipLaunchKernelGGL(accumulator_reduce_kernel, dim3(n_blocks, (uint32_t)m), dim3(ACC_THREADS), 0, stream, a, totals, n_blocks);
      mark(1);
      hipLaunchKernelGGL(accumulator_scan_kernel, dim3((uint32_t)m), dim3(ACC_THREADS), 0, stream, a, totals, n_blocks, per_thread, counts);
      mark(2);
      hipLaunchKernelGGL(accumulator_rows_kernel, dim3(all_blocks, (uint32_t)m), dim3(ACC_THREADS), 0, stream, a, (const uint64_t*)totals, n_blocks,
                         counts);
      mark(3);
      if (counts)
        hipLaunchKernelGGL(accumulator_count_kernel, dim3((uint32_t)m), dim3(ACC_THREADS), 0, stream, (const uint32_t*)counts, n_blocks + 1, d_over);
      mark(4);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = hm_fail(HM_ERR_HIP, std::string("accumulator_witness: ") + hipGetErrorString(e));
    }
    if (part_ms) {
      if (rc == HM_OK && hipEventSynchronize(ev[4]) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "accumulator_witness: hipEventSynchronize failed");
      for (int i = 0; i < 4; ++i) {
        float ms = 0;
        if (rc == HM_OK && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "accumulator_witness: hipEventElapsedTime failed");
        part_ms[i] = ms;
      }
      for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    }
    return rc;
  });
}

}  // namespace hm
