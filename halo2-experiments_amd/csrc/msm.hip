// msm.hip -- Pippenger bucket MSM over BN256 G1 for gfx950 (replaces
// halo2_proofs::arithmetic::best_multiexp, SURVEY.md §3.3: sum_i coeffs[i] * bases[i]).
//
// Pipeline (all device-resident, nothing is read back before the final window sums):
//   K0  digits      scalar (radix-2^256 Montgomery) -> canonical -> W signed c-bit digits
//   K2  sort        two-level counting sort through LDS (coarse partition, then one workgroup per
//                   region: fine histogram -> bucket counts; global scan -> bucket + task offsets;
//                   in-region scatter) -> point indices grouped by bucket
//   K2b task order  counting sort of the tasks by chain length, longest first: the 64 lanes of a
//                   K3 wave run chains of equal length
//   K3  accumulate  one lane per task (a bucket, or a <= L-long slice of a long bucket): a serial
//                   chain of extended-Jacobian mixed additions, the accumulator living in registers
//   K3b finalize    per bucket: sum of its task partials (lane / workgroup / sliced workgroups)
//   K4a/K4b reduce  per window sum_b b*B_b by segmented running sums, then a tree in LDS
//   host            Horner over the W window sums (c doublings each) and affine normalisation
// Differences from the reference's CPU algorithm that do not change the (canonical) result:
// signed digits (half the buckets), a window size chosen for the whole array instead of per
// thread chunk, buckets summed in sorted order.  Long buckets (constant columns, tiny scalars) are
// split into tasks so that one hot bucket cannot serialise the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "fq_inverse.h"
#include "hm_internal.h"
#include "host_fq.h"
#include "msm_dev.h"

namespace hm {


// Every counter an MSM starts from zero is cleared by ONE launch of its own (instead of four
// hipMemsetAsync calls): the bucket counts (the cooperative histogram adds into them), the big-region
// list count, the task-length key histogram, the hot-bucket queue counts.
__global__ void msm_init_counters_kernel(uint32_t* __restrict__ bcnt, size_t nbt, uint32_t* __restrict__ br_count,
                                         uint32_t* __restrict__ khist, uint32_t nkeys, uint32_t* __restrict__ big_count) {
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = i0; i < nbt; i += stride) bcnt[i] = 0;
  if (i0 < nkeys) khist[i0] = 0;
  if (i0 < 4) {
    if (br_count) br_count[i0] = 0;
    big_count[i0] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// bases: external affine -> internal packed (x, y) + identity flags
// ---------------------------------------------------------------------------------------------
__global__ void msm_convert_bases_kernel(const uint32_t* __restrict__ ext, uint32_t* __restrict__ xy,
                                         uint8_t* __restrict__ inf, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(ext + i * 16);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const uint32_t wy[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= wx[k] | wy[k];
  uint32_t ox[8], oy[8];
  fe_pack(ox, fe_from_ext<FqParams>(wx));
  fe_pack(oy, fe_from_ext<FqParams>(wy));
  uint4* o = reinterpret_cast<uint4*>(xy + i * 16);
  o[0] = make_uint4(ox[0], ox[1], ox[2], ox[3]);
  o[1] = make_uint4(ox[4], ox[5], ox[6], ox[7]);
  o[2] = make_uint4(oy[0], oy[1], oy[2], oy[3]);
  o[3] = make_uint4(oy[4], oy[5], oy[6], oy[7]);
  inf[i] = any == 0 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// K0: signed window digits.  digits[w*n + i] in [-2^(c-1)+1, 2^(c-1)], 0 = skip.
// ---------------------------------------------------------------------------------------------
// Tasks are cut to at most L pairs.  The host picks L for the worst case (every digit non-zero); the
// first sort level counts the pairs that really exist, and when they are far fewer (zero or repeated
// digits: flag and selector-like columns) every later kernel derives the same shorter L from that
// count, so that K3 still gets >= TARGET_TASKS chains to fill the chip with.
// (TARGET_TASKS and every other size the host plan shares with these kernels: msm_plan.inc)
__device__ __forceinline__ uint32_t effective_task_len(const uint32_t* __restrict__ pairs, uint32_t L_host) {
  if (pairs == nullptr) return L_host;
  const uint32_t by_fill = pairs[0] / TARGET_TASKS;
  const uint32_t L = L_host < by_fill ? L_host : by_fill;
  return L < 16u ? 16u : L;
}

// Windows [0, n_wide) are c bits wide, the others c - 1 (n_wide = W: every window c bits, the top one implicitly shorter).
// A GROUP of MSMs over the same points (blockIdx.y = the element): element e reads scalars list.s[e] and writes its own
// W x n digit array behind the previous element's (pointer / dword tables of a by-value argument are read with scalar
// loads: graph.hip's note on what must not travel by value does not apply).
struct MsmGroupScalars {
  const uint32_t* s[HM_MSM_GROUP];
};
// One point's W digits: digits[w * n + i] (0 for a base flagged as the identity).  COUNT: each non-zero digit is also
// counted in its window's row of `hist` (LDS, W x NC counters): coarse bin = (|digit| - 1) >> fb, as the first sort level bins it.
template <bool COUNT>
__device__ __forceinline__ void msm_digits_point(const uint4 lo, const uint4 hi, bool skip, int32_t* __restrict__ digits, size_t n,
                                                 size_t i, uint32_t c, uint32_t W, uint32_t n_wide, uint32_t* hist, uint32_t fb,
                                                 uint32_t NC) {
  const uint32_t w_in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  // s_mont * 32 * 2^-261 = s_mont * 2^-256 = the canonical scalar (Fr::to_repr)
  Fr k32 = fe_zero<FrParams>();
  k32.l[0] = 32;
  const Fr s = fe_canonical(fe_mul(fe_unpack<FrParams>(w_in), k32));
  uint32_t v[9];
  {
    uint32_t t[8];
    fe_pack(t, s);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t[k];
    v[8] = 0;
  }
  uint32_t carry = 0;
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t bits = w < n_wide ? c : c - 1;
    const uint32_t mask = (1u << bits) - 1u, half = 1u << (bits - 1);
    uint32_t d = (v[0] & mask) + carry;
    int32_t sd;
    if (d > half) {
      sd = (int32_t)d - (int32_t)(1u << bits);
      carry = 1;
    } else {
      sd = (int32_t)d;
      carry = 0;
    }
    // a narrow window's digit is DOUBLED and its table entry holds half the weight (2^(offset - 1) P): its points then
    // spread over the even buckets of the whole range instead of filling the lower half only (every coarse region of
    // the sort gets the same share: the lower half would hold seven times the upper one at c = 22, W = 12)
    const int32_t out = skip ? 0 : (w < n_wide ? sd : 2 * sd);
    digits[(size_t)w * n + i] = out;
    if constexpr (COUNT) {
      if (out != 0) (void)lds_inc(hist + (size_t)w * NC, ((uint32_t)(out < 0 ? -out : out) - 1u) >> fb);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = __funnelshift_r(v[k], v[k + 1], bits);
  }
}

// COUNT = false: one lane per point (blockIdx.x * blockDim.x + threadIdx.x), nothing but the digits.
// COUNT = true: the first sort level's coarse-bin counts come out of the same pass (a shared bucket set whose first-level
// chunks each lie inside one window: n a multiple of the chunk).  The digit is in a register when it is stored, so the
// histogram pass that would read all W n of them back (msm_part1_hist_kernel) is not launched.  Workgroup pc = blockIdx.x
// takes the points [pc * chunk, + chunk) through ALL windows: W first-level chunks.  It keeps W x NC counters in LDS
// (24 KiB at c = 22: W = 12, NC = 512) and ends by writing its W rows of chist with plain stores, row
// set * G + w * (n / chunk) + pc: exactly what msm_part1_hist_kernel's workgroup (g, set) writes.  No global atomics,
// nothing to zero first.  At 2^24 points that is one workgroup of 1024 lanes per CU; every lane requests its next scalar
// before it works on the current one, which keeps the loads in flight that the short-lived workgroups of the plain form
// get from their number.  The host launches this form only where n is a multiple of the chunk.
template <bool COUNT>
__global__ __launch_bounds__(COUNT ? DIGITS_COUNT_THREADS : DIGITS_THREADS) void msm_digits_kernel(
    MsmGroupScalars list, const uint8_t* __restrict__ inf, int32_t* __restrict__ digits, size_t n, uint32_t c, uint32_t W,
    uint32_t n_wide, uint32_t* __restrict__ chist, size_t chunk, uint32_t G, uint32_t fb, uint32_t NC) {
  const uint32_t* __restrict__ scalars = list.s[blockIdx.y];
  digits += (size_t)blockIdx.y * W * n;
  if constexpr (!COUNT) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(scalars + i * 8);
    msm_digits_point<false>(q[0], q[1], inf[i] != 0, digits, n, i, c, W, n_wide, nullptr, 0, 0);
  } else {
    extern __shared__ uint32_t hist[];
    const uint32_t pc = blockIdx.x;
    for (uint32_t k = threadIdx.x; k < W * NC; k += DIGITS_COUNT_THREADS) hist[k] = 0;
    __syncthreads();
    const size_t lo = (size_t)pc * chunk, hi = lo + chunk < n ? lo + chunk : n;
    size_t i = lo + threadIdx.x;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    bool skip = true;
    if (i < hi) {
      const uint4* q = reinterpret_cast<const uint4*>(scalars + i * 8);
      q0 = q[0];
      q1 = q[1];
      skip = inf[i] != 0;
    }
    while (i < hi) {
      const size_t in = i + DIGITS_COUNT_THREADS;
      uint4 n0 = q0, n1 = q1;
      bool nskip = true;
      if (in < hi) {
        const uint4* q = reinterpret_cast<const uint4*>(scalars + in * 8);
        n0 = q[0];
        n1 = q[1];
        nskip = inf[in] != 0;
      }
      msm_digits_point<true>(q0, q1, skip, digits, n, i, c, W, n_wide, hist, fb, NC);
      q0 = n0;
      q1 = n1;
      skip = nskip;
      i = in;
    }
    __syncthreads();
    const size_t cpw = n / chunk;                              // chunks per window
    for (uint32_t w = 0; w < W; ++w) {
      uint32_t* out = chist + ((size_t)blockIdx.y * G + (size_t)w * cpw + pc) * NC;
      for (uint32_t b = threadIdx.x; b < NC; b += DIGITS_COUNT_THREADS) out[b] = hist[(size_t)w * NC + b];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K2: grouping (bucket, point index) pairs by bucket -- a two-level counting sort through LDS.
//
// A one-level sort (every chunk scattering straight into 2^(c-1) bucket runs) writes each 32-byte
// HBM sector from ~8 different workgroups at different times: 8x write amplification, measured
// (profiles/r01_pmc_traffic.json: 8.2 GiB written for a 1 GiB index array).  Instead:
//   part 1  partition by the HIGH `cb` bits of the bucket: each (chunk, window) workgroup appends
//           its items to 2^cb coarse bins in ~1 KiB runs; an item is ONE 32-bit word
//           [fine bucket bits | sign | point index].
//   part 2  one workgroup per (coarse bin, window) owns a contiguous region of the final array:
//           fine histogram in LDS -> bucket counts; after the global scan it scatters the items of
//           its own region, so every sector is completed by one workgroup while still in L2.
// When fine bits + sign + index bits fit 32 bits with cb = 0 (n <= 2^19) part 1 disappears and
// part 2 reads the digits directly.
// ---------------------------------------------------------------------------------------------

// Apply f(index, word) to base[lo .. hi) with the whole workgroup, 16 bytes per lane per load:
// one 4-byte load in flight per lane keeps only ~1 MB outstanding chip-wide (latency-bound at
// ~0.5 TB/s); four words per load quadruple the bytes in flight.
template <class T, class F>
__device__ __forceinline__ void block_for_each_word(const T* __restrict__ base, size_t lo, size_t hi, F f) {
  size_t a = lo;
  while (a < hi && (reinterpret_cast<uintptr_t>(base + a) & (4 * sizeof(T) - 1))) ++a;   // aligned start
  const size_t nvec = (hi - a) / 4;
  if (threadIdx.x < a - lo) f(lo + threadIdx.x, base[lo + threadIdx.x]);     // <= 3 head words
  const size_t tail = a + nvec * 4;
  if (threadIdx.x < hi - tail) f(tail + threadIdx.x, base[tail + threadIdx.x]);   // <= 3 tail words
  typedef T vec4 __attribute__((ext_vector_type(4)));
  const vec4* vb = reinterpret_cast<const vec4*>(base + a);
  for (size_t v = threadIdx.x; v < nvec; v += SORT_THREADS) {
    const vec4 q = vb[v];
    const size_t i = a + v * 4;
    f(i, q.x);
    f(i + 1, q.y);
    f(i + 2, q.z);
    f(i + 3, q.w);
  }
}

__global__ __launch_bounds__(SORT_THREADS) void msm_part1_hist_kernel(const int32_t* __restrict__ digits,
                                                                      uint32_t* __restrict__ chist, size_t n, size_t chunk,
                                                                      uint32_t fb, uint32_t NC) {
  extern __shared__ uint32_t hist[];
  const uint32_t g = blockIdx.x, w = blockIdx.y, G = gridDim.x;
  for (uint32_t b = threadIdx.x; b < NC; b += SORT_THREADS) hist[b] = 0;
  __syncthreads();
  const size_t lo = (size_t)g * chunk, hi = lo + chunk < n ? lo + chunk : n;
  const int32_t* dw = digits + (size_t)w * n;
  block_for_each_word(dw, lo, hi, [&](size_t, int32_t d) {
    if (d != 0) (void)lds_inc(hist, ((uint32_t)(d < 0 ? -d : d) - 1u) >> fb);
  });
  __syncthreads();
  uint32_t* out = chist + ((size_t)w * G + g) * NC;
  for (uint32_t b = threadIdx.x; b < NC; b += SORT_THREADS) out[b] = hist[b];
}

// per (window, coarse bin): exclusive prefix over chunks in place, total into ctot.
// One 64-lane workgroup per (window, bin): lanes take contiguous runs of chunks, then a wave scan.
__global__ __launch_bounds__(64) void msm_part1_scan_kernel(uint32_t* __restrict__ chist, uint32_t* __restrict__ ctot, uint32_t G,
                                                            uint32_t NC, uint32_t W) {
  const uint32_t idx = blockIdx.x;
  if (idx >= W * NC) return;
  const uint32_t w = idx / NC, b = idx - w * NC;
  const uint32_t lane = threadIdx.x;
  const uint32_t per = (G + 63) / 64;
  const uint32_t lo = lane * per, hi = lo + per < G ? lo + per : G;
  uint32_t sum = 0;
  for (uint32_t g = lo; g < hi; ++g) sum += chist[((size_t)w * G + g) * NC + b];
  uint32_t incl = sum;                       // inclusive scan across the 64 lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off, 64);
    if (lane >= (uint32_t)off) incl += v;
  }
  uint32_t run = incl - sum;
  for (uint32_t g = lo; g < hi; ++g) {
    uint32_t* p = chist + ((size_t)w * G + g) * NC + b;
    const uint32_t t = *p;
    *p = run;
    run += t;
  }
  if (lane == 63) ctot[idx] = incl;
}

// one block: cstart = exclusive scan of ctot (count <= 16 * 1024 + 1 entries; cstart[count] = total)
__global__ __launch_bounds__(1024) void msm_part1_starts_kernel(const uint32_t* __restrict__ ctot,
                                                                uint32_t* __restrict__ cstart, uint32_t count) {
  __shared__ uint32_t s[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (count + 1023) / 1024;
  const uint32_t lo = t * per, hi = lo + per < count ? lo + per : count;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += ctot[i];
  s[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    uint32_t a = 0;
    if (t >= off) a = s[t - off];
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  uint32_t run = s[t] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    cstart[i] = run;
    run += ctot[i];
  }
  if (t == 1023) cstart[count] = s[1023];
}

// ITEM = uint32_t when [fine bits | sign | index] fits 32 bits, else uint64_t
template <class ITEM>
__global__ __launch_bounds__(SORT_THREADS) void msm_part1_scatter_kernel(const int32_t* __restrict__ digits,
                                                                         const uint32_t* __restrict__ chist,
                                                                         const uint32_t* __restrict__ cstart,
                                                                         ITEM* __restrict__ tmp, size_t n, size_t chunk,
                                                                         uint32_t fb, uint32_t ib, uint32_t NC) {
  extern __shared__ uint32_t cursor[];
  const uint32_t g = blockIdx.x, w = blockIdx.y, G = gridDim.x;
  const uint32_t* pre = chist + ((size_t)w * G + g) * NC;
  const uint32_t* cs = cstart + (size_t)w * NC;
  for (uint32_t b = threadIdx.x; b < NC; b += SORT_THREADS) cursor[b] = cs[b] + pre[b];
  __syncthreads();
  const size_t lo = (size_t)g * chunk, hi = lo + chunk < n ? lo + chunk : n;
  const int32_t* dw = digits + (size_t)w * n;
  const uint32_t fmask = (1u << fb) - 1u;
  const ITEM imask = ((ITEM)1 << ib) - 1;     // positional items keep only the low ib bits of the index (see msm_issue)
  block_for_each_word(dw, lo, hi, [&](size_t i, int32_t d) {
    if (d != 0) {
      const uint32_t b1 = (uint32_t)(d < 0 ? -d : d) - 1u;
      const uint32_t pos = lds_inc(cursor, b1 >> fb);
      tmp[pos] = ((ITEM)(b1 & fmask) << (ib + 1)) | ((ITEM)(d < 0 ? 1u : 0u) << ib) | ((ITEM)i & imask);
    }
  });
}

// part 1 scatter, tiled form: the chunk is processed in tiles of 4096 digits that are first
// counting-sorted by coarse bin inside LDS, so that consecutive lanes append to the same coarse run
// (sector-complete stores, as in the tiled part-2 scatter below).  Used while NC <= 4096, for 64-bit items only: 32-bit items
// take the vector-load form (msm_part1_scatter_v2_kernel), which alone has the big tiles of P1_BIG_IPT items per lane.
// P1_IPT items per lane and tile: a tile should bring >= 8 items (one 32-byte sector) to every coarse bin
template <class ITEM>
__global__ __launch_bounds__(SORT_THREADS) void msm_part1_scatter_tiled_kernel(const int32_t* __restrict__ digits,
                                                                               const uint32_t* __restrict__ chist,
                                                                               const uint32_t* __restrict__ cstart,
                                                                               ITEM* __restrict__ tmp, size_t n, size_t chunk,
                                                                               uint32_t fb, uint32_t ib, uint32_t NC) {
  static_assert(sizeof(ITEM) == 8, "no plan selects the tiled first-level scatter for 32-bit items");
  extern __shared__ uint32_t sm[];
  constexpr int P1_IPT = P1_IPT_DEFAULT;
  constexpr int P1_TILE = SORT_THREADS * P1_IPT;
  const uint32_t g = blockIdx.x, w = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  uint32_t* gcur = sm;                 // global cursor of every coarse bin for this chunk
  uint32_t* tcnt = gcur + NC;
  uint32_t* tstart = tcnt + NC;
  uint32_t* wsum = tstart + NC;
  uint32_t* st_bin = wsum + 32;
  ITEM* st_item = reinterpret_cast<ITEM*>(st_bin + P1_TILE);
  const uint32_t* pre = chist + ((size_t)w * G + g) * NC;
  const uint32_t* cs = cstart + (size_t)w * NC;
  for (uint32_t b = tid; b < NC; b += SORT_THREADS) { gcur[b] = cs[b] + pre[b]; tcnt[b] = 0; }
  __syncthreads();
  const size_t lo = (size_t)g * chunk, hi = lo + chunk < n ? lo + chunk : n;
  const int32_t* dw = digits + (size_t)w * n;
  const uint32_t fmask = (1u << fb) - 1u;
  const ITEM imask = ((ITEM)1 << ib) - 1;
  const uint32_t per = (NC + SORT_THREADS - 1) / SORT_THREADS;
  for (size_t t0 = lo; t0 < hi; t0 += P1_TILE) {
    const uint32_t tile_n = hi - t0 < (size_t)P1_TILE ? (uint32_t)(hi - t0) : (uint32_t)P1_TILE;
    ITEM item[P1_IPT];
    uint32_t bin[P1_IPT], rank[P1_IPT];
#pragma unroll
    for (int k = 0; k < P1_IPT; ++k) {
      const uint32_t e = (uint32_t)k * SORT_THREADS + tid;
      bin[k] = 0xffffffffu;
      if (e < tile_n) {
        const int32_t d = dw[t0 + e];
        if (d != 0) {
          const uint32_t b1 = (uint32_t)(d < 0 ? -d : d) - 1u;
          bin[k] = b1 >> fb;
          item[k] = ((ITEM)(b1 & fmask) << (ib + 1)) | ((ITEM)(d < 0 ? 1u : 0u) << ib) | ((ITEM)(t0 + e) & imask);
          rank[k] = lds_inc(tcnt, bin[k]);
        }
      }
    }
    __syncthreads();
    {   // exclusive scan of tcnt[0 .. NC)
      const uint32_t b0 = tid * per;
      uint32_t v[4096 / SORT_THREADS] = {}, sum = 0;
      for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < NC) { v[k] = tcnt[b0 + k]; sum += v[k]; }
      uint32_t incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off, 64);
        if ((tid & 63) >= (uint32_t)off) incl += u;
      }
      if ((tid & 63) == 63) wsum[tid >> 6] = incl;
      __syncthreads();
      if (tid < 64) {
        const uint32_t ws = tid < (SORT_THREADS / 64) ? wsum[tid] : 0;
        uint32_t wi = ws;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t u = __shfl_up(wi, off, 64);
          if (tid >= (uint32_t)off) wi += u;
        }
        if (tid < (SORT_THREADS / 64)) wsum[tid] = wi - ws;
      }
      __syncthreads();
      uint32_t run = wsum[tid >> 6] + incl - sum;
      for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < NC) { tstart[b0 + k] = run; run += v[k]; }
    }
    __syncthreads();
    uint32_t kept = 0;
#pragma unroll
    for (int k = 0; k < P1_IPT; ++k) {
      if (bin[k] != 0xffffffffu) {
        const uint32_t pos = tstart[bin[k]] + rank[k];
        st_item[pos] = item[k];
        st_bin[pos] = bin[k];
      }
    }
    __syncthreads();
    kept = tstart[NC - 1] + tcnt[NC - 1];      // non-zero digits of this tile
    for (uint32_t e = tid; e < kept; e += SORT_THREADS) {
      const uint32_t b = st_bin[e];
      tmp[gcur[b] + (e - tstart[b])] = st_item[e];
    }
    __syncthreads();
    for (uint32_t b = tid; b < NC; b += SORT_THREADS) { gcur[b] += tcnt[b]; tcnt[b] = 0; }
    __syncthreads();
  }
}

// part 2, first half: fine histogram of one (coarse bin, window) region -> bucket counts.
// FROM_DIGITS (cb = 0): the "region" is the whole window and items are read from the digit array.
// Regions larger than `big` items (a hot bucket: constant or flag columns send a whole window to one
// region) are left to the COOP instantiation, which many workgroups run on slices of such a region
// (work list built by msm_big_regions_kernel) and which ADDS its counts to bcnt with global atomics.
template <bool FROM_DIGITS, class ITEM, bool COOP = false>
__global__ __launch_bounds__(SORT_THREADS) void msm_part2_hist_kernel(const ITEM* __restrict__ tmp,
                                                                      const int32_t* __restrict__ digits,
                                                                      const uint32_t* __restrict__ cstart,
                                                                      uint32_t* __restrict__ bcnt, size_t n, uint32_t fb,
                                                                      uint32_t ib, uint32_t NC, uint32_t NBP, uint32_t big,
                                                                      uint32_t slice, const uint2* __restrict__ list,
                                                                      const uint32_t* __restrict__ list_count) {
  extern __shared__ uint32_t fine[];
  uint32_t hb = blockIdx.x, w = blockIdx.y, sl = 0;
  if (COOP) {
    if (blockIdx.x >= *list_count) return;
    const uint2 it = list[blockIdx.x];
    w = it.x / NC;
    hb = it.x - w * NC;
    sl = it.y;
  }
  const uint32_t NF = 1u << fb;
  if (!FROM_DIGITS && !COOP && cstart[w * NC + hb + 1] - cstart[w * NC + hb] > big) return;   // bcnt was zeroed
  for (uint32_t b = threadIdx.x; b < NF; b += SORT_THREADS) fine[b] = 0;
  __syncthreads();
  if (FROM_DIGITS) {
    const int32_t* dw = digits + (size_t)w * n;
    block_for_each_word(dw, 0, n, [&](size_t, int32_t d) {
      if (d != 0) (void)lds_inc(fine, (uint32_t)(d < 0 ? -d : d) - 1u);
    });
  } else {
    uint32_t lo = cstart[w * NC + hb], hi = cstart[w * NC + hb + 1];
    if (COOP) {
      lo += sl * slice;
      hi = lo + slice < hi ? lo + slice : hi;
    }
    block_for_each_word(tmp, lo, hi, [&](size_t, ITEM item) { (void)lds_inc(fine, (uint32_t)(item >> (ib + 1))); });
  }
  __syncthreads();
  uint32_t* out = bcnt + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  if (COOP) {
    for (uint32_t b = threadIdx.x; b < NF; b += SORT_THREADS)
      if (fine[b]) atomicAdd(&out[b], fine[b]);
  } else {
    for (uint32_t b = threadIdx.x; b < NF; b += SORT_THREADS) out[b] = fine[b];
    if (hb == 0 && threadIdx.x == 0) bcnt[(size_t)w * NBP] = 0;   // bucket 0 (digit 0) is never used
  }
}

// work list of (region, slice) pairs for regions with more than `big` items
__global__ void msm_big_regions_kernel(const uint32_t* __restrict__ cstart, uint32_t nregions, uint32_t big, uint32_t slice,
                                       uint2* __restrict__ list, uint32_t* __restrict__ list_count, uint32_t capacity) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nregions) return;
  const uint32_t size = cstart[r + 1] - cstart[r];
  if (size <= big) return;
  const uint32_t nsl = (size + slice - 1) / slice;
  const uint32_t at = atomicAdd(list_count, nsl);
  for (uint32_t i = 0; i < nsl && at + i < capacity; ++i) list[at + i] = make_uint2(r, i);
}

// part 2, second half: scatter the region's items to their final places (boff = global bucket offsets)
template <bool FROM_DIGITS, class ITEM>
__global__ __launch_bounds__(SORT_THREADS) void msm_part2_scatter_kernel(const ITEM* __restrict__ tmp,
                                                                         const int32_t* __restrict__ digits,
                                                                         const uint32_t* __restrict__ cstart,
                                                                         const uint32_t* __restrict__ boff,
                                                                         uint32_t* __restrict__ sorted, size_t n, uint32_t fb,
                                                                         uint32_t ib, uint32_t NC, uint32_t NBP) {
  extern __shared__ uint32_t cursor[];
  const uint32_t hb = blockIdx.x, w = blockIdx.y;
  const uint32_t NF = 1u << fb;
  const uint32_t* bo = boff + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  for (uint32_t b = threadIdx.x; b < NF; b += SORT_THREADS) cursor[b] = bo[b];
  __syncthreads();
  if (FROM_DIGITS) {
    const int32_t* dw = digits + (size_t)w * n;
    block_for_each_word(dw, 0, n, [&](size_t i, int32_t d) {
      if (d != 0) {
        const uint32_t pos = lds_inc(cursor, (uint32_t)(d < 0 ? -d : d) - 1u);
        sorted[pos] = (uint32_t)i | (d < 0 ? 0x80000000u : 0u);
      }
    });
  } else {
    const uint32_t lo = cstart[w * NC + hb], hi = cstart[w * NC + hb + 1];
    const ITEM imask = ((ITEM)1 << ib) - 1;
    block_for_each_word(tmp, lo, hi, [&](size_t, ITEM item) {
      const uint32_t pos = lds_inc(cursor, (uint32_t)(item >> (ib + 1)));
      sorted[pos] = (uint32_t)(item & imask) | ((uint32_t)((item >> ib) & 1) << 31);
    });
  }
}

// part 2, second half, tiled form (regions read from tmp): the region is processed in tiles of
// 4096 items that are first counting-sorted by fine bucket inside LDS, so that consecutive lanes write
// consecutive addresses of a bucket run -- every 32-byte sector of the final array is written by one
// wave instruction (or two adjacent tiles) instead of by eight separate 4-byte stores spread over the
// workgroup's lifetime, which is what kept missing L2 once a region had more than ~128 runs.
// LDS of the tiled and vector-load kernels at their largest plans (part 2: fb = 12; part 1's big tiles: 2 048 coarse bins, 4-byte items):
// gfx950 has 160 KiB per workgroup
static_assert(((size_t)3 * 4096 + 32 + P2_TILE) * 4 + (size_t)P2_TILE * 2 <= 160 * 1024, "part-2 tile does not fit the LDS");
static_assert(((size_t)3 * 2048 + 32 + SORT_THREADS * P1_BIG_IPT) * 4 + (size_t)SORT_THREADS * P1_BIG_IPT * 4 <= 160 * 1024,
              "part-1 big tile does not fit the LDS");
// COOP: slices of big regions (work list); the per-bucket cursors then live in global memory
// (`gcursor`, a copy of boff) and every tile reserves its runs with one atomicAdd per non-empty bucket.
// POSITIONAL (a shared bucket set of n * W > 2^27 items: fine bits + sign + a 28-bit index do not fit one word): an
// item carries only the low `ib` bits of its index.  The rest is its SUPER-CHUNK, 2^ib consecutive indices = `gpc`
// chunks of the first sort level, and the first level lays the runs of a coarse bin down in chunk order -- so the
// super-chunk of an item follows from its POSITION in the region: the boundaries are the (already scanned) per-chunk
// offsets chist[g * NC + bin] at g = 0, gpc, 2 gpc, ...  They go to LDS (at most PS_MAX_SC + 1 words) and every item
// finds its piece by a binary search.  Half the bytes of the 64-bit items this replaces, at every level of the sort.
// Positional items are 32-bit: msm_part2_scatter_v2_kernel places them; the tiled kernel below serves 64-bit items, which carry
// their whole index.
struct Positional {
  const uint32_t* chist;    // scanned per-chunk offsets: [set][g][NC] (a shared bucket set is one "window"; a group of MSMs has one set each)
  uint32_t G, gpc, nsc;     // chunks, chunks per super-chunk, super-chunks (0: items carry their whole index)
};
template <class ITEM, bool COOP = false>
__global__ __launch_bounds__(SORT_THREADS) void msm_part2_scatter_tiled_kernel(const ITEM* __restrict__ tmp,
                                                                               const uint32_t* __restrict__ cstart,
                                                                               const uint32_t* __restrict__ boff,
                                                                               uint32_t* __restrict__ sorted, uint32_t fb,
                                                                               uint32_t ib, uint32_t NC, uint32_t NBP, uint32_t big,
                                                                               uint32_t slice, const uint2* __restrict__ list,
                                                                               const uint32_t* __restrict__ list_count,
                                                                               uint32_t* __restrict__ gcursor) {
  static_assert(sizeof(ITEM) == 8, "no plan selects the tiled second-level scatter for 32-bit items");
  extern __shared__ uint32_t sm[];
  uint32_t hb = blockIdx.x, w = blockIdx.y, sl = 0;
  const uint32_t tid = threadIdx.x;
  if (COOP) {
    if (blockIdx.x >= *list_count) return;
    const uint2 it = list[blockIdx.x];
    w = it.x / NC;
    hb = it.x - w * NC;
    sl = it.y;
  } else if (cstart[w * NC + hb + 1] - cstart[w * NC + hb] > big) {
    return;
  }
  const uint32_t NF = 1u << fb;                       // <= 4096
  uint32_t* gcur = sm;                                // global cursor of every fine bucket
  uint32_t* tcnt = gcur + NF;                         // items of the current tile per bucket
  uint32_t* tstart = tcnt + NF;                       // exclusive prefix of tcnt
  uint32_t* wsum = tstart + NF;                       // 32 wave totals of the scan
  uint32_t* st_pay = wsum + 32;                       // tile items in bucket order
  uint16_t* st_bin = reinterpret_cast<uint16_t*>(st_pay + P2_TILE);   // their fine buckets (< 2^12)
  const uint32_t* bo = boff + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  uint32_t* gc = gcursor + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  for (uint32_t b = tid; b < NF; b += SORT_THREADS) { gcur[b] = bo[b]; tcnt[b] = 0; }
  __syncthreads();
  uint32_t lo = cstart[w * NC + hb], hi = cstart[w * NC + hb + 1];
  if (COOP) {
    lo += sl * slice;
    hi = lo + slice < hi ? lo + slice : hi;
  }
  const ITEM imask = ((ITEM)1 << ib) - 1;
  const uint32_t per = (NF + SORT_THREADS - 1) / SORT_THREADS;   // scan entries per lane (1 .. 4)
  for (uint32_t t0 = lo; t0 < hi; t0 += P2_TILE) {
    const uint32_t tile_n = hi - t0 < (uint32_t)P2_TILE ? hi - t0 : (uint32_t)P2_TILE;
    uint32_t pay[P2_IPT], bin[P2_IPT], rank[P2_IPT];
#pragma unroll
    for (int k = 0; k < P2_IPT; ++k) {
      const uint32_t e = (uint32_t)k * SORT_THREADS + tid;
      if (e < tile_n) {
        const ITEM item = tmp[t0 + e];
        bin[k] = (uint32_t)(item >> (ib + 1));
        pay[k] = (uint32_t)(item & imask) | ((uint32_t)((item >> ib) & 1) << 31);
        rank[k] = lds_inc(tcnt, bin[k]);
      }
    }
    __syncthreads();
    // exclusive scan of tcnt[0 .. NF): lane-serial over `per` entries, wave scan, then wave totals
    {
      const uint32_t b0 = tid * per;
      uint32_t v[4096 / SORT_THREADS] = {}, sum = 0;
      for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < NF) { v[k] = tcnt[b0 + k]; sum += v[k]; }
      uint32_t incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off, 64);
        if ((tid & 63) >= (uint32_t)off) incl += u;
      }
      if ((tid & 63) == 63) wsum[tid >> 6] = incl;
      __syncthreads();
      if (tid < 64) {
        const uint32_t ws = tid < (SORT_THREADS / 64) ? wsum[tid] : 0;
        uint32_t wi = ws;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t u = __shfl_up(wi, off, 64);
          if (tid >= (uint32_t)off) wi += u;
        }
        if (tid < (SORT_THREADS / 64)) wsum[tid] = wi - ws;   // exclusive wave offsets
      }
      __syncthreads();
      uint32_t run = wsum[tid >> 6] + incl - sum;
      for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < NF) { tstart[b0 + k] = run; run += v[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P2_IPT; ++k) {
      const uint32_t e = (uint32_t)k * SORT_THREADS + tid;
      if (e < tile_n) {
        const uint32_t pos = tstart[bin[k]] + rank[k];
        st_pay[pos] = pay[k];
        st_bin[pos] = (uint16_t)bin[k];
      }
    }
    if (COOP)      // reserve this tile's run in every non-empty bucket
      for (uint32_t b = tid; b < NF; b += SORT_THREADS)
        if (tcnt[b]) gcur[b] = atomicAdd(&gc[b], tcnt[b]);
    __syncthreads();
    for (uint32_t e = tid; e < tile_n; e += SORT_THREADS) {
      const uint32_t b = st_bin[e];
      sorted[gcur[b] + (e - tstart[b])] = st_pay[e];
    }
    __syncthreads();
    for (uint32_t b = tid; b < NF; b += SORT_THREADS) {
      if (!COOP) gcur[b] += tcnt[b];
      tcnt[b] = 0;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// The tiled scatters, second form ("v2", 32-bit items; round 4).  SQ counters on the kernels above at 2^24 on the table
// (profiles/r04_b_side_measurements.txt) showed both of them bound by instruction issue and latency, not by HBM: 2.3
// wave-instructions per item (147 lane-instructions), and in the ISA every one of a lane's 16 loads of a tile sits in its
// own branch region behind its own `s_waitcnt vmcnt(0)` -- sixteen serial HBM round trips per tile (a tile took 32 us) --
// and the positional walk is a divergent loop of dependent LDS reads per item.  Here a lane takes FOUR consecutive items
// per 16-byte load, all loads of a tile are issued before anything waits, the super-chunk of an item comes from a per-tile
// table (one entry per 64 positions, filled by a few lanes while the loads are in flight) plus a compare against the next
// boundary, and the wave-uniformity test that guards the LDS counters is made once per four items.
// ---------------------------------------------------------------------------------------------
// A workgroup barrier that orders LDS accesses only: __syncthreads() also waits for every outstanding global access
// (s_waitcnt vmcnt(0)), which would drain a tile's scattered stores -- and the next tile's prefetched loads -- at each of
// the six barriers of a tile.  The v2 scatters never read back what they store to global memory.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Exclusive scan of cnt[0 .. NB) (NB <= 4096) into start[], by the whole workgroup; returns the total to every lane.
// Three barriers; cnt is left untouched.
__device__ __forceinline__ uint32_t tile_exclusive_scan(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ start,
                                                        uint32_t* __restrict__ wsum, uint32_t NB, uint32_t tid) {
  const uint32_t per = (NB + SORT_THREADS - 1) / SORT_THREADS, b0 = tid * per;
  uint32_t v[4096 / SORT_THREADS] = {}, sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4096 / SORT_THREADS; ++k)
    if (k < per && b0 + k < NB) { v[k] = cnt[b0 + k]; sum += v[k]; }
  uint32_t incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(incl, off, 64);
    if ((tid & 63) >= (uint32_t)off) incl += u;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  lds_barrier();
  if (tid < 64) {
    const uint32_t ws = tid < (SORT_THREADS / 64) ? wsum[tid] : 0;
    uint32_t wi = ws;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(wi, off, 64);
      if (tid >= (uint32_t)off) wi += u;
    }
    if (tid < (SORT_THREADS / 64)) wsum[tid] = wi - ws;   // exclusive wave offsets
    if (tid == SORT_THREADS / 64 - 1) wsum[SORT_THREADS / 64] = wi;   // the total
  }
  lds_barrier();
  uint32_t run = wsum[tid >> 6] + incl - sum;
#pragma unroll
  for (uint32_t k = 0; k < 4096 / SORT_THREADS; ++k)
    if (k < per && b0 + k < NB) { start[b0 + k] = run; run += v[k]; }
  const uint32_t total = wsum[SORT_THREADS / 64];
  lds_barrier();
  return total;
}

// rank[k] = cnt[bin[k]]++ for the valid ones of a lane's four items (FULL: all four are).  When every item of the WAVE
// goes to one counter (constant and flag columns: lds_inc's reason) one lane adds for all of them.  Called with the whole
// wave converged.
template <bool FULL>
__device__ __forceinline__ void lds_rank4(uint32_t* cnt, const uint32_t bin[4], uint32_t valid_mask, uint32_t rank[4]) {
  if (FULL) valid_mask = 0xfu;
  const uint64_t active = FULL ? ~0ull : __ballot(valid_mask != 0);
  if (!FULL && active == 0) return;                            // wave-uniform
  uint32_t mine = bin[0];
  if (!FULL) {
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if (valid_mask & (1u << k)) mine = bin[k];               // a valid bin of this lane (its first)
  }
  const uint32_t v = FULL ? (uint32_t)__builtin_amdgcn_readfirstlane((int)mine)
                          : (uint32_t)__builtin_amdgcn_readlane((int)mine, __builtin_ctzll(active));
  bool same = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) same = same && (!(valid_mask & (1u << k)) || bin[k] == v);
  if (__ballot(same) == ~0ull) {                               // every valid item of the wave wants counter v
    const uint32_t mycount = (uint32_t)__popc(valid_mask);
    uint32_t incl = mycount;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off, 64);
      if ((threadIdx.x & 63) >= (uint32_t)off) incl += u;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(&cnt[v], total);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    uint32_t r = base + incl - mycount;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (valid_mask & (1u << k)) rank[k] = r++;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (FULL || (valid_mask & (1u << k))) rank[k] = atomicAdd(&cnt[bin[k]], 1u);
}

// One tile of the first-level scatter.  FULL: every position of the tile is a digit of the chunk (all but the first and
// last tile of a chunk): no masks, no predication.  `base + r` is digit lo + r - mis.
template <int IPT>
__device__ __forceinline__ void p1v2_load(const int32_t* __restrict__ base, uint32_t rb, uint32_t end, uint32_t tid, int4 (&q)[IPT / 4]) {
#pragma unroll
  for (int j = 0; j < IPT / 4; ++j) {
    const uint32_t r = rb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    q[j] = *reinterpret_cast<const int4*>(base + (r < end ? r : 0u));      // (a vector past the end reads the first one again)
  }
}
template <int IPT, bool FULL>
__device__ __forceinline__ void p1v2_tile(const int4 (&q)[IPT / 4], uint32_t rb, uint32_t mis, uint32_t end, uint32_t lo32,
                                          uint32_t fb, uint32_t ib, uint32_t NC, uint32_t* __restrict__ tmp, uint32_t* gcur, uint32_t* tcnt,
                                          uint32_t* tstart, uint32_t* wsum, uint32_t* st_bin, uint32_t* st_item, uint32_t tid) {
  constexpr int NV = IPT / 4;
  const uint32_t fmask = (1u << fb) - 1u, imask = (1u << ib) - 1u;
  uint32_t rank[IPT], vmask[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t r = rb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    const int32_t d4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
    uint32_t m = 0, bin[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int32_t d = d4[c];
      const bool ok = (FULL || (r + c >= mis && r + c < end)) && d != 0;      // zero digits are not items
      bin[c] = ((uint32_t)(d < 0 ? -d : d) - 1u) >> fb;
      m |= ok ? 1u << c : 0u;
    }
    vmask[j] = m;
    if (__ballot(m != 0xfu) == 0) lds_rank4<true>(tcnt, bin, m, &rank[4 * j]);     // no zero digit in the wave's 256: the usual case
    else lds_rank4<false>(tcnt, bin, m, &rank[4 * j]);
  }
  lds_barrier();
  const uint32_t kept = tile_exclusive_scan(tcnt, tstart, wsum, NC, tid);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t r = rb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    const int32_t d4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (vmask[j] & (1u << c)) {
        const int32_t d = d4[c];
        const uint32_t b1 = (uint32_t)(d < 0 ? -d : d) - 1u, bin = b1 >> fb;
        const uint32_t pos = lo32 + (r + c - mis);                              // the item's index in its bucket set (low `ib` bits kept)
        const uint32_t dst = tstart[bin] + rank[4 * j + c];
        st_item[dst] = ((b1 & fmask) << (ib + 1)) | ((d < 0 ? 1u : 0u) << ib) | (pos & imask);
        st_bin[dst] = bin;
      }
  }
  lds_barrier();
  if (kept == (uint32_t)(SORT_THREADS * IPT)) {
#pragma unroll 4
    for (int k = 0; k < IPT; ++k) {
      const uint32_t e = (uint32_t)k * SORT_THREADS + tid, b = st_bin[e];
      tmp[gcur[b] + (e - tstart[b])] = st_item[e];
    }
  } else {
    for (uint32_t e = tid; e < kept; e += SORT_THREADS) {
      const uint32_t b = st_bin[e];
      tmp[gcur[b] + (e - tstart[b])] = st_item[e];
    }
  }
  lds_barrier();
  for (uint32_t b = tid; b < NC; b += SORT_THREADS) { gcur[b] += tcnt[b]; tcnt[b] = 0; }
  lds_barrier();
}

template <int IPT>
__global__ __launch_bounds__(SORT_THREADS) void msm_part1_scatter_v2_kernel(const int32_t* __restrict__ digits,
                                                                            const uint32_t* __restrict__ chist,
                                                                            const uint32_t* __restrict__ cstart,
                                                                            uint32_t* __restrict__ tmp, size_t n, size_t chunk,
                                                                            uint32_t fb, uint32_t ib, uint32_t NC) {
  extern __shared__ uint32_t sm[];
  constexpr uint32_t TILE = SORT_THREADS * IPT;
  const uint32_t g = blockIdx.x, w = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  uint32_t* gcur = sm;                 // global cursor of every coarse bin for this chunk
  uint32_t* tcnt = gcur + NC;
  uint32_t* tstart = tcnt + NC;
  uint32_t* wsum = tstart + NC;        // 32 words
  uint32_t* st_bin = wsum + 32;
  uint32_t* st_item = st_bin + TILE;
  const uint32_t* pre = chist + ((size_t)w * G + g) * NC;
  const uint32_t* cs = cstart + (size_t)w * NC;
  for (uint32_t b = tid; b < NC; b += SORT_THREADS) { gcur[b] = cs[b] + pre[b]; tcnt[b] = 0; }
  lds_barrier();
  const size_t lo = (size_t)g * chunk, hi = lo + chunk < n ? lo + chunk : n;
  if (lo >= hi) return;
  // tiles start where the ADDRESS is 16-byte aligned: `mis` <= 3 positions before lo (masked off; for w > 0 they are the
  // previous window's last digits, for w = 0 the array is 256-byte aligned and mis = lo & 3).  Positions are counted from
  // that address: r in [mis, mis + len) is digit lo + r - mis.
  const int32_t* dw = digits + (size_t)w * n + lo;
  const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(dw) >> 2) & 3);
  const int32_t* base = dw - mis;
  const uint32_t end = mis + (uint32_t)(hi - lo);              // chunks are far below 2^32 items
  int4 q[IPT / 4], qn[IPT / 4];
  p1v2_load<IPT>(base, 0, end, tid, q);
  for (uint32_t rb = 0; rb < end; rb += TILE) {
    const bool more = rb + TILE < end;
    if (more) p1v2_load<IPT>(base, rb + TILE, end, tid, qn);     // the next tile's digits travel while this one is ranked and staged
    if (rb >= mis && rb + TILE <= end)
      p1v2_tile<IPT, true>(q, rb, mis, end, (uint32_t)lo, fb, ib, NC, tmp, gcur, tcnt, tstart, wsum, st_bin, st_item, tid);
    else
      p1v2_tile<IPT, false>(q, rb, mis, end, (uint32_t)lo, fb, ib, NC, tmp, gcur, tcnt, tstart, wsum, st_bin, st_item, tid);
    if (more) {
#pragma unroll
      for (int j = 0; j < IPT / 4; ++j) q[j] = qn[j];
    }
  }
}

__device__ __forceinline__ uint32_t dst_of(const uint32_t* tstart, uint32_t bin, uint32_t rank) { return tstart[bin] + rank; }

// One tile of the second-level scatter.  FULL: every position of the tile is an item of the region / slice.
__device__ __forceinline__ void p2v2_load(const uint32_t* __restrict__ tmp, uint32_t tb, uint32_t lo, uint32_t hi, uint32_t tid,
                                          uint4 (&q)[P2_IPT / 4]) {
#pragma unroll
  for (int j = 0; j < P2_IPT / 4; ++j) {
    const uint32_t p = tb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    q[j] = *reinterpret_cast<const uint4*>(tmp + (p < hi ? p : (lo & ~3u)));
  }
}
template <bool COOP, bool FULL>
__device__ __forceinline__ void p2v2_tile(const uint4 (&q)[P2_IPT / 4], uint32_t* __restrict__ sorted, uint32_t tb, uint32_t lo,
                                          uint32_t hi, uint32_t region_lo, uint32_t ib, uint32_t NF, const Positional& ps, uint32_t* gcur,
                                          uint32_t* tcnt, uint32_t* tstart, uint32_t* wsum, uint32_t* st_pay, uint16_t* st_bin,
                                          const uint32_t* sc_start, uint32_t* tile_sc, uint32_t* __restrict__ gc, uint32_t tid) {
  constexpr int NV = P2_IPT / 4;
  const uint32_t imask = (1u << ib) - 1u;
  if (ps.nsc && tid < P2_TILE / 64) {                  // while the loads are in flight: the largest sc with sc_start[sc] <= position
    const uint32_t p0 = tb + 64u * tid;
    const uint32_t rel = p0 > region_lo ? p0 - region_lo : 0u;
    uint32_t a = 0, b = ps.nsc;                        // invariant: sc_start[a] <= rel (sc_start[0] = 0), and rel < sc_start[b] or b = nsc
    while (b - a > 1) {
      const uint32_t m = (a + b) >> 1;
      if (sc_start[m] <= rel) a = m; else b = m;
    }
    tile_sc[tid] = a;
  }
  uint32_t rank[P2_IPT], vmask[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t p = tb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    const uint32_t i4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
    uint32_t m = 0, bin[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bin[c] = i4[c] >> (ib + 1);
      m |= (FULL || (p + c >= lo && p + c < hi)) ? 1u << c : 0u;
    }
    vmask[j] = m;
    lds_rank4<FULL>(tcnt, bin, m, &rank[4 * j]);
  }
  lds_barrier();
  const uint32_t kept = tile_exclusive_scan(tcnt, tstart, wsum, NF, tid);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t p = tb + 4u * ((uint32_t)j * SORT_THREADS + tid);
    const uint32_t i4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
    uint32_t a = 0, nb = 0xffffffffu;
    if (ps.nsc && (FULL || vmask[j])) {                // super-chunk of the vector's first position: the tile table, then a short walk
      const uint32_t rel = (p > region_lo ? p - region_lo : 0u);
      a = tile_sc[(p - tb) >> 6];
      while (sc_start[a + 1] <= rel && a + 1 < ps.nsc) ++a;
      nb = sc_start[a + 1];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (FULL || (vmask[j] & (1u << c))) {
        uint32_t pay = (i4[c] & imask) | (((i4[c] >> ib) & 1u) << 31);
        if (ps.nsc) {
          const uint32_t rel = p + c - region_lo;
          while (nb <= rel && a + 1 < ps.nsc) { ++a; nb = sc_start[a + 1]; }   // almost never: runs are ~2 000 items long
          pay |= a << ib;
        }
        const uint32_t bin = i4[c] >> (ib + 1);
        st_pay[dst_of(tstart, bin, rank[4 * j + c])] = pay;
        st_bin[dst_of(tstart, bin, rank[4 * j + c])] = (uint16_t)bin;
      }
  }
  if (COOP)      // reserve this tile's run in every non-empty bucket
    for (uint32_t b = tid; b < NF; b += SORT_THREADS)
      if (tcnt[b]) gcur[b] = atomicAdd(&gc[b], tcnt[b]);
  lds_barrier();
  if (FULL) {
#pragma unroll 4
    for (int k = 0; k < P2_IPT; ++k) {
      const uint32_t e = (uint32_t)k * SORT_THREADS + tid, b = st_bin[e];
      sorted[gcur[b] + (e - tstart[b])] = st_pay[e];
    }
  } else {
    for (uint32_t e = tid; e < kept; e += SORT_THREADS) {
      const uint32_t b = st_bin[e];
      sorted[gcur[b] + (e - tstart[b])] = st_pay[e];
    }
  }
  lds_barrier();
  for (uint32_t b = tid; b < NF; b += SORT_THREADS) {
    if (!COOP) gcur[b] += tcnt[b];
    tcnt[b] = 0;
  }
  lds_barrier();
}

template <bool COOP>
__global__ __launch_bounds__(SORT_THREADS) void msm_part2_scatter_v2_kernel(const uint32_t* __restrict__ tmp,
                                                                            const uint32_t* __restrict__ cstart,
                                                                            const uint32_t* __restrict__ boff,
                                                                            uint32_t* __restrict__ sorted, uint32_t fb,
                                                                            uint32_t ib, uint32_t NC, uint32_t NBP, uint32_t big,
                                                                            uint32_t slice, const uint2* __restrict__ list,
                                                                            const uint32_t* __restrict__ list_count,
                                                                            uint32_t* __restrict__ gcursor, Positional ps) {
  extern __shared__ uint32_t sm[];
  __shared__ uint32_t sc_start[PS_MAX_SC + 2];
  __shared__ uint32_t tile_sc[P2_TILE / 64];                  // super-chunk of every 64th position of the current tile
  uint32_t hb = blockIdx.x, w = blockIdx.y, sl = 0;
  const uint32_t tid = threadIdx.x;
  if (COOP) {
    if (blockIdx.x >= *list_count) return;
    const uint2 it = list[blockIdx.x];
    w = it.x / NC;
    hb = it.x - w * NC;
    sl = it.y;
  } else if (cstart[w * NC + hb + 1] - cstart[w * NC + hb] > big) {
    return;
  }
  const uint32_t NF = 1u << fb;                       // <= 4096
  uint32_t* gcur = sm;                                // global cursor of every fine bucket
  uint32_t* tcnt = gcur + NF;                         // items of the current tile per bucket
  uint32_t* tstart = tcnt + NF;                       // exclusive prefix of tcnt
  uint32_t* wsum = tstart + NF;                       // 32 words
  uint32_t* st_pay = wsum + 32;                       // tile items in bucket order
  uint16_t* st_bin = reinterpret_cast<uint16_t*>(st_pay + P2_TILE);   // their fine buckets (< 2^12)
  const uint32_t* bo = boff + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  uint32_t* gc = gcursor + (size_t)w * NBP + 1 + ((size_t)hb << fb);
  for (uint32_t b = tid; b < NF; b += SORT_THREADS) { gcur[b] = bo[b]; tcnt[b] = 0; }
  uint32_t lo = cstart[w * NC + hb], hi = cstart[w * NC + hb + 1];
  const uint32_t region_lo = lo, region_n = hi - lo;
  if (ps.nsc) {                                        // region-relative start of every super-chunk's runs; a sentinel behind them
    for (uint32_t sc = tid; sc <= ps.nsc + 1; sc += SORT_THREADS)
      sc_start[sc] = sc < ps.nsc ? ps.chist[((size_t)w * ps.G + (size_t)sc * ps.gpc) * NC + hb] : (sc == ps.nsc ? region_n : 0xffffffffu);
  }
  lds_barrier();
  if (COOP) {
    lo += sl * slice;
    hi = lo + slice < hi ? lo + slice : hi;
  }
  if (lo >= hi) return;
  uint4 q[P2_IPT / 4], qn[P2_IPT / 4];
  p2v2_load(tmp, lo & ~3u, lo, hi, tid, q);
  for (uint32_t tb = lo & ~3u; tb < hi; tb += P2_TILE) {   // tmp is 256-byte aligned: positions that are multiples of 4 are 16-byte addresses
    const bool more = tb + P2_TILE < hi;
    if (more) p2v2_load(tmp, tb + P2_TILE, lo, hi, tid, qn);     // the next tile's items travel while this one is ranked and staged
    if (tb >= lo && tb + P2_TILE <= hi)
      p2v2_tile<COOP, true>(q, sorted, tb, lo, hi, region_lo, ib, NF, ps, gcur, tcnt, tstart, wsum, st_pay, st_bin, sc_start, tile_sc, gc, tid);
    else
      p2v2_tile<COOP, false>(q, sorted, tb, lo, hi, region_lo, ib, NF, ps, gcur, tcnt, tstart, wsum, st_pay, st_bin, sc_start, tile_sc, gc, tid);
    if (more) {
#pragma unroll
      for (int j = 0; j < P2_IPT / 4; ++j) q[j] = qn[j];
    }
  }
}

// Measured negative in round 6 (profiles/r06_sort_ab.txt): the second-level scatter writes 4-item = 16-byte runs at 2^24 on the table
// (2.1 x its bytes in WRITE_SIZE; with every tile stored where it was read the kernel takes 0.48 ms instead of 0.83 -- the ceiling).
// A form with carry slots in LDS (8 words per bucket, items leave in whole aligned 32-byte sectors; needs fb <= 11, so one more coarse
// bit and half-size tiles) was correct and SLOWER than the plain scatter on the same plan, 906 against 716 us: two more per-bucket
// passes and a barrier per tile cost more than the full sectors save; ten coarse bits alone only move 0.13 ms from this level to the
// first.  The plan stays 9 + 12 bits.

// bucket offsets (exclusive scan of counts) and task offsets (exclusive scan of ceil(count / L)):
// three small launches -- per-block sums, a one-block scan of those, per-block rescan + offset.

__device__ __forceinline__ void block_scan_pair(uint32_t& p, uint32_t& t, uint32_t* s_p, uint32_t* s_t) {
  // inclusive scan over the block of (p, t); returns inclusive values in p, t
  const uint32_t tid = threadIdx.x;
  s_p[tid] = p;
  s_t[tid] = t;
  __syncthreads();
  for (uint32_t off = 1; off < SCAN_THREADS; off <<= 1) {
    uint32_t a = 0, b = 0;
    if (tid >= off) { a = s_p[tid - off]; b = s_t[tid - off]; }
    __syncthreads();
    s_p[tid] += a;
    s_t[tid] += b;
    __syncthreads();
  }
  p = s_p[tid];
  t = s_t[tid];
}

__global__ __launch_bounds__(SCAN_THREADS) void msm_scan_partial_kernel(const uint32_t* __restrict__ bcnt,
                                                                        uint32_t* __restrict__ blocksums, uint32_t NBT,
                                                                        const uint32_t* __restrict__ pairs, uint32_t L_host) {
  __shared__ uint32_t s_p[SCAN_THREADS], s_t[SCAN_THREADS];
  const uint32_t L = effective_task_len(pairs, L_host);
  const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  uint32_t sp = 0, st = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const uint32_t c = base + k < NBT ? bcnt[base + k] : 0u;
    sp += c;
    st += (c + L - 1) / L;
  }
  block_scan_pair(sp, st, s_p, s_t);
  if (threadIdx.x == SCAN_THREADS - 1) {
    blocksums[2 * blockIdx.x] = sp;
    blocksums[2 * blockIdx.x + 1] = st;
  }
}

// one block: exclusive scan of the per-block sums in place; totals[0] = pairs, totals[1] = tasks.
// totals[2] = 1 and totals[1] = 0 if the task count exceeds the capacity of the task arrays (a host-side
// bound that cannot be reached; if it ever were, every later kernel sees the flag and touches nothing,
// and msm_finish reports the error -- no out-of-bounds write happens first).
__global__ __launch_bounds__(SCAN_THREADS) void msm_scan_blocksums_kernel(uint32_t* __restrict__ blocksums, uint32_t nblocks,
                                                                          uint32_t* __restrict__ totals, uint32_t task_capacity) {
  __shared__ uint32_t s_p[SCAN_THREADS], s_t[SCAN_THREADS];
  uint32_t carry_p = 0, carry_t = 0;
  for (uint32_t start = 0; start < nblocks; start += SCAN_THREADS) {
    const uint32_t i = start + threadIdx.x;
    uint32_t p = i < nblocks ? blocksums[2 * i] : 0u, t = i < nblocks ? blocksums[2 * i + 1] : 0u;
    const uint32_t p0 = p, t0 = t;
    block_scan_pair(p, t, s_p, s_t);
    if (i < nblocks) {
      blocksums[2 * i] = carry_p + p - p0;
      blocksums[2 * i + 1] = carry_t + t - t0;
    }
    carry_p += s_p[SCAN_THREADS - 1];
    carry_t += s_t[SCAN_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool over = carry_t > task_capacity;
    totals[0] = carry_p;
    totals[1] = over ? 0u : carry_t;
    totals[2] = over ? 1u : 0u;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void msm_scan_final_kernel(const uint32_t* __restrict__ bcnt,
                                                                      const uint32_t* __restrict__ blocksums,
                                                                      uint32_t* __restrict__ boff, uint32_t* __restrict__ toff,
                                                                      const uint32_t* __restrict__ totals, uint32_t NBT,
                                                                      const uint32_t* __restrict__ pairs, uint32_t L_host,
                                                                      uint32_t* __restrict__ gcursor) {
  __shared__ uint32_t s_p[SCAN_THREADS], s_t[SCAN_THREADS];
  const uint32_t L = effective_task_len(pairs, L_host);
  const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  uint32_t c[SCAN_ITEMS];
  uint32_t sp = 0, st = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    c[k] = base + k < NBT ? bcnt[base + k] : 0u;
    sp += c[k];
    st += (c[k] + L - 1) / L;
  }
  const uint32_t sp0 = sp, st0 = st;
  block_scan_pair(sp, st, s_p, s_t);
  uint32_t rp = blocksums[2 * blockIdx.x] + sp - sp0, rt = blocksums[2 * blockIdx.x + 1] + st - st0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < NBT) {
      boff[base + k] = rp;
      toff[base + k] = rt;
      if (gcursor) gcursor[base + k] = rp;   // the cooperative scatter's global per-bucket cursors start at the offsets
    }
    rp += c[k];
    rt += (c[k] + L - 1) / L;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) toff[NBT] = totals[1];
}
// (with the overflow flag set toff keeps the unclamped offsets, so every consumer of toff checks totals[2] first)

// bucket order (small inputs): task t runs in slot t
__global__ void msm_task_fill_kernel(const uint32_t* __restrict__ toff, uint32_t* __restrict__ task_bucket,
                                     uint32_t* __restrict__ task_order, uint32_t NBT, const uint32_t* __restrict__ totals) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= NBT || totals[2]) return;
  const uint32_t lo = toff[b], hi = toff[b + 1];
  for (uint32_t t = lo; t < hi; ++t) {
    task_bucket[t] = b;
    task_order[t] = t;
  }
}

// Task list in order of decreasing chain length.  The 64 lanes of a K3 wave run in lockstep until the
// longest of their chains ends, so a wave of tasks taken in bucket order costs max-of-64 bucket sizes
// (for uniform scalars: mean + ~2.4 sigma, 12 % of the lane-cycles idle).  A counting sort of the tasks
// by length (1024 keys, descending) puts equal-length chains side by side, and starting with the longest
// also shortens the tail of the launch.  Only the ORDER of execution changes: task t still owns
// partial[t], so nothing downstream depends on the (atomic, run-to-run varying) order within one key.
constexpr uint32_t ORDER_HOT = 32;    // hot buckets a workgroup fills cooperatively (more fall back to their lane)

__device__ __forceinline__ uint32_t task_key(uint32_t len, uint32_t L) {   // len in [1, L]; key 0 = longest
  const uint32_t k = L < TASK_KEYS ? len : (uint32_t)(((uint64_t)len * (TASK_KEYS - 1)) / L);
  return (TASK_KEYS - 1) - k;
}

__global__ __launch_bounds__(ORDER_THREADS) void msm_task_hist_kernel(const uint32_t* __restrict__ bcnt, uint32_t NBT,
                                                                      const uint32_t* __restrict__ pairs, uint32_t L_host,
                                                                      uint32_t* __restrict__ khist) {
  __shared__ uint32_t h[TASK_KEYS];
  const uint32_t L = effective_task_len(pairs, L_host);
  h[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ORDER_ITEMS; ++k) {
    const uint32_t b = (blockIdx.x * ORDER_ITEMS + k) * ORDER_THREADS + threadIdx.x;
    if (b < NBT) {
      const uint32_t c = bcnt[b], full = c / L, rem = c - full * L;
      if (full) atomicAdd(&h[task_key(L, L)], full);
      if (rem) atomicAdd(&h[task_key(rem, L)], 1u);
    }
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&khist[threadIdx.x], h[threadIdx.x]);
}

// one block: khist -> exclusive start of every key, left in kcursor for the scatter to advance
__global__ __launch_bounds__(ORDER_THREADS) void msm_task_keyscan_kernel(const uint32_t* __restrict__ khist,
                                                                         uint32_t* __restrict__ kcursor) {
  __shared__ uint32_t s[TASK_KEYS];
  const uint32_t tid = threadIdx.x, v = khist[tid];
  s[tid] = v;
  __syncthreads();
  for (uint32_t off = 1; off < TASK_KEYS; off <<= 1) {
    const uint32_t a = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += a;
    __syncthreads();
  }
  kcursor[tid] = s[tid] - v;
}

__global__ __launch_bounds__(ORDER_THREADS) void msm_task_order_kernel(const uint32_t* __restrict__ bcnt,
                                                                       const uint32_t* __restrict__ toff, uint32_t NBT,
                                                                       const uint32_t* __restrict__ pairs, uint32_t L_host,
                                                                       uint32_t* __restrict__ kcursor,
                                                                       uint32_t* __restrict__ task_bucket,
                                                                       uint32_t* __restrict__ task_order,
                                                                       const uint32_t* __restrict__ totals) {
  __shared__ uint32_t h[TASK_KEYS], base[TASK_KEYS];
  if (totals[2]) return;                   // task arrays too small (see msm_scan_blocksums_kernel): write nothing
  const uint32_t L = effective_task_len(pairs, L_host);
  h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t cnt[ORDER_ITEMS];
#pragma unroll
  for (int k = 0; k < ORDER_ITEMS; ++k) {
    const uint32_t b = (blockIdx.x * ORDER_ITEMS + k) * ORDER_THREADS + threadIdx.x;
    cnt[k] = b < NBT ? bcnt[b] : 0u;
    const uint32_t full = cnt[k] / L, rem = cnt[k] - full * L;
    if (full) atomicAdd(&h[task_key(L, L)], full);
    if (rem) atomicAdd(&h[task_key(rem, L)], 1u);
  }
  __syncthreads();
  {   // one global reservation per key and workgroup; h becomes the local cursor
    const uint32_t mine = h[threadIdx.x];
    base[threadIdx.x] = mine ? atomicAdd(&kcursor[threadIdx.x], mine) : 0u;
    h[threadIdx.x] = 0;
  }
  __syncthreads();
  // a bucket cut into many full-length tasks (a hot bucket) is written by the whole workgroup
  __shared__ uint32_t hot_n, hot[ORDER_HOT][4];
  if (threadIdx.x == 0) hot_n = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ORDER_ITEMS; ++k) {
    const uint32_t b = (blockIdx.x * ORDER_ITEMS + k) * ORDER_THREADS + threadIdx.x;
    if (cnt[k] == 0) continue;
    const uint32_t full = cnt[k] / L, rem = cnt[k] - full * L;
    const uint32_t t0 = toff[b];
    if (full) {
      const uint32_t key = task_key(L, L), at = base[key] + atomicAdd(&h[key], full);
      const uint32_t slot = full > 64 ? atomicAdd(&hot_n, 1u) : ORDER_HOT;
      if (slot < ORDER_HOT) {
        hot[slot][0] = b; hot[slot][1] = t0; hot[slot][2] = full; hot[slot][3] = at;
      } else {
        for (uint32_t i = 0; i < full; ++i) {
          task_bucket[t0 + i] = b;
          task_order[at + i] = t0 + i;
        }
      }
    }
    if (rem) {
      const uint32_t key = task_key(rem, L);
      task_bucket[t0 + full] = b;
      task_order[base[key] + atomicAdd(&h[key], 1u)] = t0 + full;
    }
  }
  __syncthreads();
  const uint32_t nh = hot_n < ORDER_HOT ? hot_n : ORDER_HOT;
  for (uint32_t e = 0; e < nh; ++e) {
    const uint32_t b = hot[e][0], t0 = hot[e][1], full = hot[e][2], at = hot[e][3];
    for (uint32_t i = threadIdx.x; i < full; i += ORDER_THREADS) {
      task_bucket[t0 + i] = b;
      task_order[at + i] = t0 + i;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K3: bucket accumulation -- one lane per task, serial chain of mixed additions
// ---------------------------------------------------------------------------------------------
// Four waves per SIMD, stated: the lockstep products of g1x_madd_fast leave the register allocator free to take 129
// VGPRs (three waves) without it; told the budget it uses 121, no scratch.  HM_K3_WAVES: another budget for A/B
// (tools/ab_build.sh).
#ifndef HM_K3_WAVES
#define HM_K3_WAVES 4
#endif
#define HM_K3_OCC __attribute__((amdgpu_waves_per_eu(HM_K3_WAVES, HM_K3_WAVES)))
__global__ __launch_bounds__(ACC_THREADS) HM_K3_OCC void msm_accumulate_kernel(const uint32_t* __restrict__ sorted,
                                                                     const uint32_t* __restrict__ task_bucket,
                                                                     const uint32_t* __restrict__ task_order,
                                                                     const uint32_t* __restrict__ boff,
                                                                     const uint32_t* __restrict__ bcnt,
                                                                     const uint32_t* __restrict__ toff,
                                                                     const uint32_t* __restrict__ xy,
                                                                     uint32_t* __restrict__ partial,
                                                                     const uint32_t* __restrict__ totals,
                                                                     const uint32_t* __restrict__ pairs, uint32_t L_host) {
  __shared__ uint4 stage[4][ACC_THREADS];
  const uint32_t L = effective_task_len(pairs, L_host);
  const uint32_t lane = threadIdx.x;
  const uint32_t slot = blockIdx.x * ACC_THREADS + lane;
  const uint32_t T = totals[1];   // task count from the scan: the grid is sized by its host-side upper bound
  uint32_t start = 0, end = 0, t = 0;
  if (slot < T) {
    t = task_order[slot];       // longest chains first, equal lengths side by side
    const uint32_t b = task_bucket[t];
    const uint32_t k = t - toff[b];
    start = boff[b] + k * L;
    const uint32_t bucket_end = boff[b] + bcnt[b];
    end = start + L < bucket_end ? start + L : bucket_end;
  }
  if (start >= end) return;       // no task for this lane (the kernel has no barriers)
  const G1Jac res = accumulate_chain<true>(sorted, xy, start, end, stage, lane);   // lockstep products: g1.h
  store_jac(partial + (size_t)t * PT_WORDS, res);
}


// K3b: bucket = sum of its task partials.  Buckets with at most FINALIZE_SERIAL partials are
// summed by one lane; longer ones (hot buckets that K3 split into many tasks) are queued for
// the workgroup-per-bucket kernel below so that no single lane walks a long chain.
// `multi_only`: the reduction reads a one-task bucket straight from its partial and an empty one as the identity
// (load_bucket_value), so only buckets with two or more partials are summed and stored here: for uniform scalars a task
// is a bucket, and the pass would otherwise copy 112 B in and 112 B out for every one of them.
__global__ __launch_bounds__(ACC_THREADS) void msm_bucket_finalize_kernel(const uint32_t* __restrict__ partial,
                                                                          const uint32_t* __restrict__ toff,
                                                                          uint32_t* __restrict__ bucket, uint32_t NBT,
                                                                          uint32_t* __restrict__ big_count,
                                                                          uint32_t* __restrict__ big_list,
                                                                          uint2* __restrict__ slice_list,
                                                                          const uint32_t* __restrict__ totals,
                                                                          uint32_t multi_only) {
  const uint32_t b = blockIdx.x * ACC_THREADS + threadIdx.x;
  if (b >= NBT) return;
  if (totals[2]) {                         // overflow flag: no partial was written; leave an identity in every bucket
    if (!multi_only) store_jac(bucket + (size_t)b * PT_WORDS, g1_identity());   // (multi_only: the reader sees the flag itself)
    return;
  }
  const uint32_t lo = toff[b], hi = toff[b + 1];
  if (multi_only && hi - lo < 2) return;
  if (hi - lo > FINALIZE_SERIAL) {
    big_list[atomicAdd(big_count, 1u)] = b;
    if (hi - lo > FINALIZE_SLICE) {   // very hot: its partials are first summed slice by slice, many workgroups
      const uint32_t nsl = (hi - lo + FINALIZE_SLICE - 1) / FINALIZE_SLICE;
      const uint32_t at = atomicAdd(big_count + 1, nsl);
      for (uint32_t k = 0; k < nsl; ++k) slice_list[at + k] = make_uint2(b, k);
    }
    return;
  }
  G1Jac acc = g1_identity();
  for (uint32_t t = lo; t < hi; ++t) acc = g1_add(acc, load_jac(partial + (size_t)t * PT_WORDS));
  store_jac(bucket + (size_t)b * PT_WORDS, acc);
}

// first level for very hot buckets: slice k of bucket b = partials [lo + k*SLICE, +SLICE) -> their sum,
// written over the slice's first partial (each slice belongs to one workgroup)
__global__ __launch_bounds__(WIN_THREADS) void msm_bucket_finalize_slices_kernel(uint32_t* __restrict__ partial,
                                                                                 const uint32_t* __restrict__ toff,
                                                                                 const uint32_t* __restrict__ big_count,
                                                                                 const uint2* __restrict__ slice_list) {
  __shared__ uint32_t tree[WIN_THREADS * PT_WORDS];
  const uint32_t count = big_count[1];
  for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
    const uint2 e = slice_list[item];
    const uint32_t lo = toff[e.x] + e.y * FINALIZE_SLICE;
    const uint32_t end = toff[e.x + 1], hi = lo + FINALIZE_SLICE < end ? lo + FINALIZE_SLICE : end;
    G1Jac acc = g1_identity();
    for (uint32_t t = lo + threadIdx.x; t < hi; t += WIN_THREADS) acc = g1_add(acc, load_jac(partial + (size_t)t * PT_WORDS));
    const G1Jac r = block_sum_points(tree, acc);   // ends with a barrier: every read of the slice is done
    if (threadIdx.x == 0) store_jac(partial + (size_t)lo * PT_WORDS, r);
    __syncthreads();
  }
}

// one workgroup per hot bucket: all of its partials, or the slice sums the first level left behind
__global__ __launch_bounds__(WIN_THREADS) void msm_bucket_finalize_big_kernel(const uint32_t* __restrict__ partial,
                                                                              const uint32_t* __restrict__ toff,
                                                                              uint32_t* __restrict__ bucket,
                                                                              const uint32_t* __restrict__ big_count,
                                                                              const uint32_t* __restrict__ big_list) {
  __shared__ uint32_t tree[WIN_THREADS * PT_WORDS];
  const uint32_t count = *big_count;
  for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
    const uint32_t b = big_list[item];
    const uint32_t lo = toff[b], hi = toff[b + 1];
    const uint32_t step = hi - lo > FINALIZE_SLICE ? FINALIZE_SLICE : 1u;
    G1Jac acc = g1_identity();
    for (uint32_t t = lo + threadIdx.x * step; t < hi; t += WIN_THREADS * step)
      acc = g1_add(acc, load_jac(partial + (size_t)t * PT_WORDS));
    const G1Jac r = block_sum_points(tree, acc);
    if (threadIdx.x == 0) store_jac(bucket + (size_t)b * PT_WORDS, r);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// K4: per-window sum_b b * B_b
// ---------------------------------------------------------------------------------------------
// Where the reduction of a shared bucket set finds bucket gb (its index over all sets).  toff == nullptr: in bucket[gb], the
// finalize pass wrote every bucket.  Else (msm_bucket_finalize_kernel's multi_only): no task = the identity, one task = that
// task's partial, more = bucket[gb]; `none` (the overflow flag totals[2]: no partial was written) = identities everywhere.
// The two task offsets are read one element ahead of the record (bucket_tasks), so that the record's address is known
// when its load is issued.
struct BucketTasks {
  uint32_t lo, hi;
};
__device__ __forceinline__ BucketTasks bucket_tasks(const uint32_t* __restrict__ toff, uint32_t gb) {
  BucketTasks r{0, 0};
  if (toff != nullptr) {
    r.lo = toff[gb];
    r.hi = toff[gb + 1];
  }
  return r;
}
__device__ __forceinline__ G1Jac load_bucket_value(const uint32_t* __restrict__ bucket, const uint32_t* __restrict__ partial,
                                                   const uint32_t* __restrict__ toff, bool none, BucketTasks tk, uint32_t gb) {
  if (toff == nullptr) return load_jac(bucket + (size_t)gb * PT_WORDS);
  if (none || tk.hi == tk.lo) return g1_identity();
  return load_jac(tk.hi - tk.lo == 1 ? partial + (size_t)tk.lo * PT_WORDS : bucket + (size_t)gb * PT_WORDS);
}

// K4a: one lane per segment of SEG consecutive buckets [lo, lo+SEG): running sums give
// sum (b - lo + 1) B_b; the remaining (lo - 1) * (sum B_b) is a short double-and-add.
__global__ __launch_bounds__(ACC_THREADS) void msm_reduce_segments_kernel(const uint32_t* __restrict__ bucket,
                                                                          uint32_t* __restrict__ segres, uint32_t W,
                                                                          uint32_t NB, uint32_t NBP, uint32_t SEG,
                                                                          uint32_t nseg) {
  const uint32_t idx = blockIdx.x * ACC_THREADS + threadIdx.x;
  if (idx >= W * nseg) return;
  const uint32_t w = idx / nseg, sgi = idx - w * nseg;
  const uint32_t lo = sgi * SEG + 1;
  const uint32_t hi = lo + SEG - 1 < NB ? lo + SEG - 1 : NB;
  const uint32_t* bw = bucket + (size_t)w * NBP * PT_WORDS;
  // one wave per SIMD runs this kernel (the work is what costs, so SEG is long): nothing hides a bucket's load but the two
  // additions of the bucket before it -- the next record is requested before they start
  G1Jac run = g1_identity(), acc = g1_identity();
  G1Jac cur = hi >= lo ? load_jac(bw + (size_t)hi * PT_WORDS) : g1_identity();
  for (uint32_t b = hi; b >= lo; --b) {
    const G1Jac nxt = b > lo ? load_jac(bw + (size_t)(b - 1) * PT_WORDS) : g1_identity();
    run = g1_add(run, cur);
    acc = g1_add(acc, run);
    cur = nxt;
  }
  uint32_t m = lo - 1;  // < NB
  if (m != 0 && !run.inf) {
    G1Jac r = g1_identity();
    for (int bit = 31 - __clz(m); bit >= 0; --bit) {
      r = g1_double(r);
      if ((m >> bit) & 1) r = g1_add(r, run);
    }
    acc = g1_add(acc, r);
  }
  store_jac(segres + (size_t)idx * PT_WORDS, acc);
}

// K4b: sum `count` points per window down to ceil(count / SUM_SPAN) (one workgroup per span: strided
// serial sums then an LDS tree); applied until one point per window is left.
__global__ __launch_bounds__(WIN_THREADS) void msm_sum_points_kernel(const uint32_t* __restrict__ in, uint32_t count,
                                                                     uint32_t* __restrict__ out, uint32_t out_count) {
  __shared__ uint32_t tree[WIN_THREADS * PT_WORDS];
  const uint32_t w = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  const uint32_t* sw = in + (size_t)w * count * PT_WORDS;
  const uint32_t lo = blk * SUM_SPAN, hi = lo + SUM_SPAN < count ? lo + SUM_SPAN : count;
  G1Jac acc = g1_identity();
  for (uint32_t s = lo + t; s < hi; s += WIN_THREADS) acc = g1_add(acc, load_jac(sw + (size_t)s * PT_WORDS));
  const G1Jac r = block_sum_points(tree, acc);
  if (t == 0) store_jac(out + ((size_t)w * out_count + blk) * PT_WORDS, r);
}

// K4 for a SHARED bucket set (one window, up to 2^21 buckets), two launches deep instead of a running-sum chain.
// With j = b - 1 = hi * M + lo (M * H = NB, both powers of two):
//     sum_b b B_b = sum_lo lo * C_lo + sum_hi (M * hi + 1) * R_hi,     C_lo = sum_hi B, R_hi = sum_lo B
// so every bucket enters two PLAIN sums (a column and a row: any order, lanes then an LDS tree), the same two additions
// per bucket the running sums cost, without their serial chain of 2 * SEG additions and the log2(NB)-bit multiple behind
// it.  The H + M sums are then split by weight BIT: S_p = sum of the sums whose weight has bit p, one workgroup per
// bit, and the host fold, which doubles its way down 255 bits anyway, reads the c - 1 records S_p as windows of one bit.
// Launch 1: workgroup `blk` < H sums row hi = blk, the others column lo = blk - H.
// blockIdx.y = the bucket set (a group of MSMs over one table: one set each, NB + 1 bucket records and H + M sums apart)
// (the buckets are read through load_bucket_value; `totals` = the chain's totals words, [2] the overflow flag)
__global__ __launch_bounds__(WIN_THREADS) void msm_reduce_rowcol_kernel(const uint32_t* __restrict__ bucket, uint32_t* __restrict__ sums,
                                                                        uint32_t m, uint32_t h, const uint32_t* __restrict__ partial,
                                                                        const uint32_t* __restrict__ toff,
                                                                        const uint32_t* __restrict__ totals) {
  __shared__ uint32_t tree[WIN_THREADS * PT_WORDS];
  const uint32_t M = 1u << m, H = 1u << h, blk = blockIdx.x, t = threadIdx.x;
  const uint32_t b1 = blockIdx.y * (M * H + 1u) + 1u;                  // bucket b = j + 1 of this set, over all sets
  sums += (size_t)blockIdx.y * ((size_t)M + H) * PT_WORDS;
  const bool none = toff != nullptr && totals[2] != 0;
  const bool row = blk < H;
  const uint32_t count = row ? M : H;                                  // elements of this sum
  const uint32_t first = row ? blk * M : blk - H, stride = row ? 1u : M;
  G1Jac acc = g1_identity();
  if (t < count) {
    G1Jac cur = load_bucket_value(bucket, partial, toff, none, bucket_tasks(toff, b1 + first + t * stride), b1 + first + t * stride);
    BucketTasks tk = t + WIN_THREADS < count ? bucket_tasks(toff, b1 + first + (t + WIN_THREADS) * stride) : BucketTasks{0, 0};
    for (uint32_t e = t; e < count; e += WIN_THREADS) {                // the next record is requested before the addition starts
      const uint32_t en = e + WIN_THREADS, en2 = en + WIN_THREADS;
      const G1Jac nxt = en < count ? load_bucket_value(bucket, partial, toff, none, tk, b1 + first + en * stride) : g1_identity();
      if (en2 < count) tk = bucket_tasks(toff, b1 + first + en2 * stride);
      acc = g1_add(acc, cur);
      cur = nxt;
    }
  }
  const G1Jac r = block_sum_points_upto(tree, acc, count < WIN_THREADS ? count : WIN_THREADS);
  if (t == 0) store_jac(sums + (size_t)blk * PT_WORDS, r);
}

// The same H + M sums with ONE WAVE per workgroup and no tree wider than it: where the launch still gives every SIMD two
// waves (H + M / 2 >= 2048: c >= 22), the 8-level trees of the form above are what it pays for -- a general addition is
// ~3 700 dependent instructions, and a tree level keeps a whole wave issuing for 128, 64, ... 1 useful lanes.
//   workgroup blk < H        row hi = blk: lane l sums the M / 64 elements lo = l, l + 64, ... then a 6-level tree of the wave;
//   workgroup H + cp         columns 2 cp and 2 cp + 1, one per half wave: lane l of a half sums the H / 32 elements
//                            hi = l, l + 32, ... then a 5-level tree inside the half.
// Wave-additions issued at c = 22 (M = 2048, H = 1024): rows 1024 x (32 + 6), column pairs 1024 x (32 + 5) = 76 800 for
// 2 x 2^21 / 64 = 65 536 useful: 1.17 x (the workgroup form: (4 x 8 + 9) x 1024 + (4 x 4 + 9) x 2048 = 93 184, 1.42 x).
// acc += q, field by field: g1_add's `return p` / `return q` copy whole records, and with them the three padding bytes behind
// the identity flag, which this kernel's loop then carries through a stack slot (12 bytes of scratch for nothing)
__device__ __forceinline__ void jac_set(G1Jac& d, const G1Jac& s) {
  d.x = s.x;
  d.y = s.y;
  d.z = s.z;
  d.inf = s.inf;
}
__device__ __forceinline__ void jac_accumulate(G1Jac& acc, const G1Jac& q) {
  if (q.inf) return;
  if (acc.inf) {
    jac_set(acc, q);
    return;
  }
  const G1Jac r = g1_add_nz(acc, q);
  jac_set(acc, r);
}
// Two waves per SIMD, stated: eight one-wave workgroups per CU and no more, so that the 2 048 of c = 22 spread over all
// 256 CUs instead of filling some CUs three deep (the register budget would allow it) while others stand idle.
__global__ __launch_bounds__(WAVE_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void msm_reduce_rowcol_wave_kernel(const uint32_t* __restrict__ bucket,
                                                                              uint32_t* __restrict__ sums, uint32_t m, uint32_t h,
                                                                              const uint32_t* __restrict__ partial,
                                                                              const uint32_t* __restrict__ toff,
                                                                              const uint32_t* __restrict__ totals) {
  __shared__ uint32_t tree[WAVE_THREADS * PT_WORDS];
  const uint32_t M = 1u << m, H = 1u << h, blk = blockIdx.x, t = threadIdx.x;
  const uint32_t b1 = blockIdx.y * (M * H + 1u) + 1u;                  // bucket b = j + 1 of this set, over all sets
  sums += (size_t)blockIdx.y * ((size_t)M + H) * PT_WORDS;
  const bool none = toff != nullptr && totals[2] != 0;
  const bool row = blk < H;
  const uint32_t width = row ? 64u : 32u;                              // lanes per sum
  const uint32_t l = t & (width - 1u);
  const uint32_t count = row ? M : H;                                  // elements of this lane's sum
  const uint32_t sum_index = row ? blk : H + 2u * (blk - H) + (t >> 5);   // where it goes: rows, then columns
  const uint32_t first = row ? blk * M : sum_index - H, stride = row ? 1u : M;
  G1Jac acc = g1_identity();
  if (l < count) {
    G1Jac cur = load_bucket_value(bucket, partial, toff, none, bucket_tasks(toff, b1 + first + l * stride), b1 + first + l * stride);
    BucketTasks tk = l + width < count ? bucket_tasks(toff, b1 + first + (l + width) * stride) : BucketTasks{0, 0};
    for (uint32_t e = l; e < count; e += width) {                      // the next record is requested before the addition starts
      const uint32_t en = e + width, en2 = en + width;
      const G1Jac nxt = en < count ? load_bucket_value(bucket, partial, toff, none, tk, b1 + first + en * stride) : g1_identity();
      if (en2 < count) tk = bucket_tasks(toff, b1 + first + en2 * stride);
      jac_accumulate(acc, cur);
      jac_set(cur, nxt);
    }
  }
  store_jac(tree + t * PT_WORDS, acc);                                 // lanes past `count` hold the identity
  __syncthreads();
  for (uint32_t off = width / 2; off > 0; off >>= 1) {
    if (l < off) {
      G1Jac a = load_jac(tree + t * PT_WORDS);
      jac_accumulate(a, load_jac(tree + (t + off) * PT_WORDS));
      store_jac(tree + t * PT_WORDS, a);
    }
    __syncthreads();
  }
  const G1Jac r = load_jac(tree + (t & ~(width - 1u)) * PT_WORDS);
  if (l == 0) store_jac(sums + (size_t)sum_index * PT_WORDS, r);
}

// Launch 2: workgroup p sums the rows / columns whose weight has bit p and writes the record the host fold reads.
// Columns: weight lo (bits 0 .. m - 1).  Rows: weight M * hi + 1 (bit 0, and bits m .. m + h - 1).
// blockIdx.y = the bucket set; its records go res_stride words behind the previous set's, each block led by a copy of the
// chain's four totals words (what the host reads per element: msm_finish_wait_fold)
__global__ __launch_bounds__(WIN_THREADS) void msm_reduce_bits_kernel(const uint32_t* __restrict__ sums, uint32_t m, uint32_t h,
                                                                      uint32_t* __restrict__ winres, uint32_t res_stride) {
  __shared__ uint32_t tree[WIN_THREADS * PT_WORDS];
  const uint32_t M = 1u << m, H = 1u << h, p = blockIdx.x, t = threadIdx.x;
  sums += (size_t)blockIdx.y * ((size_t)M + H) * PT_WORDS;
  if (blockIdx.y != 0 && p == 0 && t < 4) (winres - 4)[(size_t)blockIdx.y * res_stride + t] = (winres - 4)[t];
  winres += (size_t)blockIdx.y * res_stride;
  const uint32_t* rows = sums;
  const uint32_t* cols = sums + (size_t)H * PT_WORDS;
  G1Jac acc = g1_identity();
  uint32_t widest = 0;                                                 // lanes holding anything: the tree's width
  if (p < m) {                                                         // the M / 2 columns with bit p of lo set
    const uint32_t half = M >> 1, low = (1u << p) - 1u;
    for (uint32_t i = t; i < half; i += WIN_THREADS) {
      const uint32_t lo = ((i & ~low) << 1) | (1u << p) | (i & low);
      acc = g1_add(acc, load_jac(cols + (size_t)lo * PT_WORDS));
    }
    widest = half;
    if (p == 0) {                                                      // every row: the + 1 of its weight
      for (uint32_t hi = t; hi < H; hi += WIN_THREADS) acc = g1_add(acc, load_jac(rows + (size_t)hi * PT_WORDS));
      if (H > widest) widest = H;
    }
  } else {                                                             // the H / 2 rows with bit p - m of hi set
    const uint32_t q = p - m, half = H >> 1, low = (1u << q) - 1u;
    for (uint32_t i = t; i < half; i += WIN_THREADS) {
      const uint32_t hi = ((i & ~low) << 1) | (1u << q) | (i & low);
      acc = g1_add(acc, load_jac(rows + (size_t)hi * PT_WORDS));
    }
    widest = half;
  }
  if (widest > WIN_THREADS) widest = WIN_THREADS;
  if (widest < 1) widest = 1;
  const G1Jac r = block_sum_points_upto(tree, acc, widest);
  if (t == 0) store_window_ext(winres + (size_t)p * 32, r);
}

// window sums -> the external Jacobian format (12 x u64 + flag word) the host fold reads
__global__ void msm_windows_to_ext_kernel(const uint32_t* __restrict__ in, uint32_t W, uint32_t* __restrict__ winres) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  store_window_ext(winres + (size_t)w * 32, load_jac(in + (size_t)w * PT_WORDS));
}

// ---------------------------------------------------------------------------------------------
// fixed-base scalar multiplication (ParamsKZG::setup's G1 work; also builds the bench SRS)
// out[i] = [k_i] B, affine external.  One lane per scalar: 4-bit fixed windows over a 64 x 15
// table of multiples of B built by the first kernel; final inversion by Fermat per lane.
// ---------------------------------------------------------------------------------------------
struct G1AffineWords {     // one external affine point, passed to the table kernel by value
  uint32_t w[16];
};
__global__ void g1_fixed_table_kernel(G1AffineWords base_ext, uint32_t* __restrict__ table) {
  // table[w][d-1] = [d * 16^w] B as Jacobian records, w < 64, d in 1..15.  One lane per window.
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= 64) return;
  uint32_t wx[8], wy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { wx[k] = base_ext.w[k]; wy[k] = base_ext.w[8 + k]; }
  G1Aff b;
  b.x = fe_from_ext<FqParams>(wx);
  b.y = fe_from_ext<FqParams>(wy);
  G1Jac p = g1_from_affine(b);
  for (uint32_t k = 0; k < 4 * w; ++k) p = g1_double(p);
  G1Jac acc = p;
  for (uint32_t d = 1; d <= 15; ++d) {
    store_jac(table + ((size_t)w * 15 + (d - 1)) * PT_WORDS, acc);
    acc = g1_add(acc, p);
  }
}

// Precomputed multiples for a fixed base set: table[j*n + i] = 2^(c*j) * P_i (affine, internal
// packed), j < W.  With them every window's digit indexes its own copy of the point and ALL windows
// share one set of 2^(c-1) buckets, so the window size is no longer capped by W bucket sets (c = 22,
// W = 12 at 2^24 instead of c = 16, W = 16: a quarter fewer mixed additions) and the final Horner
// disappears.  One lane per point: c doublings, then a Fermat inversion per stored multiple.
__global__ __launch_bounds__(ACC_THREADS) void msm_precompute_kernel(uint32_t* __restrict__ table,
                                                                     const uint8_t* __restrict__ inf, size_t n, uint32_t c,
                                                                     uint32_t W, uint32_t n_wide) {
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  if (inf[i]) {
    for (uint32_t j = 1; j < W; ++j) {
      uint4* o = reinterpret_cast<uint4*>(table + ((size_t)j * n + i) * 16);
      o[0] = o[1] = o[2] = o[3] = make_uint4(0, 0, 0, 0);
    }
    return;
  }
  G1Jac p = g1_from_affine(load_base(table, (uint32_t)i));
  for (uint32_t j = 1; j < W; ++j) {
    const uint32_t bits = j < n_wide ? c : c - 1;           // multiple j = 2^(offset of window j) P, HALF of it for a narrow window (see msm_digits_kernel)
    for (uint32_t k = 0; k < bits; ++k) p = g1_double_nz(p);   // a point of odd prime order never doubles to the identity
    const Fq zi = fq_inverse(p.z);
    const Fq zi2 = fe_sqr(zi);
    const Fq zi3 = fe_mul(zi2, zi);
    uint32_t ox[8], oy[8];
    fe_pack(ox, fe_mul(p.x, zi2));
    fe_pack(oy, fe_mul(p.y, zi3));
    uint4* o = reinterpret_cast<uint4*>(table + ((size_t)j * n + i) * 16);
    o[0] = make_uint4(ox[0], ox[1], ox[2], ox[3]);
    o[1] = make_uint4(ox[4], ox[5], ox[6], ox[7]);
    o[2] = make_uint4(oy[0], oy[1], oy[2], oy[3]);
    o[3] = make_uint4(oy[4], oy[5], oy[6], oy[7]);
  }
}

// The same table in two passes with ONE inversion per point instead of one per stored multiple (Montgomery's trick
// over the W - 1 Z coordinates of a point's chain): a Fermat inversion costs ~380 products, the c doublings between
// two multiples ~130, so the single-pass kernel above spends three quarters of its time inverting (674 ms for 2^24
// points, W = 12).  Pass A runs the doubling chain and leaves every multiple in JACOBIAN form -- (X, Y) packed in its
// table slot, Z and the running product Z_1 ... Z_j in a scratch array; pass B inverts the last running product and
// walks back, turning every slot into the affine point.
__device__ __forceinline__ void store_packed(uint32_t* dst, const Fq& v) {
  uint32_t w[8];
  fe_pack(w, v);
  uint4* o = reinterpret_cast<uint4*>(dst);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
__device__ __forceinline__ Fq load_packed(const uint32_t* src) {
  const uint4* q = reinterpret_cast<const uint4*>(src);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return fe_unpack<FqParams>(w);
}
// ztmp: [2][W - 1][n][8 words]: half 0 the Z coordinates, half 1 their running products
// Both passes work on a SLAB of m points starting at `first` (the scratch is per slab: [2][W - 1][m][8 words]).
__global__ __launch_bounds__(ACC_THREADS) void msm_precompute_chain_kernel(uint32_t* __restrict__ table, uint32_t* __restrict__ ztmp,
                                                                           const uint8_t* __restrict__ inf, size_t n, uint32_t c,
                                                                           uint32_t W, uint32_t n_wide, size_t first, size_t m) {
  const size_t r = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x, i = first + r;
  if (r >= m || i >= n || inf[i]) return;           // identity bases: pass B zeroes their slots
  G1Jac p = g1_from_affine(load_base(table, (uint32_t)i));
  Fq run = fe_one<FqParams>();
  for (uint32_t j = 1; j < W; ++j) {
    const uint32_t bits = j < n_wide ? c : c - 1;           // as in msm_precompute_kernel
    for (uint32_t k = 0; k < bits; ++k) p = g1_double_nz(p);   // a point of odd prime order never doubles to the identity
    uint32_t* slot = table + ((size_t)j * n + i) * 16;
    store_packed(slot, p.x);
    store_packed(slot + 8, p.y);
    run = j == 1 ? p.z : fe_mul(run, p.z);
    store_packed(ztmp + ((size_t)(j - 1) * m + r) * 8, p.z);
    store_packed(ztmp + ((size_t)(W - 1 + j - 1) * m + r) * 8, run);
  }
}
__global__ __launch_bounds__(ACC_THREADS) void msm_precompute_normalise_kernel(uint32_t* __restrict__ table,
                                                                               const uint32_t* __restrict__ ztmp,
                                                                               const uint8_t* __restrict__ inf, size_t n, uint32_t W,
                                                                               size_t first, size_t m) {
  const size_t r = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x, i = first + r;
  if (r >= m || i >= n) return;
  if (inf[i]) {
    for (uint32_t j = 1; j < W; ++j) {
      uint4* o = reinterpret_cast<uint4*>(table + ((size_t)j * n + i) * 16);
      o[0] = o[1] = o[2] = o[3] = make_uint4(0, 0, 0, 0);
    }
    return;
  }
  Fq inv = fq_inverse(load_packed(ztmp + ((size_t)(W - 1 + W - 2) * m + r) * 8));      // 1 / (Z_1 ... Z_{W-1})
  for (uint32_t j = W - 1; j >= 1; --j) {
    const Fq zj = load_packed(ztmp + ((size_t)(j - 1) * m + r) * 8);
    const Fq zi = j > 1 ? fe_mul(inv, load_packed(ztmp + ((size_t)(W - 1 + j - 2) * m + r) * 8)) : inv;   // 1 / Z_j
    inv = fe_mul(inv, zj);                                                                // 1 / (Z_1 ... Z_{j-1})
    const Fq zi2 = fe_sqr(zi);
    const Fq zi3 = fe_mul(zi2, zi);
    uint32_t* slot = table + ((size_t)j * n + i) * 16;
    const Fq ax = fe_mul(load_packed(slot), zi2), ay = fe_mul(load_packed(slot + 8), zi3);
    store_packed(slot, ax);
    store_packed(slot + 8, ay);
  }
}

__global__ __launch_bounds__(ACC_THREADS) void g1_fixed_base_mul_kernel(const uint32_t* __restrict__ scalars,
                                                                        const uint32_t* __restrict__ table,
                                                                        uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(scalars + i * 8);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w_in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  Fr k32 = fe_zero<FrParams>();
  k32.l[0] = 32;
  uint32_t v[8];
  fe_pack(v, fe_canonical(fe_mul(fe_unpack<FrParams>(w_in), k32)));
  G1Jac acc = g1_identity();
  for (uint32_t w = 0; w < 64; ++w) {
    const uint32_t d = (v[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (d != 0) acc = g1_add(acc, load_jac(table + ((size_t)w * 15 + (d - 1)) * PT_WORDS));
  }
  uint32_t ox[8], oy[8];
  if (acc.inf) {
#pragma unroll
    for (int k = 0; k < 8; ++k) ox[k] = oy[k] = 0;
  } else {
    const Fq zi = fq_inverse(acc.z);
    const Fq zi2 = fe_sqr(zi);
    const Fq zi3 = fe_mul(zi2, zi);
    fe_to_ext(ox, fe_mul(acc.x, zi2));
    fe_to_ext(oy, fe_mul(acc.y, zi3));
  }
  uint4* o = reinterpret_cast<uint4*>(out + i * 16);
  o[0] = make_uint4(ox[0], ox[1], ox[2], ox[3]);
  o[1] = make_uint4(ox[4], ox[5], ox[6], ox[7]);
  o[2] = make_uint4(oy[0], oy[1], oy[2], oy[3]);
  o[3] = make_uint4(oy[4], oy[5], oy[6], oy[7]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int msm_convert_bases(const uint32_t* d_bases_ext, uint32_t* d_xy, uint8_t* d_inf, size_t n, hipStream_t stream) {
  if (n == 0) return HM_OK;
  hipLaunchKernelGGL(msm_convert_bases_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_bases_ext, d_xy,
                     d_inf, n);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// host-side Horner over the window sums and affine normalisation (host_fq.h: native 4 x u64
// arithmetic on the external-format words the reduction kernel wrote)
// result = sum_w 2^(offset of window w) * S_w: Horner from the top window, shifting by the width of window w
// before its sum is added (widths == nullptr: every window is c bits wide)
static void host_fold(const uint32_t* winres, uint32_t W, uint32_t c, uint64_t out_jac_ext[12], int* out_is_identity,
                      const uint8_t* widths = nullptr) {
  host::G1J acc = host::g1_identity();
  for (int w = (int)W - 1; w >= 0; --w) {
    const uint32_t shift = widths ? widths[w] : c;
    for (uint32_t k = 0; k < shift; ++k) acc = host::g1_double(acc);
    const uint32_t* o = winres + (size_t)w * 32;
    if (o[24] == 0) {
      host::G1J p;
      std::memcpy(p.x.l, o, 32);
      std::memcpy(p.y.l, o + 8, 32);
      std::memcpy(p.z.l, o + 16, 32);
      acc = host::g1_add(acc, p);
    }
  }
  host::g1_normalise(acc, out_jac_ext, out_is_identity);
}

// sum of `count` external Jacobian points (12 u64 each, z = 0 for the identity) on the host:
// the fold of per-GPU partial MSM results after the RCCL all-gather (a few points, latency only)
void host_sum_points(const uint64_t* pts, size_t count, uint64_t out_jac_ext[12], int* out_is_identity) {
  std::vector<uint32_t> win(count * 32, 0);
  for (size_t i = 0; i < count; ++i) {
    const uint64_t* p = pts + i * 12;
    std::memcpy(&win[i * 32], p, 96);
    win[i * 32 + 24] = (p[8] | p[9] | p[10] | p[11]) == 0 ? 1u : 0u;
  }
  host_fold(win.data(), (uint32_t)count, 0, out_jac_ext, out_is_identity);
}

static std::atomic<int> g_window_override{0};   // process-wide knob, read once per MSM
// Per-phase events (digits / sort / accumulate / reduce, and the accumulate kernel alone) cost seven event records per
// MSM -- nothing against a 20 ms MSM, a fifth of the host time of a prover-sized one.  -1: the general pipeline records
// them, the five-launch plan does not; 0 / 1: never / always (hm_msm_set_phase_timing).
static std::atomic<int> g_phase_timing{-1};
void msm_set_phase_timing(int mode) { g_phase_timing.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }
bool msm_phase_timing(bool small_plan) {
  const int m = g_phase_timing.load(std::memory_order_relaxed);
  return m < 0 ? !small_plan : m != 0;
}
void msm_set_window_override(int c) { g_window_override.store(c, std::memory_order_relaxed); }

// The one reader of what a call is told from outside (msm_plan.inc: MsmKnobs): the window override and the three switches the
// tests use as their reference arm -- read at every call, so that one process can run both arms.
static MsmKnobs msm_read_knobs(bool window_only = false) {
  const auto tri = [](const char* name) {
    const char* v = std::getenv(name);
    return v && *v ? (*v == '1' ? 1 : 0) : -1;
  };
  MsmKnobs k;
  k.window_override = g_window_override.load(std::memory_order_relaxed);
  if (window_only) return k;                      // the window queries of the prover's small path: no environment read
  k.digits_count = tri("HALO2_MI355X_DIGITS_COUNT");
  k.k3b_copy = tri("HALO2_MI355X_K3B_COPY");
  k.k4_wave_sums = tri("HALO2_MI355X_K4_WAVE_SUMS");
  return k;
}

uint32_t msm_precomp_window(size_t n) { return plan_precomp_window(n); }

int msm_precompute(uint32_t* d_table, const uint8_t* d_inf, size_t n, uint32_t c, uint32_t W, hipStream_t stream) {
  if (n == 0 || W <= 1) return HM_OK;
  uint32_t wide, n_wide;
  balanced_windows(W, &wide, &n_wide);
  if (wide != c) return hm_fail(HM_ERR_INTERNAL, "msm: precomputation window is not the balanced width");
  const dim3 grid((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS)), block(ACC_THREADS);
  // two passes with one inversion per point (scratch: 64 B per stored multiple, freed before returning); the one-pass
  // kernel when that scratch cannot be had
  uint32_t* d_z = nullptr;
  static const bool one_pass = [] { const char* v = std::getenv("HALO2_MI355X_PRECOMP_ONE_PASS"); return v && *v == '1'; }();
  const size_t slab = n < ((size_t)1 << 20) ? n : ((size_t)1 << 20);      // <= 1 GiB of scratch whatever the set's size
  if (!one_pass && hipMalloc((void**)&d_z, (size_t)2 * (W - 1) * slab * 32) == hipSuccess) {
    const dim3 sgrid((uint32_t)((slab + ACC_THREADS - 1) / ACC_THREADS));
    for (size_t first = 0; first < n; first += slab) {
      hipLaunchKernelGGL(msm_precompute_chain_kernel, sgrid, block, 0, stream, d_table, d_z, d_inf, n, c, W, n_wide, first, slab);
      hipLaunchKernelGGL(msm_precompute_normalise_kernel, sgrid, block, 0, stream, d_table, (const uint32_t*)d_z, d_inf, n, W, first, slab);
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(stream);
    (void)hipFree(d_z);
    if (e1 != hipSuccess || e2 != hipSuccess) return hm_fail(HM_ERR_HIP, "msm: precomputation failed");
    return HM_OK;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(msm_precompute_kernel, grid, block, 0, stream, d_table, d_inf, n, c, W, n_wide);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

static_assert(MSM_GROUP_MAX == HM_MSM_GROUP, "msm_plan.inc and hm_internal.h disagree about the group size");

struct MsmWorkspace {       // a slot's workspace under a plan's region table
  uint8_t* base;
  const MsmPlan& p;
  template <class T = uint32_t> T* at(MsmRegion r) const { return (T*)(base + p.region[r].off); }
};

// The first sort level (where the plan has one) and the bucket counts; regions far above their share go to the cooperative
// kernels.  64-bit items exist in ONE combination (tests/test_msm_plan_host.py): a first level by histogram, both tiled scatters.
template <class ITEM>
static void launch_sort(const MsmPlan& p, const MsmWorkspace& w, hipStream_t stream) {
  const MsmLaunch* const l = p.launch;
  int32_t* digits = w.at<int32_t>(MR_DIGITS);
  uint32_t *chist = w.at(MR_CHIST), *ctot = w.at(MR_CTOT), *cstart = w.at(MR_CSTART), *bcnt = w.at(MR_BCNT), *brcount = w.at(MR_BRCOUNT);
  ITEM* tmp = w.at<ITEM>(MR_TMP);
  uint2* brlist = w.at<uint2>(MR_BRLIST);
  if constexpr (sizeof(ITEM) == 4) {
    if (p.first_level == MSM_P1_NONE)
      return launch(msm_part2_hist_kernel<true, ITEM, false>, l[ML_P2_HIST], stream, tmp, digits, cstart, bcnt, p.sn, p.fb, p.ib, p.NC, p.NBP,
                    0xffffffffu, 0u, (const uint2*)nullptr, (const uint32_t*)nullptr);
  }
  launch(msm_part1_hist_kernel, l[ML_P1_HIST], stream, digits, chist, p.sn, p.chunk, p.fb, p.NC);   // not after the counting digits pass
  launch(msm_part1_scan_kernel, l[ML_P1_SCAN], stream, chist, ctot, p.G, p.NC, p.SW);
  launch(msm_part1_starts_kernel, l[ML_P1_STARTS], stream, ctot, cstart, p.SW * p.NC);
  const auto scatter = [&](auto kernel) { launch(kernel, l[ML_P1_SCATTER], stream, digits, chist, cstart, tmp, p.sn, p.chunk, p.fb, p.ib, p.NC); };
  if constexpr (sizeof(ITEM) == 8) scatter(msm_part1_scatter_tiled_kernel<ITEM>);
  else if (p.p1_scatter == MSM_P1S_DIRECT) scatter(msm_part1_scatter_kernel<ITEM>);
  else if (p.p1_scatter == MSM_P1S_VEC_BIG) scatter(msm_part1_scatter_v2_kernel<P1_BIG_IPT>);
  else scatter(msm_part1_scatter_v2_kernel<P1_IPT_DEFAULT>);
  launch(msm_big_regions_kernel, l[ML_BIG_REGIONS], stream, cstart, p.SW * p.NC, p.br_big, p.br_slice, brlist, brcount, p.br_capacity);
  launch(msm_part2_hist_kernel<false, ITEM, false>, l[ML_P2_HIST], stream, tmp, digits, cstart, bcnt, p.sn, p.fb, p.ib, p.NC, p.NBP, p.br_big,
         p.br_slice, brlist, brcount);
  launch(msm_part2_hist_kernel<false, ITEM, true>, l[ML_P2_HIST_COOP], stream, tmp, digits, cstart, bcnt, p.sn, p.fb, p.ib, p.NC, p.NBP,
         p.br_big, p.br_slice, brlist, brcount);
}

// The second sort level's scatter, after the scan of the bucket counts.
template <class ITEM>
static void launch_sort_scatter(const MsmPlan& p, const MsmWorkspace& w, hipStream_t stream) {
  const MsmLaunch &s = p.launch[ML_P2_SCATTER], &sc = p.launch[ML_P2_SCATTER_COOP];
  const int32_t* digits = w.at<int32_t>(MR_DIGITS);
  const ITEM* tmp = w.at<ITEM>(MR_TMP);
  const uint32_t *cstart = w.at(MR_CSTART), *boff = w.at(MR_BOFF), *brcount = w.at(MR_BRCOUNT);
  const uint2* brlist = w.at<uint2>(MR_BRLIST);
  uint32_t *sorted = w.at(MR_SORTED), *gcursor = w.at(MR_GCUR);
  if constexpr (sizeof(ITEM) == 8) {
    launch(msm_part2_scatter_tiled_kernel<ITEM, false>, s, stream, tmp, cstart, boff, sorted, p.fb, p.ib, p.NC, p.NBP, p.br_big, p.br_slice,
           brlist, brcount, gcursor);
    launch(msm_part2_scatter_tiled_kernel<ITEM, true>, sc, stream, tmp, cstart, boff, sorted, p.fb, p.ib, p.NC, p.NBP, p.br_big, p.br_slice,
           brlist, brcount, gcursor);
  } else if (p.p2_scatter == MSM_P2S_DIGITS) {
    launch(msm_part2_scatter_kernel<true, ITEM>, s, stream, tmp, digits, cstart, boff, sorted, p.sn, p.fb, p.ib, p.NC, p.NBP);
  } else if (p.p2_scatter == MSM_P2S_DIRECT) {
    launch(msm_part2_scatter_kernel<false, ITEM>, s, stream, tmp, digits, cstart, boff, sorted, p.sn, p.fb, p.ib, p.NC, p.NBP);
  } else {
    const Positional ps{w.at(MR_CHIST), p.ps_G, p.ps_gpc, p.ps_nsc};
    launch(msm_part2_scatter_v2_kernel<false>, s, stream, tmp, cstart, boff, sorted, p.fb, p.ib, p.NC, p.NBP, p.br_big, p.br_slice, brlist,
           brcount, gcursor, ps);
    launch(msm_part2_scatter_v2_kernel<true>, sc, stream, tmp, cstart, boff, sorted, p.fb, p.ib, p.NC, p.NBP, p.br_big, p.br_slice, brlist,
           brcount, gcursor, ps);
  }
}

int msm_slot_prepare(MsmSlot& sl) {
  if (!sl.ev_ready) {
    for (int i = 0; i < 7; ++i) HM_HIP_CHECK(hipEventCreate(&sl.ev[i]));
    HM_HIP_CHECK(hipHostMalloc((void**)&sl.h_land, (size_t)HM_MSM_GROUP * (128 * 32 + 4) * sizeof(uint32_t), hipHostMallocDefault));
    sl.ev_ready = true;
  }
  return HM_OK;
}

// the sort kernels that ask for more dynamic LDS than the default, and how much each may have (per device: a process may drive several GPUs)
static int msm_set_lds_attributes() {
  static const void* const kFine[] = {      // the LDS-histogram kernels: MSM_LDS_FINE
      (const void*)msm_part2_hist_kernel<true, uint32_t, false>,  (const void*)msm_part2_hist_kernel<false, uint32_t, false>,
      (const void*)msm_part2_hist_kernel<false, uint64_t, false>, (const void*)msm_part2_hist_kernel<false, uint32_t, true>,
      (const void*)msm_part2_hist_kernel<false, uint64_t, true>,  (const void*)msm_part2_scatter_kernel<true, uint32_t>,
      (const void*)msm_part2_scatter_kernel<false, uint32_t>,     (const void*)msm_part1_scatter_tiled_kernel<uint64_t>};
  static const void* const kAll[] = {       // the LDS-sorted tiles of the scatters: MSM_LDS_ALL
      (const void*)msm_part1_scatter_v2_kernel<P1_IPT_DEFAULT>,         (const void*)msm_part1_scatter_v2_kernel<P1_BIG_IPT>,
      (const void*)msm_part2_scatter_v2_kernel<false>,                  (const void*)msm_part2_scatter_v2_kernel<true>,
      (const void*)msm_part2_scatter_tiled_kernel<uint64_t, false>,     (const void*)msm_part2_scatter_tiled_kernel<uint64_t, true>};
  for (const void* k : kFine) HM_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MSM_LDS_FINE));
  for (const void* k : kAll) HM_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MSM_LDS_ALL));
  return HM_OK;
}

// Enqueue every kernel of one MSM on `stream` using workspace slot `slot`; nothing here waits for
// the device.  d_xy: n points (plain) or the precomputed table of precomp_W * n points
// (precomp_c != 0).  msm_finish() later waits for the slot, folds the window sums on the host and
// fills the statistics.
// `group` MSMs over the same points in ONE launch chain (group > 1: only on a fixed-base table set below the positional
// plan's sizes -- msm_table_group_max -- where every element is one bucket set of the same sort and the same K3 launch).
// Every size, variant, grid and workspace offset is msm_plan's (msm_plan.inc); launches the plan does not make are skipped.
static int msm_issue(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                     const uint8_t* d_inf, size_t n, uint32_t precomp_c, hipStream_t stream) {
  MsmSlot& sl = ctx.msm_slots[slot];
  const MsmPlan p = msm_plan(n, group, precomp_c, msm_read_knobs());
  if (p.err != MSM_PLAN_OK) return hm_fail(p.err, p.err_msg);
  if (p.route == MSM_ROUTE_EMPTY) return HM_OK;
  if (p.route == MSM_ROUTE_SMALL) return msm_issue_small(ctx, slot, d_scalars_list, 1, d_xy, d_inf, n, p.c, stream);
  const MsmLaunch* const l = p.launch;
  const MsmWorkspace w{(uint8_t*)sl.ws.ensure(p.ws_bytes), p};
  if (!w.base) return hm_fail(HM_ERR_HIP, "msm: workspace allocation failed");
  int32_t* d_digits = w.at<int32_t>(MR_DIGITS);
  uint32_t *d_chist = w.at(MR_CHIST), *d_bcnt = w.at(MR_BCNT), *d_boff = w.at(MR_BOFF), *d_toff = w.at(MR_TOFF), *d_bsum = w.at(MR_BSUM);
  uint32_t *d_sorted = w.at(MR_SORTED), *d_tb = w.at(MR_TB), *d_torder = w.at(MR_TORDER), *d_khist = w.at(MR_TKEYS), *d_kcursor = d_khist + TASK_KEYS;
  uint32_t *d_partial = w.at(MR_PARTIAL), *d_bucket = w.at(MR_BUCKET), *d_seg = w.at(MR_SEG), *d_seg2 = w.at(MR_SEG2);
  uint32_t *d_tot = w.at(MR_RES), *d_win = d_tot + 4;       // per element: 4 totals words, then its records (one D2H copy)
  uint32_t *d_big_count = w.at(MR_BIG), *d_big_list = d_big_count + 4;
  uint2* d_slices = w.at<uint2>(MR_SLICES);
  // pair count for effective_task_len: the first sort level leaves it behind its region starts; an
  // input small enough to need no first level keeps the host's L
  const uint32_t* d_pairs = p.cb ? w.at(MR_CSTART) + (size_t)p.SW * p.NC : nullptr;
  const uint32_t NBT = p.NBT, L = p.L;

  int rc = ctx.msm_attr_set ? HM_OK : msm_set_lds_attributes();      // per device: a process may drive several GPUs
  if (rc == HM_OK) rc = msm_slot_prepare(sl);
  if (rc != HM_OK) return rc;
  ctx.msm_attr_set = true;
  hipEvent_t* ev = sl.ev;
  const bool k4_2d = p.reduction != MSM_RED_CHAIN, wide_items = p.item == MSM_ITEM_U64;
  // the host fold reads window sums, or the one-bit records of a shared set
  sl.describe(p.RW, p.c, p.W, group, p.res_stride, p.T_max, d_tot, k4_2d, msm_phase_timing(false));
  if (k4_2d) std::memset(sl.win_bits, 1, p.RW);
  sl.live_ptr = nullptr;                          // the general pipeline writes all over the workspace
  const bool pt = sl.phase_timed;
  HM_HIP_CHECK(hipEventRecord(ev[0], stream));

  // ---- K0: digits ----------------------------------------------------------------------------
  MsmGroupScalars list;
  for (uint32_t e = 0; e < (uint32_t)HM_MSM_GROUP; ++e) list.s[e] = d_scalars_list[e < group ? e : 0];
  if (p.digits == MSM_DIGITS_COUNTING)
    launch(msm_digits_kernel<true>, l[ML_DIGITS], stream, list, d_inf, d_digits, n, p.c, p.W, p.n_wide, d_chist, p.chunk, p.G, p.fb, p.NC);
  else
    launch(msm_digits_kernel<false>, l[ML_DIGITS], stream, list, d_inf, d_digits, n, p.c, p.W, p.n_wide, (uint32_t*)nullptr, (size_t)0, 0u, 0u, 0u);
  HM_HIP_CHECK(hipGetLastError());
  if (pt) HM_HIP_CHECK(hipEventRecord(ev[1], stream));

  // ---- K2: sort, scan, task order ------------------------------------------------------------
  launch(msm_init_counters_kernel, l[ML_INIT], stream, d_bcnt, (size_t)NBT, p.cb ? w.at(MR_BRCOUNT) : (uint32_t*)nullptr, d_khist, TASK_KEYS,
         d_big_count);
  HM_HIP_CHECK(hipGetLastError());
  wide_items ? launch_sort<uint64_t>(p, w, stream) : launch_sort<uint32_t>(p, w, stream);
  launch(msm_scan_partial_kernel, l[ML_SCAN_PARTIAL], stream, d_bcnt, d_bsum, NBT, d_pairs, L);
  launch(msm_scan_blocksums_kernel, l[ML_SCAN_BLOCKSUMS], stream, d_bsum, l[ML_SCAN_PARTIAL].gx, d_tot, (uint32_t)std::min<uint64_t>(p.T_max, 0xffffffffull));
  launch(msm_scan_final_kernel, l[ML_SCAN_FINAL], stream, d_bcnt, d_bsum, d_boff, d_toff, d_tot, NBT, d_pairs, L,
         p.coop_sort ? w.at(MR_GCUR) : (uint32_t*)nullptr);
  HM_HIP_CHECK(hipGetLastError());
  wide_items ? launch_sort_scatter<uint64_t>(p, w, stream) : launch_sort_scatter<uint32_t>(p, w, stream);
  // small inputs fill the task list in bucket order (three more launches cost more than the idle lanes they would save); else by length
  launch(msm_task_fill_kernel, l[ML_TASK_FILL], stream, d_toff, d_tb, d_torder, NBT, d_tot);
  launch(msm_task_hist_kernel, l[ML_TASK_HIST], stream, d_bcnt, NBT, d_pairs, L, d_khist);
  launch(msm_task_keyscan_kernel, l[ML_TASK_KEYSCAN], stream, d_khist, d_kcursor);
  launch(msm_task_order_kernel, l[ML_TASK_ORDER], stream, d_bcnt, d_toff, NBT, d_pairs, L, d_kcursor, d_tb, d_torder, d_tot);
  HM_HIP_CHECK(hipGetLastError());
  if (pt) HM_HIP_CHECK(hipEventRecord(ev[2], stream));

  // ---- K3: accumulate, then one point per bucket -----------------------------------------------
  // The exact task count T stays on the device (d_tot[1]); the grid covers its host-side bound (the plan's T_max): surplus
  // single-wave workgroups exit at once.
  if (pt) HM_HIP_CHECK(hipEventRecord(ev[5], stream));
  launch(msm_accumulate_kernel, l[ML_ACCUMULATE], stream, d_sorted, d_tb, d_torder, d_boff, d_bcnt, d_toff, d_xy, d_partial, d_tot, d_pairs, L);
  HM_HIP_CHECK(hipGetLastError());
  if (pt) HM_HIP_CHECK(hipEventRecord(ev[6], stream));
  launch(msm_bucket_finalize_kernel, l[ML_FINALIZE], stream, d_partial, d_toff, d_bucket, NBT, d_big_count, d_big_list, d_slices, d_tot,
         p.direct_buckets ? 1u : 0u);
  HM_HIP_CHECK(hipGetLastError());
  launch(msm_bucket_finalize_slices_kernel, l[ML_FINALIZE_SLICES], stream, d_partial, d_toff, d_big_count, d_slices);   // both stride over their queues
  launch(msm_bucket_finalize_big_kernel, l[ML_FINALIZE_BIG], stream, d_partial, d_toff, d_bucket, d_big_count, d_big_list);
  HM_HIP_CHECK(hipGetLastError());
  if (pt) HM_HIP_CHECK(hipEventRecord(ev[3], stream));

  // ---- K4: reduce ------------------------------------------------------------------------------
  if (k4_2d) {     // a shared bucket set: row / column sums, then one record per weight bit
    const uint32_t* rd_partial = p.direct_buckets ? d_partial : nullptr;
    const uint32_t* rd_toff = p.direct_buckets ? d_toff : nullptr;
    if (p.reduction == MSM_RED_ROWCOL_WAVE)
      launch(msm_reduce_rowcol_wave_kernel, l[ML_ROWCOL], stream, d_bucket, d_seg, p.k4_m, p.k4_h, rd_partial, rd_toff, d_tot);
    else
      launch(msm_reduce_rowcol_kernel, l[ML_ROWCOL], stream, d_bucket, d_seg, p.k4_m, p.k4_h, rd_partial, rd_toff, d_tot);
    launch(msm_reduce_bits_kernel, l[ML_BITS], stream, d_seg, p.k4_m, p.k4_h, d_win, p.res_stride);
  } else {         // a bucket set per window: running sums per segment, then sums of the segments' points
    launch(msm_reduce_segments_kernel, l[ML_SEGMENTS], stream, d_bucket, d_seg, p.SW, p.NB, p.NBP, p.SEG, p.nseg);
    uint32_t *cur = d_seg, *nxt = d_seg2;
    for (uint32_t lv = 0; lv < p.sum_levels; ++lv, std::swap(cur, nxt))
      launch(msm_sum_points_kernel, l[ML_SUM_0 + lv], stream, cur, p.sum_count[lv], nxt, l[ML_SUM_0 + lv].gx);
    launch(msm_windows_to_ext_kernel, l[ML_TO_EXT], stream, cur, p.SW, d_win);
  }
  HM_HIP_CHECK(hipGetLastError());
  // pinned landing zone, so that this copy (and therefore msm_enqueue) does not wait for the device
  HM_HIP_CHECK(hipMemcpyAsync(sl.totals(), d_tot, p.region[MR_RES].bytes, hipMemcpyDeviceToHost, stream));
  HM_HIP_CHECK(hipEventRecord(ev[4], stream));
  return HM_OK;
}

uint32_t msm_table_group_max(size_t n, uint32_t precomp_c) { return plan_table_group_max(n, precomp_c); }
int msm_enqueue_table_group(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                            const uint8_t* d_inf, size_t n, uint32_t precomp_c, hipStream_t stream) {
  MsmSlot& sl = ctx.msm_slots[slot];
  if (group == 0 || group > msm_table_group_max(n, precomp_c)) return hm_fail(HM_ERR_INTERNAL, "msm: table group larger than the plan allows");
  sl.n = n;
  sl.stream = stream;
  sl.group = 1;
  if (n == 0) return HM_OK;
  return msm_issue(ctx, slot, d_scalars_list, group, d_xy, d_inf, n, precomp_c, stream);
}

int msm_enqueue(DeviceCtx& ctx, int slot, const uint32_t* d_scalars_ext, const uint32_t* d_xy, const uint8_t* d_inf, size_t n,
                uint32_t precomp_c, hipStream_t stream) {
  return msm_enqueue_table_group(ctx, slot, &d_scalars_ext, 1, d_xy, d_inf, n, precomp_c, stream);      // a group of one, on either layout
}

// the five-launch chain's window for n points sized for `live_rows` of them, or 0 when that chain does not apply (msm_plan.inc)
static uint32_t small_plan_window(size_t n, uint32_t precomp_c, size_t live_rows = 0) {
  return plan_small_window(n, precomp_c, live_rows, msm_read_knobs(true));
}
bool msm_group_applies(size_t n, uint32_t precomp_c) { return small_plan_window(n, precomp_c) != 0; }

// `group` MSMs over the same n points through ONE launch chain (msm_small.hip); the slot then carries `group` results.
int msm_enqueue_group(DeviceCtx& ctx, int slot, const uint32_t* const* d_scalars_list, uint32_t group, const uint32_t* d_xy,
                      const uint8_t* d_inf, size_t n, hipStream_t stream, size_t live_rows) {
  MsmSlot& sl = ctx.msm_slots[slot];
  const uint32_t c = small_plan_window(n, 0, live_rows);
  if (!c) return hm_fail(HM_ERR_INTERNAL, "msm: a group needs the five-launch plan");
  sl.n = n;
  sl.stream = stream;
  return msm_issue_small(ctx, slot, d_scalars_list, group, d_xy, d_inf, n, c, stream);
}

// Wait for the slot's chain and fold the window sums of each of its MSMs (host Horner + affine normalisation).  Touches
// only the slot: a busy slot is not handed out again, so this part runs without the context lock.
int msm_finish_wait_fold(MsmSlot& sl, uint64_t* out_jac_ext, int* out_is_identity, double* host_us) {
  *host_us = 0;
  if (sl.n == 0) {
    std::memset(out_jac_ext, 0, 96);
    *out_is_identity = 1;
    return HM_OK;
  }
  HM_HIP_CHECK(hipEventSynchronize(sl.ev[4]));
  const auto f0 = std::chrono::steady_clock::now();
  for (uint32_t e = 0; e < sl.group; ++e) {
    const uint32_t* land = sl.h_land + (size_t)e * sl.res_stride;      // group == 1: res_stride is not used
    if (land[2] != 0) return hm_fail(HM_ERR_INTERNAL, "msm: task count exceeds its bound");
    host_fold(land + 4, sl.SW, sl.c, out_jac_ext + 12 * e, out_is_identity + e, sl.balanced ? sl.win_bits : nullptr);   // SW == 1: just the normalisation
  }
  *host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - f0).count();
  return HM_OK;
}

// statistics of the MSM just finished on `slot` (ctx.mu held)
void msm_finish_record(DeviceCtx& ctx, int slot, double host_us) {
  MsmSlot& sl = ctx.msm_slots[slot];
  if (sl.n == 0) return;
  ctx.calls.msm_host_us += host_us;
  hipEvent_t* ev = sl.ev;
  float ms[4] = {0, 0, 0, 0}, total = 0, acc_kernel = 0;
  (void)hipEventElapsedTime(&total, ev[0], ev[4]);
  if (sl.phase_timed) {
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    (void)hipEventElapsedTime(&acc_kernel, ev[5], ev[6]);
  }
  ctx.last_msm.t_accum_kernel_ms = acc_kernel;
  ctx.last_msm.t_digits_ms = ms[0];
  ctx.last_msm.t_sort_ms = ms[1];
  ctx.last_msm.t_accum_ms = ms[2];
  ctx.last_msm.t_reduce_ms = ms[3];
  ctx.last_msm.t_total_ms = total;
  ctx.last_msm.pairs = sl.totals()[0];
  ctx.last_msm.tasks = sl.totals()[1];
  ctx.last_msm.c = sl.c;
  ctx.last_msm.windows = sl.W;
}

int msm_finish(DeviceCtx& ctx, int slot, uint64_t out_jac_ext[12], int* out_is_identity) {
  double host_us = 0;
  const int rc = msm_finish_wait_fold(ctx.msm_slots[slot], out_jac_ext, out_is_identity, &host_us);
  if (rc == HM_OK) msm_finish_record(ctx, slot, host_us);
  else ctx.msm_slots[slot].live_ptr = nullptr;     // a chain that failed may have left its block counters anywhere
  return rc;
}

// the synchronous form: slot 0, enqueue then finish
int msm_run(DeviceCtx& ctx, const uint32_t* d_scalars_ext, const uint32_t* d_xy, const uint8_t* d_inf, size_t n,
            uint32_t precomp_c, uint64_t out_jac_ext[12], int* out_is_identity, hipStream_t stream) {
  if (ctx.msm_slots[0].busy) return hm_fail(HM_ERR_BAD_ARG, "msm: slot 0 is held by an un-awaited hm_msm_submit_dev ticket");
  const int rc = msm_enqueue(ctx, 0, d_scalars_ext, d_xy, d_inf, n, precomp_c, stream);
  if (rc != HM_OK) return rc;
  return msm_finish(ctx, 0, out_jac_ext, out_is_identity);
}

int g1_fixed_base_mul_run(DeviceCtx& ctx, const uint32_t* d_scalars_ext, size_t n, const uint64_t base_affine_ext[8],
                          uint32_t* d_out_affine_ext, hipStream_t stream) {
  if (n == 0) return HM_OK;
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {      // the multiples table is per stream in use
    uint32_t* d_table = (uint32_t*)aux_buffer(slot, AuxBuf::table, HM_AUX_TABLE_MIN, "fixed-base");
    if (!d_table) return HM_ERR_HIP;
    G1AffineWords base;
    std::memcpy(base.w, base_affine_ext, 64);
    hipLaunchKernelGGL(g1_fixed_table_kernel, dim3(1), dim3(64), 0, stream, base, d_table);
    HM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(g1_fixed_base_mul_kernel, dim3((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0,
                       stream, d_scalars_ext, (const uint32_t*)d_table, d_out_affine_ext, n);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

}  // namespace hm
