// Microbenchmark: forms of the 9 x 29-bit Montgomery product (csrc/ff29.h) by how the limb carries
// travel.  Dependent products per lane, occupancy forced to 4 waves per SIMD (the bucket accumulation
// kernel's) and to 8 by dynamic LDS, all 256 CUs filled.  Not part of the product path.
//
//   a  operand scanning, carries added with a 64-bit add per round / per output limb (ff29.h's single products)
//   b  product scanning, the carry starts the next column's mad chain; every accumulation and shift is
//      pinned with an empty asm so that the compiler cannot move the carry to the end of the sum again
//   c  form b on two independent products advanced in lockstep (ff29.h's fe_mul_x2: what profiles/r07_a_mont_forms.txt chose)
//   d  product scanning with the wide mad itself inside the asm statement (one chain)
//   e  form d on two independent products in lockstep
//   f  form d with up to three mads per asm statement (one chain)
//   h  form d with each column's mads in two asm statements (the a*b terms, then the m*p terms)
//   g  the column-wise source with nothing pinned: what the compiler makes of it on its own
//
// Every form is checked against form a on the device before it is timed (bit-identical limbs).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/ubench/mont_forms.hip -o mont_forms && ./mont_forms
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../halo2-experiments_amd/csrc/g1.h"

using namespace hm;

constexpr int ITERS = 8192;  // products per lane and launch (even): ~50 ms per launch at 4 waves per SIMD

// ---- a: operand scanning --------------------------------------------------------------------
template <class F>
__device__ __forceinline__ Fe<F> mul_opscan(const Fe<F>& a, const Fe<F>& b) {
  uint64_t t[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)a.l[j] * b.l[i];
    const uint32_t m = ((uint32_t)t[0] * F::INV29) & MASK29;
#pragma unroll
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)m * F::MOD[j];
    t[1] += t[0] >> 29;
#pragma unroll
    for (int j = 0; j < 9; ++j) t[j] = t[j + 1];
    t[9] = 0;
  }
  Fe<F> r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    r.l[j] = (uint32_t)t[j] & MASK29;
    t[j + 1] += t[j] >> 29;
  }
  r.l[8] = (uint32_t)t[8];
  return r;
}

// ---- how one accumulation step is written ----------------------------------------------------
struct Plain {  // what the compiler makes of the column-wise source on its own
  static __device__ __forceinline__ void mad(uint64_t& acc, uint32_t x, uint32_t y) { acc += (uint64_t)x * y; }
  static __device__ __forceinline__ void madc(uint64_t& acc, uint32_t x, uint32_t k) { acc += (uint64_t)x * k; }
  static __device__ __forceinline__ void shr(uint64_t& acc) { acc >>= 29; }
};
struct Pinned {
  static __device__ __forceinline__ void mad(uint64_t& acc, uint32_t x, uint32_t y) {
    acc += (uint64_t)x * y;
    asm("" : "+v"(acc));
  }
  static __device__ __forceinline__ void madc(uint64_t& acc, uint32_t x, uint32_t k) { mad(acc, x, k); }
  static __device__ __forceinline__ void shr(uint64_t& acc) {
    acc >>= 29;
    asm("" : "+v"(acc));
  }
};
struct AsmMad {
  static __device__ __forceinline__ void mad(uint64_t& acc, uint32_t x, uint32_t y) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y) : "vcc");
  }
  static __device__ __forceinline__ void madc(uint64_t& acc, uint32_t x, uint32_t k) {  // k: a modulus limb, wave-uniform
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "s"(k) : "vcc");
  }
  static __device__ __forceinline__ void shr(uint64_t& acc) { acc >>= 29; }
};

// ---- b / d: product scanning, one chain --------------------------------------------------------
template <class P, class F>
__device__ __forceinline__ Fe<F> mul_colscan(const Fe<F>& a, const Fe<F>& b) {
  uint64_t acc = 0;
  uint32_t m[9];
  Fe<F> r;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
#pragma unroll
    for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); ++i) P::mad(acc, a.l[i], b.l[k - i]);
#pragma unroll
    for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k - 1 : 8); ++i) P::madc(acc, m[i], F::MOD[k - i]);
    if (k < 9) {
      m[k] = ((uint32_t)acc * F::INV29) & MASK29;
      P::madc(acc, m[k], F::MOD[0]);
    } else {
      r.l[k - 9] = (uint32_t)acc & MASK29;
    }
    P::shr(acc);
  }
  r.l[8] = (uint32_t)acc;
  return r;
}

// ---- c / e: two independent products in lockstep ------------------------------------------------
template <class P, class F>
__device__ __forceinline__ void mul_colscan_x2(Fe<F>& r0, Fe<F>& r1, const Fe<F>& a0, const Fe<F>& b0, const Fe<F>& a1,
                                               const Fe<F>& b1) {
  uint64_t acc0 = 0, acc1 = 0;
  uint32_t m0[9], m1[9];
  Fe<F> o0, o1;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
#pragma unroll
    for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); ++i) {
      P::mad(acc0, a0.l[i], b0.l[k - i]);
      P::mad(acc1, a1.l[i], b1.l[k - i]);
    }
#pragma unroll
    for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k - 1 : 8); ++i) {
      P::madc(acc0, m0[i], F::MOD[k - i]);
      P::madc(acc1, m1[i], F::MOD[k - i]);
    }
    if (k < 9) {
      m0[k] = ((uint32_t)acc0 * F::INV29) & MASK29;
      m1[k] = ((uint32_t)acc1 * F::INV29) & MASK29;
      P::madc(acc0, m0[k], F::MOD[0]);
      P::madc(acc1, m1[k], F::MOD[0]);
    } else {
      o0.l[k - 9] = (uint32_t)acc0 & MASK29;
      o1.l[k - 9] = (uint32_t)acc1 & MASK29;
    }
    P::shr(acc0);
    P::shr(acc1);
  }
  o0.l[8] = (uint32_t)acc0;
  o1.l[8] = (uint32_t)acc1;
  r0 = o0;
  r1 = o1;
}

// ---- f: form d with three mads per asm statement where the column has them -------------------------
struct AsmMad3 {
  static __device__ __forceinline__ void mad3(uint64_t& acc, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t x2,
                                              uint32_t y2) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_mad_u64_u32 %0, vcc, %5, %6, %0"
        : "+v"(acc)
        : "v"(x0), "v"(y0), "v"(x1), "v"(y1), "v"(x2), "v"(y2)
        : "vcc");
  }
};

template <class F>
__device__ __forceinline__ Fe<F> mul_colscan3(const Fe<F>& a, const Fe<F>& b) {
  uint64_t acc = 0;
  uint32_t m[9];
  Fe<F> r;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
    const int lo = k > 8 ? k - 8 : 0, hi = k < 8 ? k : 8;
    int i = lo;
#pragma unroll
    for (; i + 2 <= hi; i += 3) AsmMad3::mad3(acc, a.l[i], b.l[k - i], a.l[i + 1], b.l[k - i - 1], a.l[i + 2], b.l[k - i - 2]);
#pragma unroll
    for (; i <= hi; ++i) AsmMad::mad(acc, a.l[i], b.l[k - i]);
#pragma unroll
    for (int j = lo; j <= (k < 8 ? k - 1 : 8); ++j) AsmMad::madc(acc, m[j], F::MOD[k - j]);
    if (k < 9) {
      m[k] = ((uint32_t)acc * F::INV29) & MASK29;
      AsmMad::madc(acc, m[k], F::MOD[0]);
    } else {
      r.l[k - 9] = (uint32_t)acc & MASK29;
    }
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}

// ---- h: form d with each column's mads in two asm statements (a*b, then m*p) ----------------------
#define HM_MAD(x, y) "v_mad_u64_u32 %0, vcc, %" #x ", %" #y ", %0\n\t"
#define HM_OPS(c, i) "v"(x[i]), c(y[-(i)])
#define HM_MADS_BODY(c)                                                                                                      \
  if constexpr (N == 1) asm(HM_MAD(1, 2) : "+v"(acc) : HM_OPS(c, 0) : "vcc");                                                \
  if constexpr (N == 2) asm(HM_MAD(1, 2) HM_MAD(3, 4) : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1) : "vcc");                     \
  if constexpr (N == 3) asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2) : "vcc"); \
  if constexpr (N == 4)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3) : "vcc"); \
  if constexpr (N == 5)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) HM_MAD(9, 10)                                                    \
        : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3), HM_OPS(c, 4) : "vcc");                         \
  if constexpr (N == 6)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) HM_MAD(9, 10) HM_MAD(11, 12)                                     \
        : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3), HM_OPS(c, 4), HM_OPS(c, 5) : "vcc");           \
  if constexpr (N == 7)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) HM_MAD(9, 10) HM_MAD(11, 12) HM_MAD(13, 14)                      \
        : "+v"(acc) : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3), HM_OPS(c, 4), HM_OPS(c, 5), HM_OPS(c, 6) : "vcc"); \
  if constexpr (N == 8)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) HM_MAD(9, 10) HM_MAD(11, 12) HM_MAD(13, 14) HM_MAD(15, 16)       \
        : "+v"(acc)                                                                                                          \
        : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3), HM_OPS(c, 4), HM_OPS(c, 5), HM_OPS(c, 6), HM_OPS(c, 7) : "vcc"); \
  if constexpr (N == 9)                                                                                                      \
    asm(HM_MAD(1, 2) HM_MAD(3, 4) HM_MAD(5, 6) HM_MAD(7, 8) HM_MAD(9, 10) HM_MAD(11, 12) HM_MAD(13, 14) HM_MAD(15, 16) HM_MAD(17, 18) \
        : "+v"(acc)                                                                                                          \
        : HM_OPS(c, 0), HM_OPS(c, 1), HM_OPS(c, 2), HM_OPS(c, 3), HM_OPS(c, 4), HM_OPS(c, 5), HM_OPS(c, 6), HM_OPS(c, 7), HM_OPS(c, 8) \
        : "vcc");

// acc += x[0]*y[0] + x[1]*y[-1] + ... (N terms); y in VGPRs / y a run of modulus limbs (wave-uniform constants)
template <int N>
__device__ __forceinline__ void mads_vv(uint64_t& acc, const uint32_t* x, const uint32_t* y) {
  HM_MADS_BODY("v")
}
template <int N>
__device__ __forceinline__ void mads_vs(uint64_t& acc, const uint32_t* x, const uint32_t* y) {
  HM_MADS_BODY("s")
}
#undef HM_MADS_BODY
#undef HM_OPS
#undef HM_MAD

template <int K, class F>
__device__ __forceinline__ void colasm_column(uint64_t& acc, uint32_t (&m)[9], Fe<F>& r, const Fe<F>& a, const Fe<F>& b) {
  constexpr int lo = K > 8 ? K - 8 : 0, hi = K < 8 ? K : 8, mhi = K < 8 ? K - 1 : 8;
  mads_vv<hi - lo + 1>(acc, &a.l[lo], &b.l[K - lo]);
  if constexpr (mhi >= lo) mads_vs<mhi - lo + 1>(acc, &m[lo], &F::MOD[K - lo]);
  if constexpr (K < 9) {
    m[K] = ((uint32_t)acc * F::INV29) & MASK29;
    AsmMad::madc(acc, m[K], F::MOD[0]);
  } else {
    r.l[K - 9] = (uint32_t)acc & MASK29;
  }
  acc >>= 29;
}
template <class F, int... Ks>
__device__ __forceinline__ Fe<F> mul_colasm_seq(const Fe<F>& a, const Fe<F>& b, std::integer_sequence<int, Ks...>) {
  uint64_t acc = 0;
  uint32_t m[9];
  Fe<F> r;
  (colasm_column<Ks>(acc, m, r, a, b), ...);
  r.l[8] = (uint32_t)acc;
  return r;
}
template <class F>
__device__ __forceinline__ Fe<F> mul_colasm(const Fe<F>& a, const Fe<F>& b) {
  return mul_colasm_seq(a, b, std::make_integer_sequence<int, 17>{});
}

// ---- kernels --------------------------------------------------------------------------------------
constexpr bool is_lockstep(int form) { return form == 2 || form == 4; }

template <int FORM>
__device__ __forceinline__ Fq mul1(const Fq& x, const Fq& b) {
  if constexpr (FORM == 0) return mul_opscan(x, b);
  if constexpr (FORM == 1) return mul_colscan<Pinned>(x, b);
  if constexpr (FORM == 3) return mul_colscan<AsmMad>(x, b);
  if constexpr (FORM == 5) return mul_colscan3(x, b);
  if constexpr (FORM == 6) return mul_colscan<Plain>(x, b);
  if constexpr (FORM == 7) return mul_colasm(x, b);
}
template <int FORM>
__device__ __forceinline__ void mul_pair(Fq& x0, Fq& x1, const Fq& b) {  // x0 *= b, x1 *= b
  if constexpr (FORM == 2) mul_colscan_x2<Pinned>(x0, x1, x0, b, x1, b);
  else if constexpr (FORM == 4) mul_colscan_x2<AsmMad>(x0, x1, x0, b, x1, b);
  else { x0 = mul1<FORM>(x0, b); x1 = mul1<FORM>(x1, b); }
}

// CHECK: both chains advance by `iters` products in every form (the same values whatever the form).
// Timing: the single-chain forms run ONE chain of `iters` dependent products, the lockstep forms two chains of
// iters / 2; either way a lane does `iters` products.
template <int FORM, int WAVES, bool CHECK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void forms_kernel(uint32_t* out, uint32_t seed,
                                                                                                       int iters) {
  extern __shared__ uint32_t occupancy_pad[];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Fq x0, x1, b;
  for (int i = 0; i < 9; ++i) {
    x0.l[i] = (seed + t * 31 + i * 7) & MASK29;
    x1.l[i] = (seed * 3 + t * 13 + i * 11) & MASK29;
    b.l[i] = (seed * 5 + t * 17 + i * 3) & MASK29;
  }
  x0.l[8] &= 0xFFFF;
  x1.l[8] &= 0xFFFF;
  b.l[8] &= 0xFFFF;
  if constexpr (CHECK) {
    for (int it = 0; it < iters; ++it) mul_pair<FORM>(x0, x1, b);
  } else if constexpr (is_lockstep(FORM)) {
    for (int it = 0; it < iters; it += 2) mul_pair<FORM>(x0, x1, b);
  } else {
    for (int it = 0; it < iters; ++it) x0 = mul1<FORM>(x0, b);
  }
  if (seed == 0xFFFFFFFFu) occupancy_pad[threadIdx.x] = t;  // keeps the dynamic LDS referenced
  for (int i = 0; i < 9; ++i) out[(size_t)t * 18 + i] = x0.l[i];
  for (int i = 0; i < 9; ++i) out[(size_t)t * 18 + 9 + i] = x1.l[i];
}

template <int FORM, int WAVES, bool CHECK>
static double run_once(uint32_t* d_out, int blocks, int iters, hipEvent_t e0, hipEvent_t e1) {
  const size_t lds = (size_t)(160 * 1024) / WAVES - 1024;  // WAVES blocks of 4 waves fit one CU's 160 KB, one more does not
  (void)hipFuncSetAttribute((const void*)forms_kernel<FORM, WAVES, CHECK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  float ms = 0;
  (void)hipEventRecord(e0, 0);
  hipLaunchKernelGGL((forms_kernel<FORM, WAVES, CHECK>), dim3(blocks), dim3(256), lds, 0, d_out, 12345u, iters);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  (void)hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

static const char* NAMES[] = {"a opscan", "b pinned colscan", "c pinned lockstep x2", "d asm-mad colscan", "e asm-mad lockstep x2",
                              "f asm-mad3 colscan", "g plain colscan", "h asm-column colscan"};

template <int FORM, int WAVES>
static bool bench(uint32_t* d_out, std::vector<uint32_t>& ref, int check_blocks, hipEvent_t e0, hipEvent_t e1) {
  // correctness first, on a small grid: limbs bit-identical to form a's
  std::vector<uint32_t> got((size_t)check_blocks * 256 * 18);
  run_once<FORM, WAVES, true>(d_out, check_blocks, 8, e0, e1);
  if (hipMemcpy(got.data(), d_out, got.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (FORM == 0 && WAVES == 4) ref = got;
  if (got != ref) {
    printf("%-24s waves/SIMD=%d  MISMATCH against form a\n", NAMES[FORM], WAVES);
    return false;
  }
  const int blocks = 256 * WAVES * 4;  // four full rounds of the machine
  run_once<FORM, WAVES, false>(d_out, blocks, ITERS, e0, e1);
  std::vector<double> ms;
  for (int rep = 0; rep < 5; ++rep) ms.push_back(run_once<FORM, WAVES, false>(d_out, blocks, ITERS, e0, e1));
  std::sort(ms.begin(), ms.end());
  const double products = (double)blocks * 256 * ITERS;
  printf("%-24s waves/SIMD=%d  median %.3f ms  min %.3f  max %.3f  spread %.2f%%  %.4e products/s\n", NAMES[FORM], WAVES, ms[2], ms[0],
         ms[4], (ms[4] - ms[0]) / ms[2] * 100.0, products / ms[2] * 1e3);
  return true;
}

template <int WAVES>
static bool bench_all(uint32_t* d_out, std::vector<uint32_t>& ref, hipEvent_t e0, hipEvent_t e1) {
  bool ok = true;
  ok &= bench<0, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<1, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<2, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<3, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<4, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<5, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<6, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<7, WAVES>(d_out, ref, 8, e0, e1);
  ok &= bench<0, WAVES>(d_out, ref, 8, e0, e1);  // form a again: its drift over the session
  return ok;
}

int main() {
  uint32_t* d_out = nullptr;
  if (hipMalloc(&d_out, (size_t)256 * 8 * 4 * 256 * 18 * 4) != hipSuccess) {
    printf("no device memory\n");
    return 2;
  }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  std::vector<uint32_t> ref;
  bool ok = bench_all<4>(d_out, ref, e0, e1);
  ok &= bench_all<8>(d_out, ref, e0, e1);
  (void)hipFree(d_out);
  return ok ? 0 : 1;
}
