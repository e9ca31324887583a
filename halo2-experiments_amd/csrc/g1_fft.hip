// g1_fft.hip -- best_fft over BN256 G1 (g_to_lagrange / ParamsKZG::downsize) and, on its twiddle, stage and store kernels, all KZG
// openings of a polynomial on its domain (FK20, further down): the kernels and the drivers g1_fft_run, kzg_open_table_run and
// kzg_open_all_run.
//
//   a[i] <- sum_j [omega^(ij)] a[j], then optionally a[i] <- [scale] a[i]   
//
// Iterative radix-2 decimation in time on a Jacobian working buffer (PT_WORDS records, internal ff29 form, identity flag):
// the load kernel writes point i to slot bitrev(i); stage s (half-size m = 2^s) runs n / 2 butterflies
//     t = [omega^(j n / 2m)] v,   (u, v) <- (u + t, u - t)
// with the complete g1_add / g1_double (t == u, t == -u and identity operands all occur), and the store kernel applies the
// scale, normalises with one Fermat inversion per point and writes the caller's layout.
//
// Twiddle uniformity: a stage has m distinct twiddles, each shared by n / 2m butterflies.  While n / 2m >= 64 the
// butterflies of one twiddle are laid along the lanes of a wavefront (G1_FFT_UNIFORM): the twiddle words are read with
// readfirstlane, the double-and-add's bit tests are scalar branches, and a lane adds only where the twiddle has a one bit
// (~127 additions per 254 doublings).  The last six stages (n / 2m < 64) have a twiddle per lane; they run the same loop with
// lane-divergent bit tests, where some lane of the wave almost always has a one, so every bit costs an addition (~1.5x the
// uniform butterfly).  A four-step split would make those stages uniform too; at 2^18..2^24 they are 6 of 18..24 stages.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "fq_inverse.h"
#include "g1_mul.h"
#include "hm_internal.h"
#include "host_fr.h"
#include "msm_dev.h"

namespace hm {

constexpr uint32_t G1_FFT_LOG_MAX = 24;

// g1_mul_words, the double-and-add of every product below, is g1_mul.h's (the per-proof sums of verify.hip run its twin there)

// -P: Y -> 6p - Y (Y < 5p, normalised limbs), brought back under 3p so that the point stays inside the Jacobian class
__device__ __forceinline__ G1Jac g1_neg(const G1Jac& p) {
  G1Jac r = p;
  r.y = fe_reduce_small(fe_norm(fe_sub<6, 29>(fe_zero<FqParams>(), p.y)));
  return r;
}

__device__ __forceinline__ uint32_t g1_fft_bitrev(uint32_t i, uint32_t log_n) {
  return log_n == 0 ? 0u : __brev(i) >> (32 - log_n);
}

// Twiddle table: external Montgomery words of omega^j (fr_powers_run) -> the canonical integers, in place (m entries of 8 words)
__global__ void g1_fft_twiddle_kernel(uint32_t* __restrict__ tw, size_t m) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint4* q = reinterpret_cast<uint4*>(tw + i * 8);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  Fr k32 = fe_zero<FrParams>();
  k32.l[0] = 32;
  uint32_t v[8];
  fe_pack(v, fe_canonical(fe_mul(fe_unpack<FrParams>(w), k32)));   // (x 2^256) * 32 * 2^-261 = x
  q[0] = make_uint4(v[0], v[1], v[2], v[3]);
  q[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// caller's points -> working buffer, slot bitrev(i).  WORDS = 16: affine (x, y), (0, 0) = identity; WORDS = 24: Jacobian
// (x, y, z), z = 0 = identity.  u32 words of external Montgomery coordinates.
template <int WORDS>
__global__ __launch_bounds__(ACC_THREADS) void g1_fft_load_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ work,
                                                                  uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(in + i * WORDS);
  uint32_t w[WORDS];
#pragma unroll
  for (int k = 0; k < WORDS / 4; ++k) {
    const uint4 v = q[k];
    w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
  }
  uint32_t wx[8], wy[8], any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    wx[k] = w[k];
    wy[k] = w[8 + k];
    any |= WORDS == 16 ? (wx[k] | wy[k]) : w[16 + k];
  }
  G1Jac p;
  p.x = fe_from_ext<FqParams>(wx);
  p.y = fe_from_ext<FqParams>(wy);
  if (WORDS == 16) {
    p.z = fe_one<FqParams>();
  } else {
    uint32_t wz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wz[k] = w[16 + k];
    p.z = fe_from_ext<FqParams>(wz);
  }
  p.inf = any == 0;
  if (p.inf) p = g1_identity();
  store_jac(work + (size_t)g1_fft_bitrev((uint32_t)i, log_n) * PT_WORDS, p);
}

// one radix-2 stage, half-size m = 2^s; thread t < n / 2 is one butterfly.  UNIFORM (n / 2m >= 64): t = j * (n / 2m) + b, so
// the 64 lanes of a wave share j; otherwise t = b * m + j (consecutive lanes, consecutive twiddles).
template <bool UNIFORM>
__global__ __launch_bounds__(ACC_THREADS) void g1_fft_stage_kernel(uint32_t* __restrict__ work, const uint32_t* __restrict__ tw,
                                                                   uint32_t log_n, uint32_t s) {
  const size_t t = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (t >= ((size_t)1 << (log_n - 1))) return;
  const uint32_t lb = log_n - 1 - s;                  // log2(n / 2m): butterflies per twiddle
  size_t j, b;
  if (UNIFORM) {
    j = t >> lb;
    b = t & (((size_t)1 << lb) - 1);
  } else {
    j = t & (((size_t)1 << s) - 1);
    b = t >> s;
  }
  const size_t lo = (b << (s + 1)) + j, hi = lo + ((size_t)1 << s);
  const uint4* q = reinterpret_cast<const uint4*>(tw + (j << lb) * 8);   // omega^(j n / 2m), index < n / 2
  const uint4 e0 = q[0], e1 = q[1];
  uint32_t e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
  if (UNIFORM) {
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = __builtin_amdgcn_readfirstlane(e[k]);
  }
  const G1Jac tv = g1_mul_words(load_jac(work + hi * PT_WORDS), e);
  const G1Jac u = load_jac(work + lo * PT_WORDS);
  store_jac(work + lo * PT_WORDS, g1_add(u, tv));
  store_jac(work + hi * PT_WORDS, g1_add(u, g1_neg(tv)));
}

struct G1FftScale {        // canonical integer of the optional scale, by value (constant indices only: scalar loads)
  uint32_t w[8];
  uint32_t on;
};

// working buffer -> caller's layout in natural order, [scale] applied: WORDS = 16 affine (0, 0) for the identity, WORDS = 24
// (x, y, 1) / all zero (hm_msm_bn256_g1_jacobian's form).  One Fermat inversion per point.
template <int WORDS>
__global__ __launch_bounds__(ACC_THREADS) void g1_fft_store_kernel(const uint32_t* __restrict__ work, uint32_t* __restrict__ out,
                                                                   uint32_t log_n, G1FftScale scale) {
  const size_t n = (size_t)1 << log_n;
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n) return;
  G1Jac p = load_jac(work + i * PT_WORDS);
  if (scale.on) {
    uint32_t e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = scale.w[k];
    p = g1_mul_words(p, e);
  }
  uint32_t w[24];
#pragma unroll
  for (int k = 0; k < 24; ++k) w[k] = 0;
  if (!p.inf) {
    const Fq zi = fq_inverse(p.z);
    const Fq zi2 = fe_sqr(zi);
    const Fq zi3 = fe_mul(zi2, zi);
    uint32_t ox[8], oy[8], oz[8];
    fe_to_ext(ox, fe_mul(p.x, zi2));
    fe_to_ext(oy, fe_mul(p.y, zi3));
    fe_to_ext(oz, fe_one<FqParams>());
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      w[k] = ox[k];
      w[8 + k] = oy[k];
      w[16 + k] = oz[k];
    }
  }
  uint4* o = reinterpret_cast<uint4*>(out + i * WORDS);
#pragma unroll
  for (int k = 0; k < WORDS / 4; ++k) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// best_fft over G1, in place on `d_points`: WORDS = 16 u32 per point (affine external, (0, 0) = identity) or 24
// (Jacobian external, z = 0 = identity; written back as (x, y, 1) / zeros).  The working buffer (n Jacobian records) and the
// twiddle table (n / 2 canonical omega^j) are allocated per call, stream-ordered on `stream`, and freed behind the last kernel.
int g1_fft_run(DeviceCtx& ctx, uint32_t* d_points, uint32_t words, const uint64_t omega_ext[4], uint32_t log_n,
               const uint64_t* scale_ext, hipStream_t stream) {
  (void)ctx;
  if (log_n > G1_FFT_LOG_MAX) return hm_fail(HM_ERR_BAD_ARG, "g1_fft: log_n > 24");
  if (words != 16 && words != 24) return hm_fail(HM_ERR_BAD_ARG, "g1_fft: point layout must be 16 or 24 words");
  const size_t n = (size_t)1 << log_n, half = n / 2;
  G1FftScale scale{};
  if (scale_ext) {
    const host::Fr4 one_int = {{1, 0, 0, 0}};
    const host::Fr4 v = host::fr_mul(host::fr_load(scale_ext), one_int);    // Montgomery words -> canonical integer
    std::memcpy(scale.w, v.l, 32);
    scale.on = 1;
  }
  const size_t work_bytes = n * PT_WORDS * 4, tw_bytes = half * 32;
  return stream_scratch("g1_fft", work_bytes + tw_bytes, stream, [&](uint8_t* mem) -> int {
    uint32_t *work = (uint32_t*)mem, *tw = work + n * PT_WORDS;
    const dim3 all((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS)), pairs((uint32_t)((half + ACC_THREADS - 1) / ACC_THREADS));
    int rc = HM_OK;
    if (half) {
      rc = fr_powers_run(tw, half, omega_ext, stream);
      if (rc == HM_OK) {
        hipLaunchKernelGGL(g1_fft_twiddle_kernel, dim3((uint32_t)((half + 255) / 256)), dim3(256), 0, stream, tw, half);
        if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "g1_fft: twiddle kernel launch failed");
      }
    }
    if (rc == HM_OK) {
      if (words == 16) hipLaunchKernelGGL(g1_fft_load_kernel<16>, all, dim3(ACC_THREADS), 0, stream, d_points, work, log_n);
      else hipLaunchKernelGGL(g1_fft_load_kernel<24>, all, dim3(ACC_THREADS), 0, stream, d_points, work, log_n);
      if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "g1_fft: load kernel launch failed");
    }
    for (uint32_t s = 0; rc == HM_OK && s < log_n; ++s) {
      if (log_n - 1 - s >= 6) hipLaunchKernelGGL(g1_fft_stage_kernel<true>, pairs, dim3(ACC_THREADS), 0, stream, work, tw, log_n, s);
      else hipLaunchKernelGGL(g1_fft_stage_kernel<false>, pairs, dim3(ACC_THREADS), 0, stream, work, tw, log_n, s);
      if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "g1_fft: stage kernel launch failed");
    }
    if (rc == HM_OK) {
      if (words == 16) hipLaunchKernelGGL(g1_fft_store_kernel<16>, all, dim3(ACC_THREADS), 0, stream, work, d_points, log_n, scale);
      else hipLaunchKernelGGL(g1_fft_store_kernel<24>, all, dim3(ACC_THREADS), 0, stream, work, d_points, log_n, scale);
      if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "g1_fft: store kernel launch failed");
    }
    return rc;
  });
}

// ---------------------------------------------------------------------------------------------
// All KZG openings of a polynomial on its domain (Feist / Khovratovich, "FK20"): the kernels and drivers of kzg_open_table_run /
// kzg_open_all_run.                                                                                         
// ---------------------------------------------------------------------------------------------
//
//   f = sum_{j<n} f_j X^j, g_i = [s^i]G1:   pi_t = [(f(s) - f(w^t)) / (s - w^t)]G1 = sum_m w^(tm) h_m,   w = omega_n,
//   h_m = sum_{i=0}^{n-2-m} f_{m+1+i} g_i  (m <= n - 2),  h_{n-1} = identity.
//
// h is a Toeplitz product, computed by a circulant embedding of size 2n:
//   x_i = g_{n-2-i} (i <= n - 2), identity elsewhere;    y_0 = f_{n-1}, y_1 .. y_{n+1} = 0, y_{n+1+j} = f_j (1 <= j <= n - 2)
//   s^ = G1-FFT_2n(x)  (the TABLE: the SRS alone, once per size),  c^ = NTT_2n(y),  u^_i = [c^_i] s^_i,
//   h = the first n entries of (2n)^-1 G1-FFT_2n(u^) taken with omega_2n^-1,   pi = G1-FFT_n(h) with omega_n.
// f_0 never enters, and the identity in slot n - 1 comes out of the arithmetic (every product that could reach it has a zero factor).
//
// The point arithmetic is the FFT's above: the same g1_mul_words / g1_add / g1_neg calls on the same operand classes (an affine point
// read with fe_from_ext and z = 1, as g1_fft_load_kernel makes it; Jacobian records as the stages leave them).

struct KzgScalar {         // a canonical integer below r, by value (constant indices only: scalar loads)
  uint32_t w[8];
};

// x of the circulant: slot i <= n - 2 is g[n - 2 - i], the other n + 1 slots the identity (0, 0)
__global__ __launch_bounds__(256) void kzg_open_arrange_points_kernel(const uint32_t* __restrict__ g, uint32_t* __restrict__ x,
                                                                      uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n) return;
  uint4* o = reinterpret_cast<uint4*>(x + i * 16);
  if (i + 2 <= n) {
    const uint4* q = reinterpret_cast<const uint4*>(g + (n - 2 - i) * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = q[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = make_uint4(0, 0, 0, 0);
  }
}

// y of the circulant from n coefficients (8 words each): every one of the 2n slots is written, the zeros too
__global__ __launch_bounds__(256) void kzg_open_arrange_coeffs_kernel(const uint32_t* __restrict__ f, uint32_t* __restrict__ y,
                                                                      uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n) return;
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (i == 0 || i >= n + 2) {
    const uint4* q = reinterpret_cast<const uint4*>(f + (i == 0 ? n - 1 : i - n - 1) * 8);
    lo = q[0];
    hi = q[1];
  }
  uint4* o = reinterpret_cast<uint4*>(y + i * 8);
  o[0] = lo;
  o[1] = hi;
}

// work[bitrev_2n(i)] = [c^_i * scale] s^_i: the scalar goes from Montgomery words to the canonical integer as in
// g1_fft_twiddle_kernel, with the constant 32 * scale in the place of 32 (scale = (2n)^-1 rides along for nothing); every lane has its
// own scalar, so the double-and-add runs with lane-divergent bit tests.  An identity table entry or a zero scalar gives the flag.
__global__ __launch_bounds__(ACC_THREADS) void kzg_open_load_mul_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ c,
                                                                        uint32_t* __restrict__ work, uint32_t log_m, KzgScalar k32s) {
  const size_t m = (size_t)1 << log_m;
  const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= m) return;
  const uint4* qc = reinterpret_cast<const uint4*>(c + i * 8);
  const uint4 c0 = qc[0], c1 = qc[1];
  const uint32_t cw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  uint32_t kw[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) kw[k] = k32s.w[k];
  uint32_t e[8];
  fe_pack(e, fe_canonical(fe_mul(fe_unpack<FrParams>(cw), fe_unpack<FrParams>(kw))));   // (c 2^256) * (32 scale) * 2^-261 = c scale
  const uint4* q = reinterpret_cast<const uint4*>(table + i * 16);
  const uint4 a0 = q[0], a1 = q[1], b0 = q[2], b1 = q[3];
  const uint32_t wx[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t wy[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= wx[k] | wy[k];
  G1Jac p;
  p.x = fe_from_ext<FqParams>(wx);
  p.y = fe_from_ext<FqParams>(wy);
  p.z = fe_one<FqParams>();
  p.inf = false;
  G1Jac r = g1_identity();
  if (any != 0) r = g1_mul_words(p, e);
  if (r.inf) r = g1_identity();
  store_jac(work + (size_t)g1_fft_bitrev((uint32_t)i, log_m) * PT_WORDS, r);
}

// slots 0 .. n - 1 of the 2n-record buffer -> an n-record buffer at bitrev_n(i): Jacobian records as they are, no inversion
__global__ __launch_bounds__(256) void kzg_open_truncate_kernel(const uint32_t* __restrict__ work2, uint32_t* __restrict__ work1,
                                                                uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(work2 + i * PT_WORDS);
  uint4* o = reinterpret_cast<uint4*>(work1 + (size_t)g1_fft_bitrev((uint32_t)i, log_n) * PT_WORDS);
#pragma unroll
  for (int k = 0; k < PT_WORDS / 4; ++k) o[k] = q[k];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t KZG_OPEN_LOG_MAX = G1_FFT_LOG_MAX - 1;      // the circulant has 2n points

// Fr::ROOT_OF_UNITY (order 2^28), its inverse and TWO_INV of halo2curves::bn256, Montgomery words
static const host::Fr4 KZG_FR_ROOT = {{0x9632c7c5b639feb8ULL, 0x985ce3400d0ff299ULL, 0xb2dd880001b0ecd8ULL, 0x1d69070d6d98ce29ULL}};
static const host::Fr4 KZG_FR_ROOT_INV = {{0x05f05c05affb3d96ULL, 0xb8e594ebfc3b5137ULL, 0x60314620b85bc4c1ULL, 0x2a4129bebb6fc591ULL}};
static const host::Fr4 KZG_FR_TWO_INV = {{0x783c14d81ffffffeULL, 0xaf982f6f0c8d1eddULL, 0x8f5f7492fcfd4f45ULL, 0x1f37631a3d9cbfacULL}};

// the 2^log-th root of unity EvaluationDomain uses (ROOT_OF_UNITY squared 28 - log times), or its inverse
static host::Fr4 kzg_open_omega(uint32_t log, bool inverse) {
  host::Fr4 w = inverse ? KZG_FR_ROOT_INV : KZG_FR_ROOT;
  for (uint32_t i = log; i < 28; ++i) w = host::fr_mul(w, w);
  return w;
}

// m canonical powers of omega at tw (g1_fft_run's twiddle table)
static int kzg_open_twiddles(uint32_t* tw, size_t m, const host::Fr4& omega, hipStream_t stream) {
  if (m == 0) return HM_OK;
  const int rc = fr_powers_run(tw, m, omega.l, stream);
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(g1_fft_twiddle_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, stream, tw, m);
  if (hipGetLastError() != hipSuccess) return hm_fail(HM_ERR_HIP, "kzg_open: twiddle kernel launch failed");
  return HM_OK;
}

// the log stages of g1_fft_run on a working buffer already in bit-reversed order
static int kzg_open_stages(uint32_t* work, const uint32_t* tw, uint32_t log, hipStream_t stream) {
  if (log == 0) return HM_OK;
  const dim3 pairs((uint32_t)((((size_t)1 << (log - 1)) + ACC_THREADS - 1) / ACC_THREADS));
  for (uint32_t s = 0; s < log; ++s) {
    if (log - 1 - s >= 6) hipLaunchKernelGGL(g1_fft_stage_kernel<true>, pairs, dim3(ACC_THREADS), 0, stream, work, tw, log, s);
    else hipLaunchKernelGGL(g1_fft_stage_kernel<false>, pairs, dim3(ACC_THREADS), 0, stream, work, tw, log, s);
    if (hipGetLastError() != hipSuccess) return hm_fail(HM_ERR_HIP, "kzg_open: stage kernel launch failed");
  }
  return HM_OK;
}

// s^ = G1-FFT_2n(x) from the first n = 2^log_n monomial points (16-word affine external): 2n affine points at d_table, which is also
// the transform's own buffer.  Asynchronous on `stream`.
int kzg_open_table_run(DeviceCtx& ctx, const uint32_t* d_g_xy, uint32_t log_n, uint32_t* d_table_xy, hipStream_t stream) {
  if (log_n > KZG_OPEN_LOG_MAX) return hm_fail(HM_ERR_BAD_ARG, "kzg_open_table: log_n > 23");
  const size_t n = (size_t)1 << log_n;
  hipLaunchKernelGGL(kzg_open_arrange_points_kernel, dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), 0, stream, d_g_xy, d_table_xy, log_n);
  if (hipGetLastError() != hipSuccess) return hm_fail(HM_ERR_HIP, "kzg_open_table: arrangement kernel launch failed");
  const host::Fr4 omega2 = kzg_open_omega(log_n + 1, false);
  return g1_fft_run(ctx, d_table_xy, 16, omega2.l, log_n + 1, nullptr, stream);
}

// All n openings of `count` polynomials (n x 8 words each, back to back at d_coeffs) over one table: count x n affine points at
// d_proofs_xy, (0, 0) for the identity; proof t of a polynomial is its opening at omega_n^t.  The buffers (2n + n Jacobian records, 2n
// Fr words, the two twiddle tables) are allocated once per call, stream-ordered, and serve every polynomial in turn; between the load
// and the store a polynomial's points stay Jacobian.  ctx.mu is held by the caller (the Fr NTT uses the context's tables).
int kzg_open_all_run(DeviceCtx& ctx, const uint32_t* d_table_xy, const uint32_t* d_coeffs, uint32_t log_n, size_t count,
                     uint32_t* d_proofs_xy, hipStream_t stream, double* times) {
  if (log_n > KZG_OPEN_LOG_MAX) return hm_fail(HM_ERR_BAD_ARG, "kzg_open_all: log_n > 23");
  if (count == 0) return HM_OK;
  const uint32_t log_m = log_n + 1;
  const size_t n = (size_t)1 << log_n, m = 2 * n;
  const host::Fr4 omega2 = kzg_open_omega(log_m, false), omega2_inv = kzg_open_omega(log_m, true), omega1 = kzg_open_omega(log_n, false);
  host::Fr4 inv_m = KZG_FR_TWO_INV;
  for (uint32_t i = 1; i < log_m; ++i) inv_m = host::fr_mul(inv_m, KZG_FR_TWO_INV);
  KzgScalar k32s;
  {
    const host::Fr4 one_int = {{1, 0, 0, 0}};
    const host::Fr4 v = host::fr_mul(host::fr_mul(inv_m, host::FR_32), one_int);   // Montgomery words -> the canonical integer 32 / 2n
    std::memcpy(k32s.w, v.l, 32);
  }
  const size_t work2_words = m * PT_WORDS, work1_words = n * PT_WORDS, y_words = m * 8, tw2_words = n * 8, tw1_words = (n / 2) * 8;
  hipEvent_t ev[8] = {};
  int rc = stream_scratch("kzg_open_all", (work2_words + work1_words + y_words + tw2_words + tw1_words) * 4, stream, [&](uint8_t* mem) -> int {
    uint32_t *work2 = (uint32_t*)mem, *work1 = work2 + work2_words, *y = work1 + work1_words;
    uint32_t *tw2 = y + y_words, *tw1 = tw2 + tw2_words;
    int rc = HM_OK;
    if (times) {
      for (int i = 0; i < 8 && rc == HM_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: hipEventCreate failed");
    }
    // with `times` the spans of the LAST polynomial are measured: one event between the steps
    auto mark = [&](int i, bool last) {
      if (times && last && rc == HM_OK && hipEventRecord(ev[i], stream) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: hipEventRecord failed");
    };
    if (rc == HM_OK) rc = kzg_open_twiddles(tw2, n, omega2_inv, stream);
    if (rc == HM_OK) rc = kzg_open_twiddles(tw1, n / 2, omega1, stream);
    const dim3 all_m64((uint32_t)((m + ACC_THREADS - 1) / ACC_THREADS)), all_n64((uint32_t)((n + ACC_THREADS - 1) / ACC_THREADS));
    const dim3 all_m256((uint32_t)((m + 255) / 256)), all_n256((uint32_t)((n + 255) / 256));
    for (size_t p = 0; rc == HM_OK && p < count; ++p) {
      const bool last = p + 1 == count;
      mark(0, last);
      hipLaunchKernelGGL(kzg_open_arrange_coeffs_kernel, all_m256, dim3(256), 0, stream, d_coeffs + p * n * 8, y, log_n);
      if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: arrangement kernel launch failed");
      mark(1, last);
      if (rc == HM_OK) {
        NttCall call{};
        call.log_n = log_m, call.batch = 1;
        NttPointers ptrs;
        ptrs.d_a = y, ptrs.omega = omega2.l;
        rc = ntt_run(ctx, call, ptrs, stream);
      }
      mark(2, last);
      if (rc == HM_OK) {
        hipLaunchKernelGGL(kzg_open_load_mul_kernel, all_m64, dim3(ACC_THREADS), 0, stream, d_table_xy, (const uint32_t*)y, work2, log_m, k32s);
        if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: load kernel launch failed");
      }
      mark(3, last);
      if (rc == HM_OK) rc = kzg_open_stages(work2, tw2, log_m, stream);
      mark(4, last);
      if (rc == HM_OK) {
        hipLaunchKernelGGL(kzg_open_truncate_kernel, all_n256, dim3(256), 0, stream, (const uint32_t*)work2, work1, log_n);
        if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: truncate kernel launch failed");
      }
      mark(5, last);
      if (rc == HM_OK) rc = kzg_open_stages(work1, tw1, log_n, stream);
      mark(6, last);
      if (rc == HM_OK) {
        hipLaunchKernelGGL(g1_fft_store_kernel<16>, all_n64, dim3(ACC_THREADS), 0, stream, (const uint32_t*)work1, d_proofs_xy + p * n * 16,
                           log_n, G1FftScale{});
        if (hipGetLastError() != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: store kernel launch failed");
      }
      mark(7, last);
    }
    return rc;
  });
  if (times) {
    if (rc == HM_OK && hipEventSynchronize(ev[7]) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: hipEventSynchronize failed");
    for (int i = 0; i < 7 && rc == HM_OK; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) != hipSuccess) rc = hm_fail(HM_ERR_HIP, "kzg_open_all: hipEventElapsedTime failed");
      times[i] = ms;
    }
    for (int i = 0; i < 8; ++i)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
  }
  return rc;
}

}  // namespace hm
