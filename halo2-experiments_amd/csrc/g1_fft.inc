// g1_fft.inc -- best_fft over BN256 G1 (g_to_lagrange / ParamsKZG::downsize): the kernels of g1_fft_run (msm.hip,
// included from inside namespace hm there, so that they fall under msm.o's ISA checks).
//
//   a[i] <- sum_j [omega^(ij)] a[j], then optionally a[i] <- [scale] a[i]   (DESIGN.md section 10)
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

constexpr uint32_t G1_FFT_LOG_MAX = 24;

// [e] b for a 256-bit integer e (8 words, little-endian), left to right; leading zero bits cost a flag test each
__device__ __forceinline__ G1Jac g1_mul_words(const G1Jac& b, const uint32_t (&e_in)[8]) {
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = e_in[k];
  G1Jac acc = g1_identity();
  for (int bit = 0; bit < 256; ++bit) {
    acc = g1_double(acc);
    if (e[7] >> 31) acc = g1_add(acc, b);
#pragma unroll
    for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
    e[0] <<= 1;
  }
  return acc;
}

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
