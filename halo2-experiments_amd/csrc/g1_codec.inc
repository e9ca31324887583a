// g1_codec.inc -- the SRS point encodings of ParamsKZG::read / write: the kernels of g1_compress_run, g1_decompress_run and
// g1_check_run (msm.hip, included from inside namespace hm there, so that they fall under msm.o's ISA checks).  DESIGN.md section 11.
// The per-point functions are host-callable too: host_check.cpp includes this file (without the kernels) for the bound proof.
//
//   compressed G1 (32 bytes): canonical x little-endian, bit 7 of byte 31 = parity of canonical y; the identity is 32 zero bytes
//   raw G1 (64 bytes):        x, y as external Montgomery words, (0, 0) = identity (the library's affine layout)
//
// Decompression is one square root per point: y = (x^3 + 3)^((p+1)/4), since p = 3 mod 4, then y^2 == x^3 + 3 decides
// whether x was on the curve (BN256 G1 has cofactor 1: that is the whole validity check).  An invalid entry is written as
// (0, 0) and lowers the device word `first_bad` (initialised to all ones) with atomicMin, so the host reads the smallest bad index.

// x^3 + 3 for x in internal form (a product output): reduced to < 3p for fe_canonical
HM_HD Fq g1_curve_rhs(const Fq& x) {
  const Fq one = fe_one<FqParams>();
  const Fq x3 = fe_mul(fe_sqr(x), x);
  return fe_reduce_small(fe_norm(fe_add(fe_add(x3, one), fe_add(one, one))));
}

// a^((p+1)/4), left to right over the 252-bit constant exponent: the bit tests are wave-uniform branches.  251 squarings and
// 108 products; a windowed form needs a table indexed at run time, which goes to scratch.
HM_HD Fq fq_sqrt_candidate(const Fq& a) {
  uint32_t m[9], e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = FqParams::MOD[i];
  m[0] += 1;                                     // MOD[0] + 1 < 2^29: no carry
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = ((m[i] >> 2) | (m[i + 1] << 27)) & MASK29;
  e[8] = m[8] >> 2;
  Fq acc = a;                                    // the top bit of e[8] (bit 19)
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    const int top = i == 8 ? 18 : 28;
    for (int bit = top; bit >= 0; --bit) {
      acc = fe_sqr(acc);
      if ((e[i] >> bit) & 1) acc = fe_mul(acc, a);
    }
  }
  return acc;
}

// 8 u32 words (little-endian) < MOD, i.e. a canonical 256-bit integer
HM_HD bool fq_words_canonical(const uint32_t (&w)[8]) {
  bool lt = false, eq = true;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    lt = lt || (eq && w[k] < FqParams::MOD32[k]);
    eq = eq && w[k] == FqParams::MOD32[k];
  }
  return lt;
}

// the canonical integer of an element in internal form: v * 2^-261 by one product with the plain integer 1
HM_HD Fq fq_to_canonical_int(const Fq& a) {
  const uint32_t one_int[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0};
  return fe_canonical(fe_mul(a, fe_const<FqParams>(one_int)));
}

HM_HD bool fq_equal(const Fq& a, const Fq& b) {   // both canonical
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) d |= a.l[k] ^ b.l[k];
  return d == 0;
}

// one point each: the formula sequences of the kernels below, also built on the host with bound tracking (host_check.cpp)
// affine external words -> compressed words.  Input is trusted (the library's own points).
HM_HD void g1_compress_one(const uint32_t (&wx)[8], const uint32_t (&wy)[8], uint32_t (&v)[8]) {
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    any |= wx[k] | wy[k];
    v[k] = 0;
  }
  if (any) {
    // Montgomery words x 2^256 times 32 * 2^-261 = the canonical integer (msm_digits_kernel's conversion, over Fq)
    const uint32_t k32[9] = {32, 0, 0, 0, 0, 0, 0, 0, 0};
    const Fq x = fe_canonical(fe_mul(fe_unpack<FqParams>(wx), fe_const<FqParams>(k32)));
    const Fq y = fe_canonical(fe_mul(fe_unpack<FqParams>(wy), fe_const<FqParams>(k32)));
    fe_pack(v, x);
    v[7] |= (y.l[0] & 1u) << 31;
  }
}

// compressed words -> affine external words; false (and (0, 0)) for x >= p or x^3 + 3 not a square
HM_HD bool g1_decompress_one(const uint32_t (&in)[8], uint32_t (&ox)[8], uint32_t (&oy)[8]) {
  uint32_t w[8], any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    w[k] = in[k];
    ox[k] = oy[k] = 0;
  }
  const uint32_t sign = w[7] >> 31;
  w[7] &= 0x7fffffffu;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= w[k];
  bool ok = fq_words_canonical(w);               // also rejects bit 6 of byte 31: MOD < 2^254
  if (ok && (any | sign)) {
    const Fq x = fe_mul(fe_unpack<FqParams>(w), fe_const<FqParams>(FqParams::R2INT));   // x * 2^522 * 2^-261 = x * 2^261
    const Fq rhs = g1_curve_rhs(x);
    Fq y = fq_sqrt_candidate(rhs);
    ok = fq_equal(fe_canonical(fe_sqr(y)), fe_canonical(rhs));
    if (ok) {
      if ((fq_to_canonical_int(y).l[0] & 1u) != sign) y = fe_norm(fe_sub<3, 29>(fe_zero<FqParams>(), y));
      fe_to_ext(ox, x);
      fe_to_ext(oy, y);
    }
  }
  return ok;
}

// the checked raw format: every coordinate word canonical (< p), and y^2 == x^3 + 3 unless the point is (0, 0)
HM_HD bool g1_check_one(const uint32_t (&wx)[8], const uint32_t (&wy)[8]) {
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) any |= wx[k] | wy[k];
  bool ok = fq_words_canonical(wx) && fq_words_canonical(wy);
  if (ok && any) {
    const Fq x = fe_from_ext<FqParams>(wx), y = fe_from_ext<FqParams>(wy);
    ok = fq_equal(fe_canonical(fe_sqr(y)), fe_canonical(g1_curve_rhs(x)));
  }
  return ok;
}

#if defined(__HIPCC__)
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
#endif
