// g1_codec.inc -- the SRS point encodings of ParamsKZG::read / write: the per-point functions of g1_compress_run, g1_decompress_run
// and g1_check_run (g1_codec.hip holds the kernels and the drivers; verify.hip decompresses a proof's points with them).  DESIGN.md
// section 11.  They are host-callable: host_check.cpp includes this file for the bound proof.  Included inside namespace hm.
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

// one point each: the formula sequences of the kernels, also built on the host with bound tracking (host_check.cpp)
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
