// verify_read.inc -- the two kernels a batch of proofs needs around the verifier's sums (batch_verifier.py is the caller):
//
//   read     one lane per (proof, 32-byte slot).  The slot kinds are the same for every proof of one constraint system and lie in a
//            DEVICE table of one word per slot: VR_POINT | VR_TAIL | index.  A point slot is decompressed (g1_codec.inc: one square
//            root per lane) into the affine Montgomery words the MSM reads -- point `index` of proof b at row b * own_points + index of
//            `points`, or, with VR_TAIL, at row b of `tail` ([h'], which enters two sums of its own) -- and the canonical 32 bytes of y
//            that the transcript absorbs behind x go to row b * n_points + index of `ybytes`.  A scalar slot is checked < r and written
//            as Montgomery words to row b * n_scalars + index of `scalars`.  A slot that cannot be read -- x >= p, x^3 + 3 not a square,
//            the all-zero point (the identity cannot be absorbed), a scalar >= r, a table entry outside its array -- sets bad[b] and
//            leaves zeros.
//   colsum   out[c] = sum of rows [lo, hi) of column c of a (rows, cols) array of Montgomery Fr words: the proofs' contributions to the
//            points they share (fixed and sigma commitments, the generator).  Montgomery words add as integers mod r, so the sum needs
//            no product: a workgroup per column, one lazy sum per lane, a tree in LDS.
// The per-slot functions of the two kernels, which verify.hip holds with their drivers.  Included inside namespace hm, behind
// g1_codec.inc; the functions are host-callable: host_check.cpp includes this file for the bound proof.

constexpr uint32_t VR_POINT = 1u << 31, VR_TAIL = 1u << 30, VR_INDEX = VR_TAIL - 1u;

HM_HD bool fr_words_canonical(const uint32_t (&w)[8]) {
  bool lt = false, eq = true;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    lt = lt || (eq && w[k] < FrParams::MOD32[k]);
    eq = eq && w[k] == FrParams::MOD32[k];
  }
  return lt;
}

// 32 canonical bytes -> Montgomery words; false (and zeros) for a value not below r
HM_HD bool proof_scalar_one(const uint32_t (&in)[8], uint32_t (&out)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = 0;
  if (!fr_words_canonical(in)) return false;
  const Fr s = fe_mul(fe_unpack<FrParams>(in), fe_const<FrParams>(FrParams::R2INT));   // s * 2^522 * 2^-261: internal form
  fe_to_ext(out, s);
  return true;
}

// 32 compressed bytes -> affine Montgomery words and the canonical words of y; false (and zeros) for what Blake2bRead::read_point refuses
HM_HD bool proof_point_one(const uint32_t (&in)[8], uint32_t (&ox)[8], uint32_t (&oy)[8], uint32_t (&ycan)[8]) {
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    any |= in[k];
    ycan[k] = 0;
  }
  const bool ok = g1_decompress_one(in, ox, oy) && any != 0;       // all zero: the identity, decoded as (0, 0) and refused here
  if (ok) {
    const uint32_t k32[9] = {32, 0, 0, 0, 0, 0, 0, 0, 0};           // as g1_compress_one: Montgomery words -> the canonical integer
    fe_pack(ycan, fe_canonical(fe_mul(fe_unpack<FqParams>(oy), fe_const<FqParams>(k32))));
  }
  return ok;
}

// one step of a column's sum: acc < 3r, w any 256-bit word -> < 3r
HM_HD Fr colsum_step(const Fr& acc, const uint32_t (&w)[8]) { return fe_reduce_small(fe_norm(fe_add(acc, fe_unpack<FrParams>(w)))); }
HM_HD Fr colsum_join(const Fr& a, const Fr& b) { return fe_reduce_small(fe_norm(fe_add(a, b))); }
HM_HD void colsum_finish(const Fr& acc, uint32_t (&w)[8]) { fe_pack(w, fe_canonical(acc)); }
