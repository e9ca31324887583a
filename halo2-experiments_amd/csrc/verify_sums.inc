// verify_sums.inc -- the two G1 points of every proof's OWN opening check, all proofs in one launch (batch_verifier.py: proof_sums,
// verdicts).  DESIGN.md section 28.  For proof b, over the arrays hm_verify_terms_dev and the read call leave on the device,
//
//     L_b = h2_l[b] [h']_b
//     R_b = sum_j own[b, j] P[b, j]  +  sum_k shared[b, k] S_k  +  h2_r[b] [h']_b          T = own + shared + 1 terms
//
// and the pair (L_b, -R_b) is written as two rows of canonical affine Montgomery words, (0, 0) for the identity: the d_g1_xy layout
// of hm_pairing_check_bn256_dev, so that e(L_b, [s]G2) e(-R_b, G2) = 1 is check b of one pairing call.
//
//   workgroup  one per proof, VS_THREADS lanes.  Lane t takes the terms t, t + VS_THREADS, ... of the T + 1 products (term T is L's);
//              a product is g1_mul_words_by_field (g1_mul.h: g1_mul_words, limb for limb, with the accumulator assigned field by
//              field, which keeps the kernel free of scratch) on the affine base with the scalar's canonical integer -- lane-divergent
//              bit tests, as in the FK20 table products -- and joins the lane's sum by the complete g1_add.  The sum stands in the
//              lane's LDS record between the terms, so no accumulator is live across a product.  L rides in the same loop on lane
//              T mod VS_THREADS, so it costs no pass of its own.
//   fold       the records are 28 words (27 limbs and the identity flag); log2(VS_THREADS) halving steps of g1_add; record
//              VS_THREADS holds L.
//   finish     lane 0 negates and normalises R, lane 1 normalises L: one Fermat inversion each, side by side in one wavefront.
// Every addition is the complete one: equal operands double, opposite ones give the identity, identity operands pass through; a
// (0, 0) base and a zero scalar give the identity.  The result is a group element in canonical form, so it does not depend on the
// fold's order.  A proof whose flag is set gets two zero rows and nothing of it is multiplied (the kernel, verify.hip).
// Included inside namespace hm by verify.hip and by host_check.cpp, which runs the same functions with the bound tracking on; needs
// g1_mul.h and fq_inverse.h.

constexpr int VS_THREADS = 128;            // lanes of a proof's workgroup: a power of two
constexpr uint32_t VS_ACC_WORDS = 28;      // an accumulator record: x, y, z limbs and the identity flag
constexpr uint32_t VS_ROW_WORDS = 16;      // an output row: 8 u64 = 16 u32
static_assert((VS_THREADS & (VS_THREADS - 1)) == 0, "the fold halves the lanes");

struct VsArgs {
  const uint32_t* bases;                   // (n_proofs * own + shared + n_proofs) x 16: own points, shared points, every proof's [h']
  const uint32_t* own_s;                   // (n_proofs * own) x 8
  const uint32_t* shared_s;                // (n_proofs, shared) x 8
  const uint32_t* h2r;                     // n_proofs x 8
  const uint32_t* h2l;                     // n_proofs x 8
  uint64_t n_proofs;
  uint32_t own, shared;
};

// an affine base as a Jacobian operand with z = 1 (kzg_open_load_mul_kernel's form); all-zero words are flagged as the identity
HM_HD G1Jac vs_load_base(const uint32_t* p) {
  uint32_t wx[8], wy[8], any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    wx[k] = p[k];
    wy[k] = p[8 + k];
    any |= wx[k] | wy[k];
  }
  G1Jac r;
  r.x = fe_from_ext<FqParams>(wx);
  r.y = fe_from_ext<FqParams>(wy);
  r.z = fe_one<FqParams>();
  r.inf = any == 0;
  return r;
}

// Montgomery words -> the canonical integer, one product: (s 2^256) * 32 * 2^-261 = s
HM_HD void vs_scalar_words(const uint32_t* p, uint32_t (&e)[8]) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = p[k];
  const uint32_t k32[8] = {32, 0, 0, 0, 0, 0, 0, 0};
  fe_pack(e, fe_canonical(fe_mul(fe_unpack<FrParams>(w), fe_unpack<FrParams>(k32))));
}

HM_HD G1Jac vs_term(const uint32_t* base, const uint32_t* scalar) {
  const G1Jac p = vs_load_base(base);
  uint32_t e[8];
  vs_scalar_words(scalar, e);
  G1Jac r = g1_identity();
  if (!p.inf) r = g1_mul_words_by_field(p, e);
  if (r.inf) r = g1_identity();
  return r;
}

HM_HD void vs_store_acc(uint32_t* p, const G1Jac& a) {
  HM_G1_CHECK(a, "vs_store_acc: accumulator outside the Jacobian class");
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    p[i] = a.x.l[i];
    p[9 + i] = a.y.l[i];
    p[18 + i] = a.z.l[i];
  }
  p[27] = a.inf ? 1u : 0u;
}
HM_HD G1Jac vs_load_acc(const uint32_t* p) {
  G1Jac r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    r.x.l[i] = p[i];
    r.y.l[i] = p[9 + i];
    r.z.l[i] = p[18 + i];
  }
  HM_DECLARE(r.x, HM_G1_XB);
  HM_DECLARE(r.y, HM_G1_YB);
  HM_DECLARE(r.z, HM_G1_ZB);
  r.inf = p[27] != 0;
  return r;
}

// Lane t of `threads`: the sum of its terms of R_b, kept in the lane's own accumulator record `mine` between the terms (nothing of it
// is live across a product); the lane that meets term T stores L_b to `left`.
HM_HD void vs_lane(const VsArgs& a, uint64_t b, uint32_t t, uint32_t threads, uint32_t* mine, uint32_t* left) {
  const uint32_t T = a.own + a.shared + 1;
  const uint32_t* tail = a.bases + (a.n_proofs * a.own + a.shared + b) * VS_ROW_WORDS;
  vs_store_acc(mine, g1_identity());
  for (uint32_t j = t; j <= T; j += threads) {
    const uint32_t *base = tail, *scalar;
    if (j < a.own) {
      base = a.bases + (b * a.own + j) * VS_ROW_WORDS;
      scalar = a.own_s + (b * a.own + j) * 8;
    } else if (j + 1 < T) {
      base = a.bases + (a.n_proofs * a.own + (j - a.own)) * VS_ROW_WORDS;
      scalar = a.shared_s + (b * a.shared + (j - a.own)) * 8;
    } else {
      scalar = (j < T ? a.h2r : a.h2l) + b * 8;
    }
    const G1Jac r = vs_term(base, scalar);
    if (j == T) vs_store_acc(left, r);
    else vs_store_acc(mine, g1_add(vs_load_acc(mine), r));
  }
}

// one halving step of the fold, lane t < off: record t += record t + off
HM_HD void vs_fold_step(uint32_t* tree, uint32_t t, uint32_t off) {
  const G1Jac x = vs_load_acc(tree + (size_t)t * VS_ACC_WORDS), y = vs_load_acc(tree + (size_t)(t + off) * VS_ACC_WORDS);
  vs_store_acc(tree + (size_t)t * VS_ACC_WORDS, g1_add(x, y));
}

// an accumulator record -> one output row: (neg ? -P : P) in canonical affine Montgomery words, zeros for the identity
HM_HD void vs_finish(const uint32_t* record, bool neg, uint32_t* row) {
  const G1Jac p = vs_load_acc(record);
  uint32_t ox[8], oy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ox[k] = oy[k] = 0;
  if (!p.inf) {
    const Fq zi = fq_inverse(p.z);
    const Fq zi2 = fe_sqr(zi);
    G1Aff q;
    q.x = fe_mul(p.x, zi2);
    q.y = fe_mul(p.y, fe_mul(zi2, zi));
    if (neg) q = g1_neg_affine(q);
    fe_to_ext(ox, q.x);
    fe_to_ext(oy, q.y);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    row[k] = ox[k];
    row[8 + k] = oy[k];
  }
}
