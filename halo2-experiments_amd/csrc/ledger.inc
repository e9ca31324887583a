// ledger.inc -- the pairing operands of one user's ledger opening (ledger.py: verify_ledger_users; the kernel: ledger.hip).  DESIGN.md
// section 31.  User b holds the row i of a ledger of n = 2^k rows: an id, P balances and one opening pi of the combined commitment
//
//     C_gamma = C_id + sum_p gamma^(p+1) C_p          at omega^i, with the value          y = id + sum_p gamma^(p+1) b_p,
//
// and the check e(pi, [s]G2) = e(R, G2) with R = C_gamma + [r - y]G + [omega^i]pi.  ld_pair writes the pair (pi, -R) as two rows of
// canonical affine Montgomery words, (0, 0) for the identity: the d_g1_xy layout of hm_pairing_check_bn256_dev.
//
//   validity   the opening's coordinate words are below p and satisfy the curve equation ((0, 0) is the identity and is valid); the
//              id's and every balance's words are below r; the row is below 2^k.  A user that fails any of these is FLAGGED: two zero
//              rows, and nothing of it is multiplied (the rule of verify_read.inc and verify_sums.inc).
//   y          by Horner on the words as they come: x 2^256 is a representative of the Montgomery form, a product with gamma in
//              internal form keeps that scale, so P products give y 2^256 and one more, by 32, the canonical integer of r - y.
//   omega^i    square-and-multiply over the k bits of i, from omega alone (2k products at the most).
//   R          [r - y]G + [omega^i]pi by a joint ladder (ld_mul2_by_field: one doubling chain for both scalars, the addends G, pi and
//              G + pi, field-by-field assignments as in g1_mul.h), then C_gamma, every addition the complete one: pi = +-G makes
//              G + pi a doubling or the identity, pi = the identity leaves the single product, y = 0 leaves pi's, R itself may be
//              the identity.
//   rows       pi is affine and canonical already and is copied; -R takes vs_finish's Fermat inversion (verify_sums.inc).
// Included inside namespace hm by ledger.hip and by host_check.cpp, which runs ld_pair with the bound tracking on (hc_ledger_pair);
// needs g1_mul.h, fq_inverse.h, g1_codec.inc (g1_check_one) and verify_sums.inc (vs_load_base, vs_store_acc, vs_finish).

constexpr uint32_t LD_MAX_ASSETS = 1u << 16;

// what every user of a call shares.  Plain words, read with constant indices only: a kernel that takes it by value reads it with
// scalar loads.
struct LdShared {
  uint32_t gamma[8];                       // Montgomery words
  uint32_t omega[8];                       // Montgomery words of the 2^k-th root of unity
  uint32_t c_gamma[16];                    // affine Montgomery words, (0, 0) = the identity
  uint32_t k, assets;
};

HM_HD bool ld_fr_words_canonical(const uint32_t (&w)[8]) {
  bool lt = false, eq = true;
#pragma unroll
  for (int j = 7; j >= 0; --j) {
    lt = lt || (eq && w[j] < FrParams::MOD32[j]);
    eq = eq && w[j] == FrParams::MOD32[j];
  }
  return lt;
}

HM_HD void ld_load8(const uint32_t* p, uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = p[j];
}

// every scalar of the user in canonical form?  (the id, then the P balances)
HM_HD bool ld_scalars_canonical(const uint32_t* id, const uint32_t* balances, uint32_t assets) {
  uint32_t w[8];
  ld_load8(id, w);
  bool ok = ld_fr_words_canonical(w);
  for (uint32_t p = 0; p < assets; ++p) {
    ld_load8(balances + (size_t)p * 8, w);
    ok = ok && ld_fr_words_canonical(w);
  }
  return ok;
}

// the canonical integer of r - y (0 for y = 0), y = id + sum_p gamma^(p+1) b_p
HM_HD void ld_minus_y(const LdShared& s, const uint32_t* id, const uint32_t* balances, uint32_t (&e)[8]) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = s.gamma[j];
  const Fr gamma = fe_from_ext<FrParams>(w);
  Fr acc = fe_zero<FrParams>();
  for (uint32_t p = s.assets; p > 0; --p) {
    ld_load8(balances + (size_t)(p - 1) * 8, w);
    acc = fe_mul(fe_norm(fe_add(acc, fe_unpack<FrParams>(w))), gamma);
  }
  ld_load8(id, w);
  acc = fe_norm(fe_add(acc, fe_unpack<FrParams>(w)));                         // y 2^256, below 8r
  const uint32_t k32[8] = {32, 0, 0, 0, 0, 0, 0, 0};
  fe_pack(e, fe_canonical(fe_mul(fe_norm(fe_sub<9, 29>(fe_zero<FrParams>(), acc)), fe_unpack<FrParams>(k32))));
}

// the canonical integer of omega^i, i below 2^k
HM_HD void ld_omega_power(const LdShared& s, uint32_t i, uint32_t (&e)[8]) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = s.omega[j];
  const Fr omega = fe_from_ext<FrParams>(w);
  Fr acc = fe_one<FrParams>();
  for (uint32_t bit = s.k; bit > 0; --bit) {
    acc = fe_sqr(acc);
    if ((i >> (bit - 1)) & 1u) acc = fe_mul(acc, omega);
  }
  const uint32_t one_int[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  fe_pack(e, fe_canonical(fe_mul(acc, fe_unpack<FrParams>(one_int))));       // v 2^-261: the integer the internal form stands for
}

// the generator (1, 2) as a Jacobian operand
HM_HD G1Jac ld_generator() {
  G1Jac g;
  g.x = fe_one<FqParams>();
  g.y = fe_norm(fe_dbl(g.x));
  g.z = g.x;
  g.inf = false;
  return g;
}

// one of three points by a lane's own selector (1, 2 or 3), limb by limb through masks: every limb of all three is read, so that
// the compiler sees values, never a choice between the addresses of three records (which would pin them to the stack)
HM_HD Fq ld_select(uint32_t sel, const Fq& a, const Fq& b, const Fq& c, double class_bound) {
  const uint32_t ma = 0u - (uint32_t)(sel == 1), mb = 0u - (uint32_t)(sel == 2), mc = 0u - (uint32_t)(sel == 3);
  Fq r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = (a.l[i] & ma) | (b.l[i] & mb) | (c.l[i] & mc);
  HM_DECLARE(r, class_bound);
  return r;
}

// [a]p + [b]q with ONE doubling chain for both 256-bit integers: per bit the accumulator doubles once and takes p, q or p + q, by the
// complete addition -- p + q may be the identity or a doubling of either.  The accumulator is assigned field by field, as in
// g1_mul_words_by_field (g1_mul.h), which keeps a kernel free of scratch.  Neither p nor q is the identity.
HM_HD G1Jac ld_mul2_by_field(const G1Jac& p, const uint32_t (&a_in)[8], const G1Jac& q, const uint32_t (&b_in)[8]) {
  uint32_t a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = a_in[j], b[j] = b_in[j];
  G1Jac pq;
  g1_assign(pq, g1_add(p, q));
  if (pq.inf) g1_assign(pq, g1_identity());
  G1Jac acc = g1_identity();
  for (int bit = 0; bit < 256; ++bit) {
    if (!acc.inf) g1_assign(acc, g1_double_nz(acc));
    const uint32_t sel = (a[7] >> 31) | ((b[7] >> 31) << 1);
    if (sel) {
      G1Jac t;
      t.x = ld_select(sel, p.x, q.x, pq.x, HM_G1_XB);
      t.y = ld_select(sel, p.y, q.y, pq.y, HM_G1_YB);
      t.z = ld_select(sel, p.z, q.z, pq.z, HM_G1_ZB);
      t.inf = sel == 3 && pq.inf;
      g1_assign(acc, g1_add(acc, t));
    }
#pragma unroll
    for (int j = 7; j > 0; --j) {
      a[j] = (a[j] << 1) | (a[j - 1] >> 31);
      b[j] = (b[j] << 1) | (b[j - 1] >> 31);
    }
    a[0] <<= 1;
    b[0] <<= 1;
  }
  return acc;
}

// One user: -> its flag; rows: 2 x 16 words, (pi, -R), zeros when flagged.
HM_HD uint32_t ld_pair(const LdShared& s, const uint32_t* opening, uint32_t index, const uint32_t* id, const uint32_t* balances,
                       uint32_t* rows) {
  uint32_t wx[8], wy[8];
  ld_load8(opening, wx);
  ld_load8(opening + 8, wy);
  const bool ok = (s.k >= 32 || (index >> s.k) == 0) && g1_check_one(wx, wy) && ld_scalars_canonical(id, balances, s.assets);
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 32; ++j) rows[j] = 0;
    return 1;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    rows[j] = wx[j];
    rows[8 + j] = wy[j];
  }
  uint32_t e[8], w[8];
  ld_minus_y(s, id, balances, e);
  const G1Jac pi = vs_load_base(opening);
  G1Jac sum;
  if (pi.inf) {
    g1_assign(sum, g1_mul_words_by_field(ld_generator(), e));                 // [r - y]G alone
  } else {
    ld_omega_power(s, index, w);
    g1_assign(sum, ld_mul2_by_field(ld_generator(), e, pi, w));               // [r - y]G + [omega^i]pi
  }
  if (sum.inf) g1_assign(sum, g1_identity());
  g1_assign(sum, g1_add(vs_load_base(s.c_gamma), sum));
  uint32_t record[VS_ACC_WORDS];
  vs_store_acc(record, sum.inf ? g1_identity() : sum);
  vs_finish(record, true, rows + VS_ROW_WORDS);
  return 0;
}
