// pairing.inc -- the optimal ate pairing on BN256 as batched product checks: for every check c, is prod_i e(P_i, Q_i) = 1 over the
// pairs [offsets[c], offsets[c + 1])?  pairing.py is the oracle; the value after the final exponentiation agrees with it bit for bit.
// DESIGN.md section 23.
//
//   tower    Fq2 = Fq[u] / (u^2 + 1), and Fq12 held FLAT over Fq2 in the basis 1, w, .., w^5 with w^6 = xi = 9 + u (Fq6 is the span of
//            the even powers).  An Fq12 value never stands in registers: it is a "slot" of 96 packed words (fe_pack, 8 per Fq) in
//            memory, word k of a lane at base[k * stride], in pairing.py's coefficient order ((a0, a1, a2), (b0, b1, b2)) = the
//            powers w^0, w^2, w^4, w^1, w^3, w^5.  Arithmetic runs one Fq2 at a time in registers: a product is the schoolbook sum
//            c_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j of fused Fq2 products (fe_mul2), lazily added, one reduction per c_k.
//   class R  every Fq that is stored, loaded or passed between the Fq2 functions: normalised limbs, value < 3p (HM_BOUNDS checks it
//            at every load and store, and every primitive in between checks its own precondition).
//   miller   one lane per pair: f_{6x+2, Q}(P) and the two Frobenius lines, T in Jacobian twist coordinates so that no step inverts.
//            A line is scaled by an Fq2 factor against pairing._line (Z3 ZZ when doubling, Z3 when adding); Fq2 lies in a proper
//            subfield, so the factor dies in the final exponentiation -- the Miller value itself is NOT pairing.miller_loop's.
//   finish   one lane per check: the product of its Miller values, f^(p^6 - 1) by one inversion (the norm to Fq2 through p^2
//            Frobenius maps, one Fq inversion by Fermat), ^(p^2 + 1), and the hard part by the EXACT exponent
//            (p^4 - p^2 + 1) / r = l0 + l1 p + l2 p^2 + p^3, l2 = 6x^2 + 1, l1 = -36x^3 - 18x^2 - 12x + 1, l0 = -36x^3 - 30x^2 - 18x - 2:
//            three powers by x, a short product chain, conjugation for the negative exponents; the squares behind the easy part
//            are cyclotomic (Granger-Scott: 9 Fq2 squares).
// Included inside namespace hm by pairing.hip, which holds the two kernels and their driver.  Everything here is host-callable:
// host_check.cpp includes this file for the bound proof and for the comparison with the oracle on a machine without a GPU.

struct Fq2 {
  Fq c0, c1;
};
// one lane's view of an Fq12 slot: word k at p[k * s]
struct PfRef {
  uint32_t* p;
  size_t s;
};
// one lane's slots: slot i begins at word 96 i
struct PfLane {
  uint32_t* base;
  size_t stride;
  HM_HD PfRef slot(uint32_t i) const { return PfRef{base + (size_t)i * 96u * stride, stride}; }
};
constexpr uint32_t PF_WORDS = 96;          // packed words of an Fq12
constexpr uint32_t PF_PAIR_SLOTS = 3;      // a pair's lane: the Miller value (slot 0, what finish reads), its twin, the line
constexpr uint32_t PF_CHECK_SLOTS = 11;    // a check's lane: see pf_finish_lane
constexpr uint32_t PF_LINE_MASK = 0x0bu;   // a line has the powers w^0, w^1, w^3
constexpr uint64_t PF_BN_X = 4965661367192848881ull;                  // the curve parameter x: 63 bits
constexpr uint64_t PF_ATE_LOW = 11347224129447541672ull;              // 6x + 2 = 2^64 + this: the 64 bits under the leading one
static_assert(PF_ATE_LOW == 6ull * PF_BN_X + 2ull, "6x + 2 mod 2^64");

// the coefficient of w^k stands at this index of pairing.py's order
HM_HD uint32_t pf_coeff(uint32_t k) { return (k & 1u) ? 3u + (k >> 1) : (k >> 1); }

#ifdef HM_BOUNDS
#define HM_PF_CHECK_R(a, what) HM_CHECK((a).lb <= MASK29 && (a).vb <= 3.0, what)
#else
#define HM_PF_CHECK_R(a, what) ((void)0)
#endif

// any lazy value below 2^261 -> class R
HM_HD Fq pf_red(const Fq& a) { return fe_reduce_small(fe_norm(a)); }

HM_HD Fq pf_load(const PfRef& m, uint32_t word) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = m.p[(size_t)(word + k) * m.s];
  Fq r = fe_unpack<FqParams>(w);
  HM_DECLARE(r, 3.0);
  return r;
}
HM_HD void pf_store(const PfRef& m, uint32_t word, const Fq& a) {
  HM_PF_CHECK_R(a, "pf_store: value outside class R");
  uint32_t w[8];
  fe_pack(w, a);
#pragma unroll
  for (int k = 0; k < 8; ++k) m.p[(size_t)(word + k) * m.s] = w[k];
}
HM_HD Fq2 pf_load2(const PfRef& m, uint32_t coeff) { return Fq2{pf_load(m, coeff * 16u), pf_load(m, coeff * 16u + 8u)}; }
HM_HD void pf_store2(const PfRef& m, uint32_t coeff, const Fq2& a) {
  pf_store(m, coeff * 16u, a.c0);
  pf_store(m, coeff * 16u + 8u, a.c1);
}

// ---- Fq2 on class R -----------------------------------------------------------------------------------------------------------
HM_HD Fq2 f2_zero() { return Fq2{fe_zero<FqParams>(), fe_zero<FqParams>()}; }
HM_HD Fq2 f2_one() { return Fq2{fe_one<FqParams>(), fe_zero<FqParams>()}; }
// c0 = a0 b0 + a1 (-b1), c1 = a0 b1 + a1 b0: product outputs
HM_HD Fq2 f2_mul(const Fq2& a, const Fq2& b) {
  const Fq nb1 = fe_sub<4, 29>(fe_zero<FqParams>(), b.c1);
  return Fq2{fe_mul2(a.c0, b.c0, a.c1, nb1), fe_mul2(a.c0, b.c1, a.c1, b.c0)};
}
// (a0 + a1)(a0 - a1), 2 a0 a1
HM_HD Fq2 f2_sqr(const Fq2& a) {
  const Fq s = fe_norm(fe_add(a.c0, a.c1)), d = fe_norm(fe_sub<4, 29>(a.c0, a.c1));
  return Fq2{fe_mul(s, d), fe_mul(fe_dbl(a.c0), a.c1)};
}
HM_HD Fq2 f2_mul_fq(const Fq2& a, const Fq& s) { return Fq2{fe_mul(a.c0, s), fe_mul(a.c1, s)}; }
HM_HD Fq2 f2_add(const Fq2& a, const Fq2& b) { return Fq2{pf_red(fe_add(a.c0, b.c0)), pf_red(fe_add(a.c1, b.c1))}; }
HM_HD Fq2 f2_dbl(const Fq2& a) { return f2_add(a, a); }
HM_HD Fq2 f2_sub(const Fq2& a, const Fq2& b) { return Fq2{pf_red(fe_sub<4, 29>(a.c0, b.c0)), pf_red(fe_sub<4, 29>(a.c1, b.c1))}; }
HM_HD Fq2 f2_neg(const Fq2& a) { return f2_sub(f2_zero(), a); }
HM_HD Fq2 f2_conj(const Fq2& a) { return Fq2{a.c0, pf_red(fe_sub<4, 29>(fe_zero<FqParams>(), a.c1))}; }
// lazy sum: limbs and value add up (the caller counts the terms)
HM_HD Fq2 f2_add_lazy(const Fq2& a, const Fq2& b) { return Fq2{fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
// (9 + u) a for a with normalised limbs (a lazy sum after fe_norm): 9 a0 - a1, a0 + 9 a1 as fused products with constants
HM_HD Fq2 f2_mul_xi(const Fq2& a) {
  const Fq nine = fe_const<FqParams>(PairingParams::NINE), m1 = fe_const<FqParams>(PairingParams::MINUS1), one = fe_one<FqParams>();
  return Fq2{fe_mul2(a.c0, nine, a.c1, m1), fe_mul2(a.c0, one, a.c1, nine)};
}

// a^(p - 2), left to right over the constant exponent (wave-uniform branches): 0 -> 0, nothing faults
HM_HD Fq fq_inv_fermat(const Fq& a) {
  uint32_t e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) e[i] = FqParams::MOD[i];
  e[0] -= 2;                                     // MOD[0] >= 2: no borrow
  Fq acc = a;                                    // the top bit of e[8] (bit 21)
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    const int top = i == 8 ? 20 : 28;
    for (int bit = top; bit >= 0; --bit) {
      acc = fe_sqr(acc);
      if ((e[i] >> bit) & 1) acc = fe_mul(acc, a);
    }
  }
  return acc;
}
static_assert((FqParams::MOD[8] >> 21) == 1, "the top limb of p has 22 bits");

HM_HD Fq2 f2_inv(const Fq2& a) {
  const Fq d = fq_inv_fermat(fe_mul2(a.c0, a.c0, a.c1, a.c1));
  return Fq2{fe_mul(a.c0, d), fe_mul(fe_sub<4, 29>(fe_zero<FqParams>(), a.c1), d)};
}

// ---- Fq12 on slots -------------------------------------------------------------------------------------------------------------
HM_HD void f12_one(const PfRef& d) {
  pf_store2(d, 0, f2_one());
  for (uint32_t c = 1; c < 6; ++c) pf_store2(d, c, f2_zero());
}
HM_HD void f12_copy(const PfRef& d, const PfRef& a) {
  for (uint32_t k = 0; k < PF_WORDS; ++k) d.p[(size_t)k * d.s] = a.p[(size_t)k * a.s];
}

// d = a b (SQR: d = a a, b unused) over the powers of b that `bmask` names; d must be neither a nor b.  At most 6 lazy terms a side.
template <bool SQR>
HM_HD void f12_mul(const PfRef& d, const PfRef& a, const PfRef& b, uint32_t bmask = 0x3fu) {
#pragma unroll 1
  for (uint32_t k = 0; k < 6; ++k) {
    Fq2 lo = f2_zero(), hi = f2_zero();
    bool any_hi = false;
#pragma unroll 1
    for (uint32_t i = 0; i < 6; ++i) {
      const uint32_t j = i <= k ? k - i : k + 6u - i;
      if (SQR ? j < i : ((bmask >> j) & 1u) == 0) continue;
      Fq2 t = f2_mul(pf_load2(a, pf_coeff(i)), pf_load2(SQR ? a : b, pf_coeff(j)));
      if (SQR && j > i) t = f2_add_lazy(t, t);
      if (i > k) {
        hi = f2_add_lazy(hi, t);
        any_hi = true;
      } else {
        lo = f2_add_lazy(lo, t);
      }
    }
    if (any_hi) lo = f2_add_lazy(lo, f2_mul_xi(Fq2{fe_norm(hi.c0), fe_norm(hi.c1)}));
    pf_store2(d, pf_coeff(k), Fq2{pf_red(lo.c0), pf_red(lo.c1)});
  }
}

// a^(p^6): the odd powers change sign.  In place.
HM_HD void f12_conj(const PfRef& d) {
  for (uint32_t c = 3; c < 6; ++c) pf_store2(d, c, f2_neg(pf_load2(d, c)));
}

template <int N, int K>
HM_HD Fq2 pf_frob_const() {
  return Fq2{fe_const<FqParams>(PairingParams::FROB[((N - 1) * 6 + K) * 2]), fe_const<FqParams>(PairingParams::FROB[((N - 1) * 6 + K) * 2 + 1])};
}
template <int N, int K>
HM_HD void f12_frob_one(const PfRef& d, const PfRef& a) {
  Fq2 c = pf_load2(a, pf_coeff(K));
  if (N & 1) c = f2_conj(c);
  if (K) c = f2_mul(c, pf_frob_const<N, K>());
  pf_store2(d, pf_coeff(K), c);
}
// d = a^(p^N), N = 1, 2, 3: coefficient by coefficient, so d may be a
template <int N>
HM_HD void f12_frob(const PfRef& d, const PfRef& a) {
  f12_frob_one<N, 0>(d, a);
  f12_frob_one<N, 1>(d, a);
  f12_frob_one<N, 2>(d, a);
  f12_frob_one<N, 3>(d, a);
  f12_frob_one<N, 4>(d, a);
  f12_frob_one<N, 5>(d, a);
}

// d = 1 / a through the norm to Fq2: g = prod_{i=1..5} a^(p^(2i)), a g in Fq2, d = g / (a g).  d, a, t0, t1 all different.
HM_HD void f12_inv(const PfRef& d, const PfRef& a, const PfRef& t0, const PfRef& t1) {
  f12_frob<2>(t0, a);
  f12_copy(d, t0);
  PfRef g = d, t = t1;
  for (int i = 2; i <= 5; ++i) {                 // four swaps: g ends in d
    f12_frob<2>(t0, t0);
    f12_mul<false>(t, g, t0);
    const PfRef o = g;
    g = t;
    t = o;
  }
  f12_mul<false>(t1, a, d);                      // the norm: only its coefficient of w^0 is not zero
  const Fq2 ninv = f2_inv(pf_load2(t1, 0));
  for (uint32_t c = 0; c < 6; ++c) pf_store2(d, c, f2_mul(pf_load2(d, c), ninv));
}

// (x0 + x1 s)^2 in Fq4 = Fq2[s] / (s^2 - xi): three Fq2 squares
HM_HD void f4_sqr(Fq2& r0, Fq2& r1, const Fq2& x0, const Fq2& x1) {
  const Fq2 t0 = f2_sqr(x0), t1 = f2_sqr(x1), s = f2_sqr(f2_add(x0, x1));
  r0 = f2_add(t0, f2_mul_xi(t1));
  r1 = f2_sub(f2_sub(s, t0), t1);
}
HM_HD Fq2 f2_triple(const Fq2& a) { return f2_add(f2_dbl(a), a); }

// d = a^2 for a in the cyclotomic subgroup (a^(p^6 + 1) = 1 and a^(p^4 - p^2 + 1) = 1: every value behind the easy part), after
// Granger and Scott: over Fq4 with s = w^3, a = A + B w + C w^2 for A = (a_0, a_3), B = (a_1, a_4), C = (a_2, a_5), and
// a^2 = (3 A^2 - 2 conj A) + (3 s C^2 + 2 conj B) w + (3 B^2 - 2 conj C) w^2: 9 Fq2 squares against 21 products.  d must not be a.
HM_HD void f12_cyc_sqr(const PfRef& d, const PfRef& a) {
  Fq2 x0 = pf_load2(a, pf_coeff(0)), x1 = pf_load2(a, pf_coeff(3)), s0, s1;
  f4_sqr(s0, s1, x0, x1);
  pf_store2(d, pf_coeff(0), f2_sub(f2_triple(s0), f2_dbl(x0)));
  pf_store2(d, pf_coeff(3), f2_add(f2_triple(s1), f2_dbl(x1)));
  x0 = pf_load2(a, pf_coeff(2)), x1 = pf_load2(a, pf_coeff(5));
  f4_sqr(s0, s1, x0, x1);                                       // C^2; s C^2 = (xi s1, s0)
  const Fq2 b0 = pf_load2(a, pf_coeff(1)), b1 = pf_load2(a, pf_coeff(4));
  pf_store2(d, pf_coeff(1), f2_add(f2_triple(f2_mul_xi(s1)), f2_dbl(b0)));
  pf_store2(d, pf_coeff(4), f2_sub(f2_triple(s0), f2_dbl(b1)));
  f4_sqr(s0, s1, b0, b1);                                       // B^2
  pf_store2(d, pf_coeff(2), f2_sub(f2_triple(s0), f2_dbl(x0)));
  pf_store2(d, pf_coeff(5), f2_add(f2_triple(s1), f2_dbl(x1)));
}

// d = a^x for the curve parameter x and a in the cyclotomic subgroup; d, a, t all different
HM_HD void f12_pow_x(const PfRef& d, const PfRef& a, const PfRef& t) {
  f12_copy(d, a);
  PfRef acc = d, tmp = t;
  for (int bit = 61; bit >= 0; --bit) {
    f12_cyc_sqr(tmp, acc);
    if ((PF_BN_X >> bit) & 1ull) {
      f12_mul<false>(acc, tmp, a);
    } else {
      const PfRef o = acc;
      acc = tmp;
      tmp = o;
    }
  }
  if (acc.p != d.p) f12_copy(d, acc);
}

// ---- the Miller loop of one pair ----------------------------------------------------------------------------------------------
struct G2Jac {
  Fq2 x, y, z;
};

// T <- 2T; the tangent at T evaluated at P = (xp, yp), times Z3 ZZ, into `line`
HM_HD void pf_double_step(G2Jac& t, const Fq& xp, const Fq& yp, const PfRef& line) {
  const Fq2 a = f2_sqr(t.x), b = f2_sqr(t.y), c = f2_sqr(b), zz = f2_sqr(t.z);
  const Fq2 d = f2_dbl(f2_dbl(f2_mul(t.x, b)));                       // 4 X Y^2
  const Fq2 e = f2_add(f2_dbl(a), a);                                 // 3 X^2
  const Fq2 x3 = f2_sub(f2_sqr(e), f2_dbl(d));
  const Fq2 y3 = f2_sub(f2_mul(e, f2_sub(d, x3)), f2_dbl(f2_dbl(f2_dbl(c))));
  const Fq2 z3 = f2_dbl(f2_mul(t.y, t.z));
  pf_store2(line, pf_coeff(0), f2_mul_fq(f2_mul(z3, zz), yp));
  pf_store2(line, pf_coeff(1), f2_neg(f2_mul_fq(f2_mul(e, zz), xp)));
  pf_store2(line, pf_coeff(3), f2_sub(f2_mul(e, t.x), f2_dbl(b)));
  t.x = x3;
  t.y = y3;
  t.z = z3;
}

// T <- T + Q for affine Q; the chord evaluated at P, times Z3, into `line`
HM_HD void pf_add_step(G2Jac& t, const Fq2& qx, const Fq2& qy, const Fq& xp, const Fq& yp, const PfRef& line) {
  const Fq2 zz = f2_sqr(t.z);
  const Fq2 h = f2_sub(f2_mul(qx, zz), t.x), r = f2_sub(f2_mul(qy, f2_mul(t.z, zz)), t.y);
  const Fq2 hh = f2_sqr(h);
  const Fq2 hhh = f2_mul(h, hh), v = f2_mul(t.x, hh);
  const Fq2 x3 = f2_sub(f2_sub(f2_sqr(r), hhh), f2_dbl(v));
  const Fq2 y3 = f2_sub(f2_mul(r, f2_sub(v, x3)), f2_mul(t.y, hhh));
  const Fq2 z3 = f2_mul(t.z, h);
  pf_store2(line, pf_coeff(0), f2_mul_fq(z3, yp));
  pf_store2(line, pf_coeff(1), f2_neg(f2_mul_fq(r, xp)));
  pf_store2(line, pf_coeff(3), f2_sub(f2_mul(r, qx), f2_mul(z3, qy)));
  t.x = x3;
  t.y = y3;
  t.z = z3;
}

HM_HD bool pf_words_canonical(const uint32_t* w) {
  bool lt = false, eq = true;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    lt = lt || (eq && w[k] < FqParams::MOD32[k]);
    eq = eq && w[k] == FqParams::MOD32[k];
  }
  return lt;
}
HM_HD Fq pf_from_ext(const uint32_t* w) {
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = w[k];
  return fe_from_ext<FqParams>(v);
}
HM_HD bool pf_equal_mod(const Fq& a, const Fq& b) {   // both class R
  return fe_is_zero_mod(fe_mul(fe_norm(fe_sub<4, 29>(a, b)), fe_one<FqParams>()));
}

constexpr uint32_t PF_PAIR_OK = 0, PF_PAIR_ONE = 1, PF_PAIR_BAD = 2;

// p: x, y of P (8 words each, Montgomery); q: x.c0, x.c1, y.c0, y.c1 of Q.  -> PF_PAIR_OK with the Miller value in slot 0 of `lane`;
// PF_PAIR_ONE for an identity on either side (the pair contributes 1, slot 0 is not written); PF_PAIR_BAD for a coordinate word
// >= p or a point off its curve (y^2 = x^3 + 3; on the twist y^2 = x^3 + 3 / xi).
HM_HD uint32_t pf_miller_lane(const uint32_t (&p)[16], const uint32_t (&q)[32], const PfLane& lane) {
  uint32_t any_p = 0, any_q = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) any_p |= p[k];
#pragma unroll
  for (int k = 0; k < 32; ++k) any_q |= q[k];
  bool ok = pf_words_canonical(p) && pf_words_canonical(p + 8);
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok && pf_words_canonical(q + 8 * k);
  if (!ok) return PF_PAIR_BAD;
  const Fq xp = pf_from_ext(p), yp = pf_from_ext(p + 8);
  const Fq2 qx{pf_from_ext(q), pf_from_ext(q + 8)}, qy{pf_from_ext(q + 16), pf_from_ext(q + 24)};
  if (any_p) {
    const Fq one = fe_one<FqParams>();
    const Fq rhs = pf_red(fe_add(fe_add(fe_mul(fe_sqr(xp), xp), one), fe_add(one, one)));
    if (!pf_equal_mod(fe_sqr(yp), rhs)) return PF_PAIR_BAD;
  }
  if (any_q) {
    const Fq2 b{fe_const<FqParams>(PairingParams::TWIST_B0), fe_const<FqParams>(PairingParams::TWIST_B1)};
    const Fq2 rhs = f2_add(f2_mul(f2_sqr(qx), qx), b), lhs = f2_sqr(qy);
    if (!pf_equal_mod(lhs.c0, rhs.c0) || !pf_equal_mod(lhs.c1, rhs.c1)) return PF_PAIR_BAD;
  }
  if (!any_p || !any_q) return PF_PAIR_ONE;

  PfRef f = lane.slot(0), tmp = lane.slot(1);
  const PfRef line = lane.slot(2);
  f12_one(f);
  G2Jac t{qx, qy, f2_one()};
  for (int bit = 63; bit >= 0; --bit) {
    f12_mul<true>(tmp, f, f);
    pf_double_step(t, xp, yp, line);
    f12_mul<false>(f, tmp, line, PF_LINE_MASK);
    if ((PF_ATE_LOW >> bit) & 1ull) {
      pf_add_step(t, qx, qy, xp, yp, line);
      f12_mul<false>(tmp, f, line, PF_LINE_MASK);
      const PfRef o = f;
      f = tmp;
      tmp = o;
    }
  }
  // Q1 = Q^p, -Q2 = -Q^(p^2): x -> conj(x) gamma_2, y -> conj(y) gamma_3
  const Fq2 q1x = f2_mul(f2_conj(qx), pf_frob_const<1, 2>()), q1y = f2_mul(f2_conj(qy), pf_frob_const<1, 3>());
  const Fq2 q2x = f2_mul(f2_conj(q1x), pf_frob_const<1, 2>()), nq2y = f2_neg(f2_mul(f2_conj(q1y), pf_frob_const<1, 3>()));
  pf_add_step(t, q1x, q1y, xp, yp, line);
  f12_mul<false>(tmp, f, line, PF_LINE_MASK);
  pf_add_step(t, q2x, nq2y, xp, yp, line);
  f12_mul<false>(f, tmp, line, PF_LINE_MASK);
  if (f.p != lane.slot(0).p) f12_copy(lane.slot(0), f);
  return PF_PAIR_OK;
}

// ---- the product and the final exponentiation of one check ---------------------------------------------------------------------
// The steps behind the product, as (op, d, a, b) on the check's slots; slots 9 and 10 are the temporaries of INV and POWX.
enum : uint32_t { PF_MUL, PF_SQR, PF_CONJ, PF_FROB1, PF_FROB2, PF_FROB3, PF_POWX, PF_INV };
constexpr uint32_t PF_STEPS = 37, PF_RESULT = 6;
HM_HD uint32_t pf_step(uint32_t i) {
#define PF_OP(op, d, a, b) ((uint32_t)(op) | ((uint32_t)(d) << 4) | ((uint32_t)(a) << 8) | ((uint32_t)(b) << 12))
  switch (i) {
    case 0: return PF_OP(PF_INV, 1, 0, 0);      // 1 / f
    case 1: return PF_OP(PF_CONJ, 0, 0, 0);
    case 2: return PF_OP(PF_MUL, 2, 0, 1);      // f^(p^6 - 1)
    case 3: return PF_OP(PF_FROB2, 1, 2, 0);
    case 4: return PF_OP(PF_MUL, 0, 1, 2);      // m = f^((p^6 - 1)(p^2 + 1))
    case 5: return PF_OP(PF_POWX, 1, 0, 0);     // a = m^x
    case 6: return PF_OP(PF_POWX, 2, 1, 0);     // b = m^(x^2)
    case 7: return PF_OP(PF_POWX, 3, 2, 0);     // c = m^(x^3)
    case 8: return PF_OP(PF_SQR, 4, 3, 0);      // c^2
    case 9: return PF_OP(PF_SQR, 5, 4, 0);      // c^4
    case 10: return PF_OP(PF_MUL, 6, 5, 4);     // c^6
    case 11: return PF_OP(PF_SQR, 4, 2, 0);     // b^2
    case 12: return PF_OP(PF_MUL, 5, 4, 2);     // b^3
    case 13: return PF_OP(PF_SQR, 4, 1, 0);     // a^2
    case 14: return PF_OP(PF_MUL, 7, 6, 5);     // c^6 b^3
    case 15: return PF_OP(PF_MUL, 6, 7, 4);     // t = c^6 b^3 a^2
    case 16: return PF_OP(PF_SQR, 7, 6, 0);     // t^2
    case 17: return PF_OP(PF_SQR, 8, 7, 0);     // t^4
    case 18: return PF_OP(PF_MUL, 6, 8, 7);     // y = t^6 = c^36 b^18 a^12
    case 19: return PF_OP(PF_SQR, 7, 5, 0);     // b^6
    case 20: return PF_OP(PF_SQR, 8, 7, 0);     // b^12
    case 21: return PF_OP(PF_SQR, 5, 4, 0);     // a^4
    case 22: return PF_OP(PF_MUL, 9, 5, 4);     // a^6
    case 23: return PF_OP(PF_MUL, 5, 8, 9);     // b^12 a^6
    case 24: return PF_OP(PF_SQR, 8, 0, 0);     // m^2
    case 25: return PF_OP(PF_MUL, 9, 5, 8);     // b^12 a^6 m^2
    case 26: return PF_OP(PF_MUL, 5, 9, 6);     // c^36 b^30 a^18 m^2
    case 27: return PF_OP(PF_CONJ, 5, 0, 0);    // m^l0
    case 28: return PF_OP(PF_CONJ, 6, 0, 0);    // 1 / y
    case 29: return PF_OP(PF_MUL, 8, 6, 0);     // m^l1
    case 30: return PF_OP(PF_FROB1, 8, 8, 0);
    case 31: return PF_OP(PF_MUL, 9, 7, 0);     // m^l2 = b^6 m
    case 32: return PF_OP(PF_FROB2, 9, 9, 0);
    case 33: return PF_OP(PF_FROB3, 4, 0, 0);   // m^(p^3)
    case 34: return PF_OP(PF_MUL, 6, 5, 8);
    case 35: return PF_OP(PF_MUL, 5, 6, 9);
    default: return PF_OP(PF_MUL, 6, 5, 4);     // the result: PF_RESULT
  }
#undef PF_OP
}

HM_HD void pf_run_step(const PfLane& lane, uint32_t code) {
  const PfRef d = lane.slot((code >> 4) & 15u), a = lane.slot((code >> 8) & 15u), b = lane.slot((code >> 12) & 15u);
  switch (code & 15u) {
    case PF_MUL: f12_mul<false>(d, a, b); break;
    case PF_SQR: f12_cyc_sqr(d, a); break;      // every square of the program stands behind the easy part
    case PF_CONJ: f12_conj(d); break;
    case PF_FROB1: f12_frob<1>(d, a); break;
    case PF_FROB2: f12_frob<2>(d, a); break;
    case PF_FROB3: f12_frob<3>(d, a); break;
    case PF_POWX: f12_pow_x(d, a, lane.slot(10)); break;
    default: f12_inv(d, a, lane.slot(9), lane.slot(10)); break;
  }
}

// slot 0 of `lane` holds f -> slot PF_RESULT holds f^((p^12 - 1) / r)
HM_HD void pf_final_exponentiation(const PfLane& lane) {
#pragma unroll 1
  for (uint32_t i = 0; i < PF_STEPS; ++i) {
    pf_run_step(lane, pf_step(i));
  }
}

// The check over pairs [lo, hi): `pairs` is pair 0's lane of the Miller kernel's slots (pair j: base + j), flags its PF_PAIR_* words.
// -> status 0 / 1 / 2; gt (48 x 8 words, pairing.py's order, canonical Montgomery) when not null -- zeros with status 2.
HM_HD uint32_t pf_finish_lane(uint64_t lo, uint64_t hi, uint64_t n_pairs, const PfLane& pairs, const uint32_t* flags, const PfLane& lane,
                              uint32_t* gt) {
  bool bad = lo > hi || hi > n_pairs;
  if (!bad)
    for (uint64_t j = lo; j < hi; ++j) bad = bad || flags[j] == PF_PAIR_BAD;
  if (bad) {
    if (gt)
      for (uint32_t k = 0; k < PF_WORDS; ++k) gt[k] = 0;
    return 2;
  }
  uint32_t acc = 0, tmp = 1;
  f12_one(lane.slot(acc));
  for (uint64_t j = lo; j < hi; ++j) {
    if (flags[j] != PF_PAIR_OK) continue;
    f12_mul<false>(lane.slot(tmp), lane.slot(acc), PfRef{pairs.base + j, pairs.stride});
    const uint32_t o = acc;
    acc = tmp;
    tmp = o;
  }
  if (acc != 0) f12_copy(lane.slot(0), lane.slot(acc));
  pf_final_exponentiation(lane);
  const PfRef r = lane.slot(PF_RESULT);
  uint32_t diff = 0, one_w[8];
  fe_to_ext(one_w, fe_one<FqParams>());
  for (uint32_t c = 0; c < 12; ++c) {
    uint32_t w[8];
    fe_to_ext(w, pf_load(r, c * 8u));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      diff |= w[k] ^ (c == 0 ? one_w[k] : 0u);
      if (gt) gt[c * 8u + k] = w[k];
    }
  }
  return diff == 0 ? 1u : 0u;
}
