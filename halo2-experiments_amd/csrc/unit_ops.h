// unit_ops.h -- every primitive of ff29.h and g1.h as one op over RAW limbs, for the unit tests on the host
// (tests/unit_ops_host.cpp) and on the device (devcheck.hip).  Not part of the product library.
//
// An op reads one fixed-size record of u32 words and writes one; operands and results are the internal limbs as they
// are, with no conversion on the way in or out, so the caller chooses the representative of every residue and the
// laziness of every limb.  Beside the limbs a record carries the class each operand is declared at: under -DHM_BOUNDS
// that becomes the operand's (vb, lb, tb), which puts the tracker's preconditions in force for that class (and a limb
// above its declared bound aborts); the other builds ignore it.
//
// Field record (templates over FqParams / FrParams):
//   in  [FIELD_IN_WORDS]:  operand i's 9 limbs at 9*i (i < 6), its class at 54 + 4*i: lb, tb, the double vb as lo, hi word
//                          (unpack / from_ext: the 8 packed words at 0); word 78: bit i set = operand i's tb is the top limb
//                          its value bound implies, which the tracker's own rule must reproduce
//   out [FIELD_OUT_WORDS]: result i's 9 limbs at 9*i (i < 3; pack / to_ext: 8 packed words at 0), a returned bool at 27;
//                          under -DHM_BOUNDS also what the tracker derived for result i, at 32 + 4*i: lb, tb, the double vb as
//                          lo, hi word, and 1 at word 44 (the other builds leave all of these 0)
// Curve record:
//   in  [CURVE_IN_WORDS]:  first point at 0: X, Y, Z (27 limbs) or X, Y, ZZ, ZZZ (36 limbs), its identity flag at 36;
//                          second operand at 40: affine x, y (18 limbs) or X, Y, Z with its identity flag at 67; neg at 68;
//                          the classes (value bounds in multiples of p) of the first point's coordinates at 70..73, of the
//                          second operand's at 74..76
//   out [CURVE_OUT_WORDS]: the point at 0 in its form (affine 18, Jacobian 27, XYZZ 36 limbs), its identity flag at 36,
//                          a returned bool at 37
#pragma once
#include <string.h>

#include "g1.h"

namespace hm {
namespace unit {

constexpr int FIELD_IN_WORDS = 80, FIELD_OUT_WORDS = 48, CURVE_IN_WORDS = 80, CURVE_OUT_WORDS = 40;

// one line per op: tests/ff29_model.py reads the numbers from here
enum FieldOp : int {
  UF_MUL = 0,
  UF_SQR = 1,
  UF_MUL2 = 2,
  UF_MUL_X2 = 3,
  UF_MUL_X3 = 4,
  UF_SQR_X2 = 5,
  UF_MUL_MUL2 = 6,
  UF_ADD = 7,
  UF_DBL = 8,
  UF_MUL4 = 9,
  UF_NORM = 10,
  UF_IS_ZERO_MOD = 11,
  UF_CANONICAL = 12,
  UF_REDUCE_SMALL = 13,
  UF_UNPACK = 14,
  UF_PACK = 15,
  UF_FROM_EXT = 16,
  UF_TO_EXT = 17,
  // fe_sub<K, BITS>: every instantiation in csrc/ (tests/test_unit_ops_host.py searches the sources for them)
  UF_SUB_3_29 = 20,
  UF_SUB_4_29 = 21,
  UF_SUB_6_29 = 22,
  UF_SUB_7_29 = 23,
  UF_SUB_9_29 = 24,
  UF_SUB_13_29 = 25,
  UF_SUB_20_29 = 26,
  UF_SUB_9_30 = 27,
  UF_SUB_10_30 = 28,
  UF_SUB_4_31 = 29,
  UF_SUB_6_31 = 30,
  UF_OP_END = 31,
};
enum CurveOp : int {
  UC_NEG_AFFINE = 0,
  UC_DOUBLE_NZ = 1,
  UC_MADD_NZ = 2,
  UC_ADD_NZ = 3,
  UC_XMADD_FAST = 4,
  UC_XMADD_FAST_LOCKSTEP = 5,
  UC_X_TO_JAC = 6,
  UC_X_FROM_JAC = 7,
  UC_XMADD = 8,
  UC_MADD = 9,
  UC_ADD = 10,
  UC_OP_END = 11,
};

// ---- records <-> elements --------------------------------------------------------------------------------------
template <class F>
HM_HD Fe<F> load_fe(const uint32_t* limbs, const uint32_t* cls, bool tb_from_vb) {
  Fe<F> a;
#pragma unroll
  for (int i = 0; i < 9; ++i) a.l[i] = limbs[i];
#ifdef HM_BOUNDS
  const uint64_t bits = (uint64_t)cls[2] | ((uint64_t)cls[3] << 32);
  double vb;
  memcpy(&vb, &bits, 8);
  set_bounds(a, vb, cls[0], cls[1]);
  for (int i = 0; i < 8; ++i) HM_CHECK(a.l[i] <= a.lb, "unit op: an operand's limb exceeds its declared bound");
  HM_CHECK(a.l[8] <= a.tb, "unit op: an operand's top limb exceeds its declared bound");
  if (tb_from_vb) HM_CHECK(a.tb == top_bound_from_value<F>(vb), "unit op: top_bound_from_value disagrees with the declared class");
#else
  (void)cls;
  (void)tb_from_vb;
#endif
  return a;
}
// a curve coordinate: normalised limbs, value < vb_p * p
HM_HD Fq load_coord(const uint32_t* limbs, uint32_t vb_p) {
  Fq a;
#pragma unroll
  for (int i = 0; i < 9; ++i) a.l[i] = limbs[i];
#ifdef HM_BOUNDS
  declare(a, (double)vb_p);
#else
  (void)vb_p;
#endif
  return a;
}
template <class F>
HM_HD void store_fe(uint32_t* out, const Fe<F>& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = a.l[i];
}

// result i of a field op: its limbs, and under HM_BOUNDS the bounds the tracker derived for it
template <class F>
HM_HD void store_res(uint32_t* out, int i, const Fe<F>& a) {
  store_fe(out + 9 * i, a);
#ifdef HM_BOUNDS
  uint64_t bits;
  memcpy(&bits, &a.vb, 8);
  out[32 + 4 * i] = (uint32_t)a.lb;
  out[33 + 4 * i] = (uint32_t)a.tb;
  out[34 + 4 * i] = (uint32_t)bits;
  out[35 + 4 * i] = (uint32_t)(bits >> 32);
#endif
}

template <class F, int K, int BITS>
HM_HD void sub_op(const uint32_t* in, uint32_t* out) {
  store_res(out, 0, fe_sub<K, BITS>(load_fe<F>(in, in + 54, in[78] & 1u), load_fe<F>(in + 9, in + 58, in[78] & 2u)));
}

// ---- the field table ---------------------------------------------------------------------------------------------
// false: no such op (nothing written)
template <class F>
HM_HD bool field_op(int op, const uint32_t* in, uint32_t* out) {
  auto A = [&](int i) { return load_fe<F>(in + 9 * i, in + 54 + 4 * i, (in[78] >> i) & 1u); };
  Fe<F> r0, r1, r2;
  uint32_t w[8];
#ifdef HM_BOUNDS
  out[44] = 1u;
#endif
  switch (op) {
    case UF_MUL: store_res(out, 0, fe_mul(A(0), A(1))); return true;
    case UF_SQR: store_res(out, 0, fe_sqr(A(0))); return true;
    case UF_MUL2: store_res(out, 0, fe_mul2(A(0), A(1), A(2), A(3))); return true;
    case UF_MUL_X2:
      fe_mul_x2(r0, r1, A(0), A(1), A(2), A(3));
      store_res(out, 0, r0);
      store_res(out, 1, r1);
      return true;
    case UF_MUL_X3:
      fe_mul_x3(r0, r1, r2, A(0), A(1), A(2), A(3), A(4), A(5));
      store_res(out, 0, r0);
      store_res(out, 1, r1);
      store_res(out, 2, r2);
      return true;
    case UF_SQR_X2:
      fe_sqr_x2(r0, r1, A(0), A(1));
      store_res(out, 0, r0);
      store_res(out, 1, r1);
      return true;
    case UF_MUL_MUL2:
      fe_mul_mul2(r0, r1, A(0), A(1), A(2), A(3), A(4), A(5));
      store_res(out, 0, r0);
      store_res(out, 1, r1);
      return true;
    case UF_ADD: store_res(out, 0, fe_add(A(0), A(1))); return true;
    case UF_DBL: store_res(out, 0, fe_dbl(A(0))); return true;
    case UF_MUL4: store_res(out, 0, fe_mul4(A(0))); return true;
    case UF_NORM: store_res(out, 0, fe_norm(A(0))); return true;
    case UF_IS_ZERO_MOD: out[27] = fe_is_zero_mod(A(0)) ? 1u : 0u; return true;
    case UF_CANONICAL: store_res(out, 0, fe_canonical(A(0))); return true;
    case UF_REDUCE_SMALL: store_res(out, 0, fe_reduce_small(A(0))); return true;
    case UF_UNPACK:
    case UF_FROM_EXT:
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = in[i];
      store_res(out, 0, op == UF_UNPACK ? fe_unpack<F>(w) : fe_from_ext<F>(w));
      return true;
    case UF_PACK:
    case UF_TO_EXT:
      if (op == UF_PACK) fe_pack(w, A(0));
      else fe_to_ext(w, A(0));
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = w[i];
      return true;
    case UF_SUB_3_29: sub_op<F, 3, 29>(in, out); return true;
    case UF_SUB_4_29: sub_op<F, 4, 29>(in, out); return true;
    case UF_SUB_6_29: sub_op<F, 6, 29>(in, out); return true;
    case UF_SUB_7_29: sub_op<F, 7, 29>(in, out); return true;
    case UF_SUB_9_29: sub_op<F, 9, 29>(in, out); return true;
    case UF_SUB_13_29: sub_op<F, 13, 29>(in, out); return true;
    case UF_SUB_20_29: sub_op<F, 20, 29>(in, out); return true;
    case UF_SUB_9_30: sub_op<F, 9, 30>(in, out); return true;
    case UF_SUB_10_30: sub_op<F, 10, 30>(in, out); return true;
    case UF_SUB_4_31: sub_op<F, 4, 31>(in, out); return true;
    case UF_SUB_6_31: sub_op<F, 6, 31>(in, out); return true;
  }
  return false;
}

// ---- the curve table ---------------------------------------------------------------------------------------------
HM_HD G1Jac load_jac(const uint32_t* limbs, uint32_t inf, const uint32_t* cls) {
  G1Jac p;
  p.x = load_coord(limbs, cls[0]);
  p.y = load_coord(limbs + 9, cls[1]);
  p.z = load_coord(limbs + 18, cls[2]);
  p.inf = inf != 0;
  return p;
}
HM_HD G1Xyzz load_xyzz(const uint32_t* limbs, uint32_t inf, const uint32_t* cls) {
  G1Xyzz p;
  p.x = load_coord(limbs, cls[0]);
  p.y = load_coord(limbs + 9, cls[1]);
  p.zz = load_coord(limbs + 18, cls[2]);
  p.zzz = load_coord(limbs + 27, cls[3]);
  p.inf = inf != 0;
  return p;
}
HM_HD G1Aff load_aff(const uint32_t* limbs, const uint32_t* cls) {
  G1Aff q;
  q.x = load_coord(limbs, cls[0]);
  q.y = load_coord(limbs + 9, cls[1]);
  return q;
}
HM_HD void store_jac(uint32_t* out, const G1Jac& p) {
  store_fe(out, p.x);
  store_fe(out + 9, p.y);
  store_fe(out + 18, p.z);
  out[36] = p.inf ? 1u : 0u;
}
HM_HD void store_xyzz(uint32_t* out, const G1Xyzz& p) {
  store_fe(out, p.x);
  store_fe(out + 9, p.y);
  store_fe(out + 18, p.zz);
  store_fe(out + 27, p.zzz);
  out[36] = p.inf ? 1u : 0u;
}

HM_HD bool curve_op(int op, const uint32_t* in, uint32_t* out) {
  const uint32_t *cls1 = in + 70, *cls2 = in + 74;
  const bool neg = in[68] != 0;
  switch (op) {
    case UC_NEG_AFFINE: {
      const G1Aff r = g1_neg_affine(load_aff(in + 40, cls2));
      store_fe(out, r.x);
      store_fe(out + 9, r.y);
      return true;
    }
    case UC_DOUBLE_NZ: store_jac(out, g1_double_nz(load_jac(in, in[36], cls1))); return true;
    case UC_MADD_NZ: store_jac(out, g1_madd_nz(load_jac(in, in[36], cls1), load_aff(in + 40, cls2), neg)); return true;
    case UC_ADD_NZ: store_jac(out, g1_add_nz(load_jac(in, in[36], cls1), load_jac(in + 40, in[67], cls2))); return true;
    case UC_XMADD_FAST:
    case UC_XMADD_FAST_LOCKSTEP: {
      G1Xyzz acc = load_xyzz(in, in[36], cls1);
      const G1Aff q = load_aff(in + 40, cls2);
      const bool done = op == UC_XMADD_FAST ? g1x_madd_fast<false>(acc, q, neg) : g1x_madd_fast<true>(acc, q, neg);
      store_xyzz(out, acc);
      out[37] = done ? 1u : 0u;
      return true;
    }
    case UC_X_TO_JAC: store_jac(out, g1x_to_jac(load_xyzz(in, in[36], cls1))); return true;
    case UC_X_FROM_JAC: store_xyzz(out, g1x_from_jac(load_jac(in, in[36], cls1))); return true;
    case UC_XMADD: store_xyzz(out, g1x_madd(load_xyzz(in, in[36], cls1), load_aff(in + 40, cls2), neg)); return true;
    case UC_MADD: store_jac(out, g1_madd(load_jac(in, in[36], cls1), load_aff(in + 40, cls2), neg)); return true;
    case UC_ADD: store_jac(out, g1_add(load_jac(in, in[36], cls1), load_jac(in + 40, in[67], cls2))); return true;
  }
  return false;
}

}  // namespace unit
}  // namespace hm
