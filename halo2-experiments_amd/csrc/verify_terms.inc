// verify_terms.inc -- the per-proof arithmetic of a batch verification on the device, one lane per proof (batch_verifier.py is the
// caller, DESIGN.md section 20): from a proof's evaluations, its instance values and its challenges to r_b x the scalar of every point
// of its opening check.
//
// A PLAN, built once per constraint system on the host (batch_verifier.TermsPlan) and checked word by word before every launch
// (vt_plan_problem), drives every loop: a header, a (column, rotation index) -> value slot map, the instance queries, the rotation sets
// and a block of constants in internal form (1 / n, the powers of omega the Lagrange values and the rotations need, the inverse of
// every prod_{m != l} (omega^r_l - omega^r_m) of a set).  It travels into the slot's argument buffer with the call, as the witness
// checker's column table does: no kernel reads a table from its kernarg segment.
//
// Every runtime-indexed per-lane array lives in ONE workspace in the interpreter's [slot][word][lane] layout, never in a local array:
//   [0, n_vals)            the value row: the proof's evaluations, then l0, l_last, l_active, x, the instance columns' evaluations, h(x)
//   [n_vals, +11)          the challenge record theta, beta, gamma, y, x, y', v, u, r_b, then x^n and 1 / (x^n - 1)
//   then n_super slots     u - x omega^rot for every rotation of the super point set
//   then VT_MAX_T slots    the Lagrange basis of the current set's points at u
//   then the program's     intermediates of ge_run (graph_interp.h)
// Every element kept there is normalised and below 3r.  An inversion is a^(r-2) in a rolled loop: the inverse of zero is zero, the
// lane is flagged and writes zero rows -- never a fault.
//
//   phase a   record and evaluations to internal form; x^n by k squarings; l0, l_last, l_blind, l_active at x; every instance
//             query sum_i v_i l_i(x omega^rot) over the rows given
//   ge_run    the numerator: the gate, permutation and lookup expressions folded in y -- the program hm_graph_create lowered from the
//             constraint system alone, through a Source whose column(src) is a slot of this lane's value row, whose dyn(word) is this
//             lane's challenge record and whose PreviousValue is zero
//   phase b   h(x) = numerator / (x^n - 1); per rotation set z_i, the basis at u, the powers of y' and v; r_b x the scalars of the
//             proof's own points (the h commitment expanded into its pieces with the powers of x^n), its row of the shared points'
//             array, and r_b u, r_b for [h'].
// The two phases are host-callable: host_check.cpp runs them under bound tracking (hc_verify_terms) with the numerator given.
// Included inside namespace hm by verify.hip, which holds the kernel and its driver, and by capi_verify.hip for the plan's check.

enum : uint32_t {
  VT_K, VT_N_SCALARS, VT_N_VALS, VT_N_LAGRANGE, VT_N_INSTQ, VT_N_SUPER, VT_N_SETS, VT_PIECES, VT_N_OWN, VT_N_SHARED, VT_N_ROT, VT_N_COLS,
  VT_OFF_COLMAP, VT_OFF_INST, VT_OFF_SETS, VT_INST_ELEMS, VT_C_LAGRANGE, VT_C_ROWS, VT_C_SUPER, VT_S_L0, VT_S_INST, VT_S_HX, VT_N_CONSTS,
  VT_OFF_CONSTS, VT_HDR
};
constexpr uint32_t VT_MAX_VALS = 256, VT_MAX_INST_ROWS = 64, VT_MAX_SUPER = 32, VT_MAX_T = 8, VT_NO_SLOT = 0xffffffffu;
constexpr uint32_t VT_T_SHARED = 1u << 31, VT_T_H = 1u << 30, VT_T_INDEX = VT_T_H - 1u;
enum : uint32_t { VT_THETA, VT_BETA, VT_GAMMA, VT_Y, VT_X, VT_Y2, VT_V, VT_U, VT_RB, VT_XN, VT_XN1_INV, VT_REC_SLOTS };
constexpr uint32_t VT_REC = 9;                                   // elements of the record the caller uploads

HM_HD uint32_t vt_ws_diff(const uint32_t* plan) { return plan[VT_N_VALS] + VT_REC_SLOTS; }
HM_HD uint32_t vt_ws_basis(const uint32_t* plan) { return vt_ws_diff(plan) + plan[VT_N_SUPER]; }
HM_HD uint32_t vt_ws_program(const uint32_t* plan) { return vt_ws_basis(plan) + VT_MAX_T; }

// nullptr, or why the plan is refused: after this every index the kernel takes from the plan lies inside its array
inline const char* vt_plan_problem(const uint32_t* p, size_t n_words, size_t n_columns) {
  if (n_words < VT_HDR) return "verify terms: the plan is shorter than its header";
  if (p[VT_K] == 0 || p[VT_K] > 28) return "verify terms: need 1 <= k <= 28";
  const uint32_t n_vals = p[VT_N_VALS], n_consts = p[VT_N_CONSTS], n_super = p[VT_N_SUPER];
  if (n_vals > VT_MAX_VALS) return "verify terms: more than 256 value slots";
  if (p[VT_N_SCALARS] > n_vals || p[VT_S_L0] > n_vals || n_vals - p[VT_S_L0] < 4 || p[VT_S_HX] >= n_vals || p[VT_S_INST] > n_vals ||
      p[VT_N_INSTQ] > n_vals - p[VT_S_INST])
    return "verify terms: a value slot of the plan lies outside the value row";
  if (n_super == 0 || n_super > VT_MAX_SUPER || p[VT_N_SETS] == 0) return "verify terms: need 1 .. 32 rotations and at least one set";
  if (p[VT_N_LAGRANGE] < 2 || p[VT_N_LAGRANGE] > (1u << 16)) return "verify terms: need l0 and l_last";
  if (p[VT_N_OWN] == 0 || p[VT_N_OWN] > (1u << 16) || p[VT_N_SHARED] == 0 || p[VT_N_SHARED] > (1u << 16) || p[VT_PIECES] > p[VT_N_OWN])
    return "verify terms: output sizes out of range";
  if (p[VT_N_COLS] != n_columns || p[VT_N_ROT] > 1024) return "verify terms: the plan was built for another number of columns";
  const uint64_t words = n_words;
  if (n_consts == 0 || n_consts > (1u << 16) || p[VT_OFF_CONSTS] > words || (uint64_t)n_consts * 9 > words - p[VT_OFF_CONSTS])
    return "verify terms: the constants lie outside the plan";
  auto consts_ok = [&](uint32_t first, uint32_t count) { return first <= n_consts && count <= n_consts - first; };
  if (!consts_ok(p[VT_C_LAGRANGE], p[VT_N_LAGRANGE]) || !consts_ok(p[VT_C_SUPER], n_super)) return "verify terms: a constant index out of range";
  const uint64_t map_words = (uint64_t)p[VT_N_COLS] * p[VT_N_ROT];
  if (p[VT_OFF_COLMAP] > words || map_words > words - p[VT_OFF_COLMAP]) return "verify terms: the column map lies outside the plan";
  for (uint64_t i = 0; i < map_words; ++i) {
    const uint32_t s = p[p[VT_OFF_COLMAP] + i];
    if (s != VT_NO_SLOT && s >= n_vals) return "verify terms: the column map names a slot outside the value row";
  }
  if (p[VT_OFF_INST] > words || (uint64_t)p[VT_N_INSTQ] * 3 > words - p[VT_OFF_INST]) return "verify terms: the instance queries lie outside the plan";
  for (uint32_t q = 0; q < p[VT_N_INSTQ]; ++q) {
    const uint32_t* e = p + p[VT_OFF_INST] + 3 * (size_t)q;
    if (e[1] > VT_MAX_INST_ROWS) return "verify terms: an instance column longer than 64 rows";
    if (e[0] > p[VT_INST_ELEMS] || e[1] > p[VT_INST_ELEMS] - e[0] || e[2] >= n_consts || !consts_ok(p[VT_C_ROWS], e[1]))
      return "verify terms: an instance query out of range";
  }
  uint64_t at = p[VT_OFF_SETS];
  for (uint32_t i = 0; i < p[VT_N_SETS]; ++i) {
    if (at + 3 > words) return "verify terms: the sets lie outside the plan";
    const uint32_t t = p[at], members = p[at + 2];
    if (t == 0 || t > VT_MAX_T || at + 3 + 2ull * t > words) return "verify terms: a set needs 1 .. 8 points";
    for (uint32_t l = 0; l < t; ++l)
      if (p[at + 3 + l] >= n_super || p[at + 3 + t + l] >= n_consts) return "verify terms: a set's point or constant out of range";
    at += 3 + 2ull * t;
    for (uint32_t j = 0; j < members; ++j) {
      if (at + 1 + t > words) return "verify terms: the sets lie outside the plan";
      const uint32_t target = p[at], index = target & VT_T_INDEX;
      if (target & VT_T_H ? ((target & VT_T_SHARED) || index > p[VT_N_OWN] || p[VT_PIECES] > p[VT_N_OWN] - index)
                          : (index >= (target & VT_T_SHARED ? p[VT_N_SHARED] : p[VT_N_OWN])))
        return "verify terms: a member's target out of range";
      for (uint32_t l = 0; l < t; ++l)
        if (p[at + 1 + l] >= n_vals) return "verify terms: a member's evaluation slot out of range";
      at += 1 + t;
    }
  }
  return nullptr;
}

struct VtMem {
  uint32_t* ws;
  uint32_t T, lane;
};

HM_HD Fr vt_load(const VtMem& m, uint32_t slot) {
  const uint32_t* p = m.ws + (size_t)slot * 9 * m.T + m.lane;
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = p[(size_t)i * m.T];
  HM_DECLARE(r, 3.0);
  return r;
}
HM_HD void vt_store(const VtMem& m, uint32_t slot, const Fr& a) {
  uint32_t* p = m.ws + (size_t)slot * 9 * m.T + m.lane;
#pragma unroll
  for (int i = 0; i < 9; ++i) p[(size_t)i * m.T] = a.l[i];
}
HM_HD Fr vt_const(const uint32_t* consts, uint32_t index) {
  const uint32_t* p = consts + (size_t)index * 9;
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = p[i];
  HM_DECLARE(r, 1.0);
  return r;
}
HM_HD Fr vt_from_ext(const uint32_t* p) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
  return fe_from_ext<FrParams>(w);
}
HM_HD void vt_to_ext(uint32_t* p, const Fr& a) {
  uint32_t w[8];
  fe_to_ext(w, a);
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = w[i];
}
HM_HD void vt_zero_rows(uint32_t* p, uint32_t rows) {
  for (uint32_t i = 0; i < rows * 8; ++i) p[i] = 0;
}
// sums and differences of elements below 3r, back below 3r
HM_HD Fr vt_add(const Fr& a, const Fr& b) { return fe_reduce_small(fe_norm(fe_add(a, b))); }
HM_HD Fr vt_sub(const Fr& a, const Fr& b) { return fe_reduce_small(fe_norm(fe_sub<4, 29>(a, b))); }
HM_HD Fr vt_neg(const Fr& a) { return vt_sub(fe_zero<FrParams>(), a); }

// a^(r-2), left to right over the constant exponent (r - 2 ends in ...0fffffff: no borrow out of the low limb): 253 squarings and the
// products of its set bits; the bit tests are wave-uniform.  The inverse of zero is zero.
HM_HD Fr vt_inv(const Fr& a) {
  Fr acc = a;                                    // the top bit of the top limb (bit 21)
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    const uint32_t e = i == 0 ? FrParams::MOD[0] - 2u : FrParams::MOD[i];
    const int top = i == 8 ? 20 : 28;
    for (int bit = top; bit >= 0; --bit) {
      acc = fe_sqr(acc);
      if ((e >> bit) & 1) acc = fe_mul(acc, a);
    }
  }
  return acc;
}

// -> false when x^n = 1 or x = 0 (the lane is then flagged; what it computes is defined, and discarded)
HM_HD bool vt_phase_a(const uint32_t* plan, const VtMem& m, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst) {
  const uint32_t* cst = plan + plan[VT_OFF_CONSTS];
  const uint32_t wc = plan[VT_N_VALS], s_l0 = plan[VT_S_L0];
  for (uint32_t j = 0; j < VT_REC; ++j) vt_store(m, wc + j, fe_canonical(vt_from_ext(rec + 8 * (size_t)j)));   // canonical: ge_run reads four of them as constants
  for (uint32_t j = 0; j < plan[VT_N_SCALARS]; ++j) vt_store(m, j, vt_from_ext(evals + 8 * (size_t)j));
  const Fr x = vt_load(m, wc + VT_X), one = fe_one<FrParams>();
  Fr xn = x;
  for (uint32_t i = 0; i < plan[VT_K]; ++i) xn = fe_sqr(xn);
  const Fr xn1 = vt_sub(xn, one);
  const bool ok = !fe_is_zero_mod(xn1) && !fe_is_zero_mod(x);
  const Fr zh = fe_mul(xn1, vt_const(cst, 0));                  // (x^n - 1) / n, the same for every rotation of x
  Fr blind = fe_zero<FrParams>();
  for (uint32_t j = 0; j < plan[VT_N_LAGRANGE]; ++j) {          // l_i(x) = omega^i (x^n - 1) / (n (x - omega^i)): l0, l_last, the blinding rows
    const Fr w = vt_const(cst, plan[VT_C_LAGRANGE] + j);
    const Fr l = fe_mul(fe_mul(w, zh), vt_inv(vt_sub(x, w)));
    if (j < 2) vt_store(m, s_l0 + j, l);
    else blind = vt_add(blind, l);
  }
  vt_store(m, s_l0 + 2, vt_sub(vt_sub(one, vt_load(m, s_l0 + 1)), blind));
  vt_store(m, s_l0 + 3, x);
  for (uint32_t q = 0; q < plan[VT_N_INSTQ]; ++q) {             // sum_i v_i l_i(x omega^rot) over the rows given
    const uint32_t* e = plan + plan[VT_OFF_INST] + 3 * (size_t)q;
    const Fr pt = fe_mul(x, vt_const(cst, e[2]));
    Fr acc = fe_zero<FrParams>();
    for (uint32_t i = 0; i < e[1]; ++i) {
      const Fr w = vt_const(cst, plan[VT_C_ROWS] + i);
      const Fr v = vt_from_ext(inst + 8 * (size_t)(e[0] + i));
      acc = vt_add(acc, fe_mul(fe_mul(v, w), vt_inv(vt_sub(pt, w))));
    }
    vt_store(m, plan[VT_S_INST] + q, fe_mul(acc, zh));
  }
  vt_store(m, wc + VT_XN, xn);
  vt_store(m, wc + VT_XN1_INV, vt_inv(xn1));
  return ok;
}

// num: the numerator, below 3r.  -> false when u hits a point of the first set's complement (z_0 = 0)
HM_HD bool vt_phase_b(const uint32_t* plan, const VtMem& m, const Fr& num, uint32_t* own, uint32_t* shared, uint32_t* h2r, uint32_t* h2l) {
  const uint32_t* cst = plan + plan[VT_OFF_CONSTS];
  const uint32_t wc = plan[VT_N_VALS], wd = vt_ws_diff(plan), wb = vt_ws_basis(plan), n_super = plan[VT_N_SUPER];
  vt_store(m, plan[VT_S_HX], fe_mul(num, vt_load(m, wc + VT_XN1_INV)));
  const Fr x = vt_load(m, wc + VT_X), y2 = vt_load(m, wc + VT_Y2), v = vt_load(m, wc + VT_V), u = vt_load(m, wc + VT_U);
  const Fr rb = vt_load(m, wc + VT_RB), xn = vt_load(m, wc + VT_XN), one = fe_one<FrParams>();
  const Fr x_inv = vt_inv(x);
  Fr zt = one;
  for (uint32_t s = 0; s < n_super; ++s) {
    const Fr d = vt_sub(u, fe_mul(x, vt_const(cst, plan[VT_C_SUPER] + s)));
    vt_store(m, wd + s, d);
    zt = fe_mul(zt, d);
  }
  Fr r_outer = fe_zero<FrParams>(), v_i = one, z0_inv = fe_zero<FrParams>();
  bool ok = true;
  size_t at = plan[VT_OFF_SETS];
  for (uint32_t i = 0; i < plan[VT_N_SETS]; ++i) {
    const uint32_t t = plan[at], mask = plan[at + 1], members = plan[at + 2];
    const uint32_t* sup = plan + at + 3;
    const uint32_t* dinv = sup + t;
    at += 3 + 2 * (size_t)t;
    Fr z = one;
    for (uint32_t s = 0; s < n_super; ++s)
      if (!((mask >> s) & 1u)) z = fe_mul(z, vt_load(m, wd + s));
    if (i == 0) {
      ok = !fe_is_zero_mod(z);
      z0_inv = vt_inv(z);
      z = one;
    } else {
      z = fe_mul(z, z0_inv);
    }
    const Fr outer = fe_mul(v_i, z);
    v_i = fe_mul(v_i, v);
    Fr xs = one;                                                 // x^-(t-1): the points are x omega^r, the constants hold the omega part
    for (uint32_t l = 1; l < t; ++l) xs = fe_mul(xs, x_inv);
    for (uint32_t l = 0; l < t; ++l) {                           // the Lagrange basis of the set's points at u
      Fr b = fe_mul(vt_const(cst, dinv[l]), xs);
      for (uint32_t k = 0; k < t; ++k)
        if (k != l) b = fe_mul(b, vt_load(m, wd + sup[k]));
      vt_store(m, wb + l, b);
    }
    Fr yj = one;
    for (uint32_t j = 0; j < members; ++j) {
      const uint32_t target = plan[at], index = target & VT_T_INDEX;
      const uint32_t* slots = plan + at + 1;
      at += 1 + (size_t)t;
      const Fr coeff = fe_mul(outer, yj);
      yj = fe_mul(yj, y2);
      Fr r_eval = fe_zero<FrParams>();
      for (uint32_t l = 0; l < t; ++l) r_eval = vt_add(r_eval, fe_mul(vt_load(m, wb + l), vt_load(m, slots[l])));
      r_outer = vt_add(r_outer, fe_mul(coeff, r_eval));
      Fr weighted = fe_mul(coeff, rb);
      if (target & VT_T_H) {                                     // [h] = sum_p x^(n p) [h_p]
        for (uint32_t p = 0; p < plan[VT_PIECES]; ++p) {
          vt_to_ext(own + 8 * (size_t)(index + p), weighted);
          weighted = fe_mul(weighted, xn);
        }
      } else if (target & VT_T_SHARED) {
        vt_to_ext(shared + 8 * (size_t)index, weighted);
      } else {
        vt_to_ext(own + 8 * (size_t)index, weighted);
      }
    }
  }
  vt_to_ext(shared + 8 * (size_t)(plan[VT_N_SHARED] - 1), vt_neg(fe_mul(r_outer, rb)));              // the generator
  vt_to_ext(own + 8 * (size_t)(plan[VT_N_OWN] - 1), vt_neg(fe_mul(fe_mul(z0_inv, zt), rb)));         // [h]
  vt_to_ext(h2r, fe_mul(u, rb));
  vt_to_ext(h2l, rb);
  return ok;
}
