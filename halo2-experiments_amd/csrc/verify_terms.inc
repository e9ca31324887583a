// verify_terms.inc -- the per-proof arithmetic of a batch verification on the device, one lane per proof (batch_verifier.py is the
// caller, DESIGN.md section 20): from a proof's evaluations, its instance values and its challenges to r_b x the scalar of every point
// of its opening check.
//
// A PLAN, built once per constraint system on the host (proof_layout.TermsPlan) and checked word by word before every launch
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
// Included inside namespace hm by verify.hip, which holds the kernels and their driver, and by capi_verify.hip for the plans' checks.
// A multi-circuit proof takes a wavefront, one lane per circuit (DESIGN.md section 29): the middle of this file holds its plan, its
// phase a and its numerator term (vtm_*).  Phase b stands last and is written ONCE: vt_set_walk walks the rotation sets for the lane
// of either road (VtSingle / VtmLane, chosen at compile time) and returns the lane's share, vt_finish writes the generator's scalar,
// [h]'s, h2_r and h2_l from the summed shares, vt_zero_lane zeroes what a lane may write; vt_phase_b is walk + finish for one circuit.

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

// nullptr, or why the plan is refused, for everything in front of the sets: the header, the column map, the instance queries and the
// constants -- the words a SHPLONK plan and a GWC plan (vg_plan_problem) share
inline const char* vt_plan_head_problem(const uint32_t* p, size_t n_words, size_t n_columns) {
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
  return nullptr;
}

// nullptr, or why the plan is refused: after this every index the kernel takes from the plan lies inside its array
inline const char* vt_plan_problem(const uint32_t* p, size_t n_words, size_t n_columns) {
  if (const char* why = vt_plan_head_problem(p, n_words, n_columns)) return why;
  const uint64_t words = n_words;
  const uint32_t n_vals = p[VT_N_VALS], n_consts = p[VT_N_CONSTS], n_super = p[VT_N_SUPER];
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
// phase a behind the loads: the record and the evaluations stand in the workspace (the multi-circuit kernel gathers them itself)
HM_HD bool vt_phase_a_rest(const uint32_t* plan, const VtMem& m, const uint32_t* inst);

HM_HD bool vt_phase_a(const uint32_t* plan, const VtMem& m, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst) {
  const uint32_t wc = plan[VT_N_VALS];
  for (uint32_t j = 0; j < VT_REC; ++j) vt_store(m, wc + j, fe_canonical(vt_from_ext(rec + 8 * (size_t)j)));   // canonical: ge_run reads four of them as constants
  for (uint32_t j = 0; j < plan[VT_N_SCALARS]; ++j) vt_store(m, j, vt_from_ext(evals + 8 * (size_t)j));
  return vt_phase_a_rest(plan, m, inst);
}

HM_HD bool vt_phase_a_rest(const uint32_t* plan, const VtMem& m, const uint32_t* inst) {
  const uint32_t* cst = plan + plan[VT_OFF_CONSTS];
  const uint32_t wc = plan[VT_N_VALS], s_l0 = plan[VT_S_L0];
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

// ---- a multi-circuit proof (create_proof_multi): one WAVEFRONT per proof, lane c = circuit c ------------------------------------------
// The multi plan (proof_layout.MultiTermsPlan) wraps the plan of ONE circuit -- the LANE plan, the words above, checked by
// vt_plan_problem as they are -- and says where a lane finds its circuit in the proof:
//   header      VM_* below; VM_N_SCALARS / VM_N_OWN are the PROOF's counts, VM_OWN_TAIL its first own row no circuit owns (random, the
//               h pieces, [h]), VM_EXPRS the E expressions one circuit folds in y
//   segments    VM_N_SEG x (count, base, stride): the lane's evaluation slots in order -- the next `count` slots of lane c are the
//               proof's scalars base + c * stride + i
//   groups      VM_N_GROUPS x (base, count): lane c owns the own rows base + c * count + i (its advice, lookup and permutation points)
//   members     per rotation set of the lane plan, in its order: p, the members that belong to a circuit (they stand first in the
//               set), then (target, stride) per member: circuit c's row is target + c * stride; a member behind the first p is the
//               proof's (a shared point, the h pieces, the random point), stride 0, target as in the lane plan
// Inside a set the members of the PROOF stand circuit 0's first, then circuit 1's, ..., then the proof's own: member j of circuit c has
// y'^(c p + j), member j of the proof's y'^(m p + j - p).  The numerator is upstream's one running value
// N = sum_c y^(E (m - 1 - c)) N_c with N_c the lane's own fold, and sum coeff * r_eval is summed over the lanes likewise: the kernel
// folds both with cross-lane moves (verify.hip), hc_verify_terms_multi with plain loops.  Lane 0 writes what belongs to the proof.
enum : uint32_t {
  VM_CIRCUITS, VM_EXPRS, VM_N_SCALARS, VM_N_OWN, VM_OWN_TAIL, VM_N_SEG, VM_OFF_SEG, VM_N_GROUPS, VM_OFF_GROUPS, VM_OFF_MEMBERS, VM_OFF_LANE,
  VM_LANE_WORDS, VM_HDR
};
constexpr uint32_t VM_MAX_CIRCUITS = 64;                         // the lanes of a gfx950 wavefront, and prover.MAX_CIRCUITS

HM_HD const uint32_t* vtm_lane_plan(const uint32_t* mp) { return mp + mp[VM_OFF_LANE]; }

// nullptr, or why the multi plan is refused: after this every index a lane of ANY circuit takes from it lies inside its array
inline const char* vtm_plan_problem(const uint32_t* p, size_t n_words, size_t n_columns, uint32_t circuits) {
  if (circuits == 0 || circuits > VM_MAX_CIRCUITS) return "verify terms multi: need 1 <= circuits <= 64";
  if (n_words < VM_HDR) return "verify terms multi: the plan is shorter than its header";
  if (p[VM_CIRCUITS] != circuits) return "verify terms multi: the plan was built for another number of circuits";
  const uint64_t words = n_words, last = circuits - 1;
  if (p[VM_OFF_LANE] < VM_HDR || p[VM_OFF_LANE] > words || p[VM_LANE_WORDS] > words - p[VM_OFF_LANE])
    return "verify terms multi: the lane plan lies outside the plan";
  const uint32_t* lp = p + p[VM_OFF_LANE];
  if (const char* why = vt_plan_problem(lp, p[VM_LANE_WORDS], n_columns)) return why;
  if (p[VM_EXPRS] == 0 || p[VM_EXPRS] > (1u << 20)) return "verify terms multi: need 1 .. 2^20 expressions";
  const uint32_t n_scalars = p[VM_N_SCALARS], n_own = p[VM_N_OWN], own_tail = p[VM_OWN_TAIL];
  if (n_scalars == 0 || n_scalars > (1u << 22) || n_own == 0 || n_own > (1u << 22) || own_tail >= n_own)
    return "verify terms multi: output sizes out of range";
  if (p[VM_OFF_SEG] > words || (uint64_t)p[VM_N_SEG] * 3 > words - p[VM_OFF_SEG]) return "verify terms multi: the segments lie outside the plan";
  uint64_t filled = 0;
  for (uint32_t s = 0; s < p[VM_N_SEG]; ++s) {
    const uint32_t* e = p + p[VM_OFF_SEG] + 3 * (size_t)s;
    const uint64_t first = e[1] + last * e[2];                   // the LAST circuit's first scalar
    if (first > n_scalars || e[0] > n_scalars - first) return "verify terms multi: a per-circuit stride leaves the proof's scalars";
    filled += e[0];
  }
  if (filled != lp[VT_N_SCALARS]) return "verify terms multi: the segments do not fill the lane's evaluations";
  if (p[VM_OFF_GROUPS] > words || (uint64_t)p[VM_N_GROUPS] * 2 > words - p[VM_OFF_GROUPS]) return "verify terms multi: the groups lie outside the plan";
  for (uint32_t g = 0; g < p[VM_N_GROUPS]; ++g) {
    const uint32_t* e = p + p[VM_OFF_GROUPS] + 2 * (size_t)g;
    if (e[0] + (uint64_t)circuits * e[1] > own_tail) return "verify terms multi: a per-circuit stride leaves the proof's own rows";
  }
  uint64_t at = lp[VT_OFF_SETS], ext = p[VM_OFF_MEMBERS];
  for (uint32_t i = 0; i < lp[VT_N_SETS]; ++i) {
    const uint32_t t = lp[at], members = lp[at + 2];             // inside the lane plan: vt_plan_problem walked them
    at += 3 + 2ull * t + (uint64_t)members * (1 + t);
    if (ext + 1 + 2ull * members > words) return "verify terms multi: the members lie outside the plan";
    const uint32_t per = p[ext];
    if (per > members) return "verify terms multi: a set with more per-circuit members than members";
    for (uint32_t j = 0; j < members; ++j) {
      const uint32_t target = p[ext + 1 + 2ull * j], stride = p[ext + 2 + 2ull * j], index = target & VT_T_INDEX;
      if (j < per) {
        if ((target & (VT_T_SHARED | VT_T_H)) || index + last * stride >= own_tail)
          return "verify terms multi: a per-circuit stride leaves the proof's own rows";
      } else if (stride != 0 || (target & VT_T_H ? ((target & VT_T_SHARED) || index > n_own || lp[VT_PIECES] > n_own - index)
                                                 : (index >= (target & VT_T_SHARED ? lp[VT_N_SHARED] : n_own)))) {
        return "verify terms multi: a member's target out of range";
      }
    }
    ext += 1 + 2ull * members;
  }
  return nullptr;
}

// a^e for an exponent every lane shares (a plan word): the bit tests are wave-uniform
HM_HD Fr vtm_pow_uniform(const Fr& a, uint32_t e) {
  Fr r = fe_one<FrParams>();
  for (uint32_t bit = 32; bit-- > 0;) {
    if (e >> bit) r = fe_sqr(r);                                 // nothing to square before the top bit
    if ((e >> bit) & 1u) r = fe_mul(r, a);
  }
  return r;
}
// a^e, e < 64, for an exponent of the lane's own: six squarings and six products on every lane, the product kept by a select
HM_HD Fr vtm_pow_lane(const Fr& a, uint32_t e) {
  Fr r = fe_one<FrParams>();
  for (uint32_t bit = 6; bit-- > 0;) {
    r = fe_sqr(r);
    const Fr with = fe_mul(r, a);
    if ((e >> bit) & 1u) r = with;                               // a select: both values exist on every lane
  }
  return r;
}

// phase a of lane c: the proof's record, the lane's evaluations gathered by the segments, then vt_phase_a_rest on its instance values
HM_HD bool vtm_phase_a(const uint32_t* mp, const VtMem& m, uint32_t c, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst) {
  const uint32_t* lp = vtm_lane_plan(mp);
  const uint32_t wc = lp[VT_N_VALS];
  for (uint32_t j = 0; j < VT_REC; ++j) vt_store(m, wc + j, fe_canonical(vt_from_ext(rec + 8 * (size_t)j)));
  uint32_t slot = 0;
  for (uint32_t s = 0; s < mp[VM_N_SEG]; ++s) {
    const uint32_t* e = mp + mp[VM_OFF_SEG] + 3 * (size_t)s;
    const uint32_t* from = evals + 8 * ((size_t)e[1] + (size_t)c * e[2]);
    for (uint32_t i = 0; i < e[0]; ++i) vt_store(m, slot++, vt_from_ext(from + 8 * (size_t)i));
  }
  return vt_phase_a_rest(lp, m, inst);
}

// lane c's term of the numerator: y^(E (m - 1 - c)) N_c
HM_HD Fr vtm_numerator_term(const uint32_t* mp, const VtMem& m, uint32_t c, const Fr& own_fold) {
  const Fr y_e = vtm_pow_uniform(vt_load(m, vtm_lane_plan(mp)[VT_N_VALS] + VT_Y), mp[VM_EXPRS]);
  return fe_mul(own_fold, vtm_pow_lane(y_e, mp[VM_CIRCUITS] - 1 - c));
}

// ---- phase b: ONE walk over the rotation sets for both roads ----------------------------------------------------------------------------
// Who walks: the one lane of a single-circuit proof, or lane c of a multi-circuit proof's wavefront.  The choice is made at compile
// time (if constexpr on Lane::multi), so the single-circuit instantiation holds none of the multi-circuit work.
struct VtSingle {
  static constexpr bool multi = false;
};
struct VtmLane {
  static constexpr bool multi = true;
  const uint32_t* mp;                                            // the multi plan; the `plan` beside it is its lane plan
  uint32_t c;
};

// the rows this lane answers for, zeroed by the lane that may write them later (one lane's stores keep their order): its circuit's
// groups, and -- the single lane, or lane 0 -- what belongs to the proof.  Called before the work and again when the proof fails.
template <class Lane>
HM_HD void vt_zero_lane(const uint32_t* plan, const Lane& lane, uint32_t* own, uint32_t* shared, uint32_t* h2r, uint32_t* h2l) {
  uint32_t first = 0, n_own = plan[VT_N_OWN];
  if constexpr (Lane::multi) {
    const uint32_t* mp = lane.mp;
    if (lane.c < mp[VM_CIRCUITS])
      for (uint32_t g = 0; g < mp[VM_N_GROUPS]; ++g) {
        const uint32_t* e = mp + mp[VM_OFF_GROUPS] + 2 * (size_t)g;
        vt_zero_rows(own + 8 * ((size_t)e[0] + (size_t)lane.c * e[1]), e[1]);
      }
    if (lane.c != 0) return;
    first = mp[VM_OWN_TAIL], n_own = mp[VM_N_OWN];
  }
  vt_zero_rows(own + 8 * (size_t)first, n_own - first);
  vt_zero_rows(shared, plan[VT_N_SHARED]);
  vt_zero_rows(h2r, 1);
  vt_zero_rows(h2l, 1);
}

struct VtmShare {
  Fr r_outer, z0_inv, zt;                                        // the lane's share of sum coeff * r_eval; 1 / z_0 and the vanishing value at u
  bool ok;                                                       // false when u hits a point of the first set's complement (z_0 = 0)
};

// num: the PROOF's numerator, below 3r.  The lane writes r_b x the scalars of its own points: all of them for a single-circuit
// proof; circuit c's for lane c of a multi-circuit proof, and lane 0 those of the proof's as well.
template <class Lane>
HM_HD VtmShare vt_set_walk(const uint32_t* plan, const VtMem& m, const Lane& lane, const Fr& num, uint32_t* own, uint32_t* shared) {
  const uint32_t* cst = plan + plan[VT_OFF_CONSTS];
  const uint32_t wc = plan[VT_N_VALS], wd = vt_ws_diff(plan), wb = vt_ws_basis(plan), n_super = plan[VT_N_SUPER];
  vt_store(m, plan[VT_S_HX], fe_mul(num, vt_load(m, wc + VT_XN1_INV)));
  const Fr x = vt_load(m, wc + VT_X), y2 = vt_load(m, wc + VT_Y2), v = vt_load(m, wc + VT_V), u = vt_load(m, wc + VT_U);
  const Fr rb = vt_load(m, wc + VT_RB), xn = vt_load(m, wc + VT_XN), one = fe_one<FrParams>();
  const Fr x_inv = vt_inv(x);
  VtmShare out;
  out.zt = one;
  for (uint32_t s = 0; s < n_super; ++s) {
    const Fr d = vt_sub(u, fe_mul(x, vt_const(cst, plan[VT_C_SUPER] + s)));
    vt_store(m, wd + s, d);
    out.zt = fe_mul(out.zt, d);
  }
  out.r_outer = fe_zero<FrParams>(), out.z0_inv = fe_zero<FrParams>(), out.ok = true;
  Fr v_i = one;
  size_t at = plan[VT_OFF_SETS];
  const uint32_t* ext = nullptr;                                 // the multi plan's member words of the current set
  if constexpr (Lane::multi) ext = lane.mp + lane.mp[VM_OFF_MEMBERS];
  for (uint32_t i = 0; i < plan[VT_N_SETS]; ++i) {
    const uint32_t t = plan[at], mask = plan[at + 1], members = plan[at + 2];
    const uint32_t* sup = plan + at + 3;
    const uint32_t* dinv = sup + t;
    at += 3 + 2 * (size_t)t;
    Fr z = one;
    for (uint32_t s = 0; s < n_super; ++s)
      if (!((mask >> s) & 1u)) z = fe_mul(z, vt_load(m, wd + s));
    if (i == 0) {
      out.ok = !fe_is_zero_mod(z);
      out.z0_inv = vt_inv(z);
      z = one;
    } else {
      z = fe_mul(z, out.z0_inv);
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
    Fr yj = one, y_tail = one;
    uint32_t per = 0;
    if constexpr (Lane::multi) {
      per = ext[0];
      const Fr y_per = vtm_pow_uniform(y2, per);                 // y'^p: one circuit's step inside this set
      y_tail = vtm_pow_uniform(y_per, lane.mp[VM_CIRCUITS]);     // where the proof's members begin
      yj = vtm_pow_lane(y_per, lane.c);
    }
    for (uint32_t j = 0; j < members; ++j) {
      uint32_t target = plan[at], index = target & VT_T_INDEX;
      const uint32_t* slots = plan + at + 1;
      at += 1 + (size_t)t;
      if constexpr (Lane::multi) {
        target = ext[1 + 2 * (size_t)j], index = (target & VT_T_INDEX) + lane.c * ext[2 + 2 * (size_t)j];
        if (j == per) yj = y_tail;
        if (j >= per && lane.c != 0) continue;                   // the proof's members are lane 0's
      }
      const Fr coeff = fe_mul(outer, yj);
      yj = fe_mul(yj, y2);
      Fr r_eval = fe_zero<FrParams>();
      for (uint32_t l = 0; l < t; ++l) r_eval = vt_add(r_eval, fe_mul(vt_load(m, wb + l), vt_load(m, slots[l])));
      out.r_outer = vt_add(out.r_outer, fe_mul(coeff, r_eval));
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
    if constexpr (Lane::multi) ext += 1 + 2 * (size_t)members;
  }
  return out;
}

// behind the walk (lane 0, behind the fold): r_outer is the sum of every lane's share, n_own the PROOF's own rows
HM_HD void vt_finish(const uint32_t* plan, uint32_t n_own, const VtMem& m, const Fr& r_outer, const VtmShare& mine, uint32_t* own,
                     uint32_t* shared, uint32_t* h2r, uint32_t* h2l) {
  const uint32_t wc = plan[VT_N_VALS];
  const Fr u = vt_load(m, wc + VT_U), rb = vt_load(m, wc + VT_RB);
  vt_to_ext(shared + 8 * (size_t)(plan[VT_N_SHARED] - 1), vt_neg(fe_mul(r_outer, rb)));              // the generator
  vt_to_ext(own + 8 * (size_t)(n_own - 1), vt_neg(fe_mul(fe_mul(mine.z0_inv, mine.zt), rb)));        // [h]
  vt_to_ext(h2r, fe_mul(u, rb));
  vt_to_ext(h2l, rb);
}

// phase b of a single-circuit proof: the walk, then the finish on its own share.  -> the share's ok
HM_HD bool vt_phase_b(const uint32_t* plan, const VtMem& m, const Fr& num, uint32_t* own, uint32_t* shared, uint32_t* h2r, uint32_t* h2l) {
  const VtmShare mine = vt_set_walk(plan, m, VtSingle{}, num, own, shared);
  vt_finish(plan, plan[VT_N_OWN], m, mine.r_outer, mine, own, shared, h2r, h2l);
  return mine.ok;
}


// ---- the GWC multiopen (gwc.py; DESIGN.md section 30): one lane per proof, its own phase b ------------------------------------------------
// A GWC plan (proof_layout.GwcTermsPlan) is a SHPLONK plan up to VT_OFF_SETS: the same header, column map, instance queries and
// constants, so phase a, the numerator's Source and the workspace are the ones above.  VT_N_SUPER = VT_N_SETS = q, the number of
// distinct query points, at most VT_MAX_SUPER.  At VT_OFF_SETS stand the q POINT GROUPS in order of first appearance in the query list:
//   per group    (c, w_row, members): the constant index of omega^rot -- the group's point is z_i = x omega^rot --, the own row of the
//                witness W_i, the number of members
//   per member   (target, slot): the target as in a rotation set (VT_T_SHARED | row of the shared array, VT_T_H | the first h piece's
//                own row, or an own row), the value slot of the member's evaluation at the group's point (VT_S_HX for h)
// The record has EIGHT elements, theta, beta, gamma, y, x, v, u, r_b (what the schedule-driven transcript kernels leave for seven
// challenges, then the caller's weight): the first five stand where the SHPLONK record has them, so the Source's dyn() and phase a's
// rest read the same slots.  The check is e(sum_i u^i W_i, [s]G2) = e(sum_i u^i z_i W_i + sum_i u^i sum_j v^j C_ij - (sum u^i v^j e_ij) G, G2):
// a commitment opened at several points is a member of several groups, so a member's scalar is ADDED to its row (the rows start at
// zero).  No Lagrange basis, and no inversion besides phase a's.
enum : uint32_t { VG_V = 5, VG_U = 6, VG_RB = 7, VG_REC = 8 };

// nullptr, or why the GWC plan is refused: after this every index the kernel takes from the plan lies inside its array
inline const char* vg_plan_problem(const uint32_t* p, size_t n_words, size_t n_columns) {
  if (const char* why = vt_plan_head_problem(p, n_words, n_columns)) return why;
  const uint64_t words = n_words;
  const uint32_t n_vals = p[VT_N_VALS], n_consts = p[VT_N_CONSTS], groups = p[VT_N_SETS];
  if (groups > VT_MAX_SUPER || groups != p[VT_N_SUPER]) return "verify terms gwc: need 1 .. 32 point groups, one per rotation";
  if (groups > p[VT_N_OWN]) return "verify terms gwc: more witness points than own points";
  uint64_t at = p[VT_OFF_SETS];
  for (uint32_t i = 0; i < groups; ++i) {
    if (at + 3 > words) return "verify terms gwc: the groups lie outside the plan";
    const uint32_t members = p[at + 2];
    if (p[at] >= n_consts) return "verify terms gwc: a group's constant out of range";
    if (p[at + 1] >= p[VT_N_OWN]) return "verify terms gwc: a witness row out of range";
    at += 3;
    if (2ull * members > words - at) return "verify terms gwc: the groups lie outside the plan";
    for (uint32_t j = 0; j < members; ++j, at += 2) {
      const uint32_t target = p[at], index = target & VT_T_INDEX;
      if (target & VT_T_H ? ((target & VT_T_SHARED) || index > p[VT_N_OWN] || p[VT_PIECES] > p[VT_N_OWN] - index)
                          : (index >= (target & VT_T_SHARED ? p[VT_N_SHARED] : p[VT_N_OWN])))
        return "verify terms gwc: a member's target out of range";
      if (p[at + 1] >= n_vals) return "verify terms gwc: a member's evaluation slot out of range";
    }
  }
  return nullptr;
}

// phase a of a GWC proof: its eight record elements, then the loads and the rest as above
HM_HD bool vg_phase_a(const uint32_t* plan, const VtMem& m, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst) {
  const uint32_t wc = plan[VT_N_VALS];
  for (uint32_t j = 0; j < VG_REC; ++j) vt_store(m, wc + j, fe_canonical(vt_from_ext(rec + 8 * (size_t)j)));
  for (uint32_t j = 0; j < plan[VT_N_SCALARS]; ++j) vt_store(m, j, vt_from_ext(evals + 8 * (size_t)j));
  return vt_phase_a_rest(plan, m, inst);
}

// every row a GWC lane may write, zeroed: before the work (the members' scalars are added) and again when the proof fails
HM_HD void vg_zero_lane(const uint32_t* plan, uint32_t* own, uint32_t* shared, uint32_t* w_left) {
  vt_zero_rows(own, plan[VT_N_OWN]);
  vt_zero_rows(shared, plan[VT_N_SHARED]);
  vt_zero_rows(w_left, plan[VT_N_SETS]);
}

// row += a, on Montgomery words (a below 3r)
HM_HD void vg_add_row(uint32_t* row, const Fr& a) { vt_to_ext(row, vt_add(vt_from_ext(row), a)); }

// num: the numerator, below 3r.  Writes r_b x the scalars of the proof's own points (W_i with u^i z_i), its row of the shared points
// (the generator last) and r_b u^i to w_left.
HM_HD void vg_phase_b(const uint32_t* plan, const VtMem& m, const Fr& num, uint32_t* own, uint32_t* shared, uint32_t* w_left) {
  const uint32_t* cst = plan + plan[VT_OFF_CONSTS];
  const uint32_t wc = plan[VT_N_VALS];
  vt_store(m, plan[VT_S_HX], fe_mul(num, vt_load(m, wc + VT_XN1_INV)));
  const Fr x = vt_load(m, wc + VT_X), v = vt_load(m, wc + VG_V), u = vt_load(m, wc + VG_U), xn = vt_load(m, wc + VT_XN);
  Fr u_i = vt_load(m, wc + VG_RB);                               // r_b u^i
  Fr e_sum = fe_zero<FrParams>();
  HM_DECLARE(e_sum, 3.0);
  size_t at = plan[VT_OFF_SETS];
  for (uint32_t i = 0; i < plan[VT_N_SETS]; ++i) {
    const uint32_t c = plan[at], w_row = plan[at + 1], members = plan[at + 2];
    at += 3;
    Fr coeff = u_i;                                              // r_b u^i v^j
    for (uint32_t j = 0; j < members; ++j, at += 2) {
      const uint32_t target = plan[at], index = target & VT_T_INDEX;
      e_sum = vt_add(e_sum, fe_mul(coeff, vt_load(m, plan[at + 1])));
      if (target & VT_T_H) {                                     // [h] = sum_p x^(n p) [h_p]
        Fr weighted = coeff;
        for (uint32_t p = 0; p < plan[VT_PIECES]; ++p) {
          vg_add_row(own + 8 * (size_t)(index + p), weighted);
          weighted = fe_mul(weighted, xn);
        }
      } else if (target & VT_T_SHARED) {
        vg_add_row(shared + 8 * (size_t)index, coeff);
      } else {
        vg_add_row(own + 8 * (size_t)index, coeff);
      }
      coeff = fe_mul(coeff, v);
    }
    vt_to_ext(own + 8 * (size_t)w_row, fe_mul(u_i, fe_mul(x, vt_const(cst, c))));   // r_b u^i z_i
    vt_to_ext(w_left + 8 * (size_t)i, u_i);
    u_i = fe_mul(u_i, u);
  }
  vt_to_ext(shared + 8 * (size_t)(plan[VT_N_SHARED] - 1), vt_neg(e_sum));              // the generator
}
