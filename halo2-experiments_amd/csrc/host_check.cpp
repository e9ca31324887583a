// host_check.cpp -- CPU build of the device arithmetic headers (ff29.h, g1.h) with worst-case
// bound tracking (-DHM_BOUNDS).  Not part of the product path: it exists so that the `-m "not gpu"`
// tests can (a) compare the exact code the kernels run with the oracle and (b) prove, by running
// every formula once with its inputs declared at the class bounds, that no 64-bit column sum,
// limb or lazy value can overflow for ANY input (the tracked bounds are data-independent).
// It also holds the host replay of the GraphEvaluator (hc_graph_replay): graph.hip's lowering, shared through graph_lower.h,
// and a restatement of its kernel's interpreter loop on these primitives.
//
// Build: g++ -O2 -std=c++17 -DHM_BOUNDS -shared -fPIC -o libhm_hostcheck.so host_check.cpp
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "fq_inverse.h"
#include "g1.h"
#include "g1_mul.h"
#include "graph_lower.h"
#include "host_fr.h"
#include "mock_check.h"   // the witness checker's key search, value key and record packing (its kernels: mock.hip)

namespace hm {
#include "g1_codec.inc"   // the per-point SRS codec formulas (the kernels: g1_codec.hip)
#include "verify_read.inc"   // the batch verifier's per-slot read and its column sum (verify.hip)
#include "verify_terms.inc"  // ... and the two phases of its per-proof terms around the interpreter's run (verify.hip)
#include "verify_sums.inc"   // ... and the lane, fold and finish functions of its per-proof sums (verify.hip)
#include "ledger.inc"     // the lane function of the ledger openings' pairing operands (ledger.hip)
#include "poseidon.inc"   // the per-hash Poseidon / Merkle node functions (poseidon.hip)
#include "range.inc"      // the range-check witness's lane function (range.hip)
#include "sorted.inc"     // the sorted-column witness's lane function and the argsort's record order (sorted.hip)
#include "accumulator.inc" // the accumulator witness's row function (accumulator.hip)
#include "logup.inc"      // the logUp argument's key, count and addition functions (logup.hip)
#include "keygen.inc"     // the permutation assembly's key packing and link rule (keygen.hip)
#include "shplonk.inc"    // the SHPLONK set quotient's plan, coefficients and row formula (polyops.hip)
#include "pairing.inc"    // the pairing's tower, Miller lane and final exponentiation (pairing.hip)
#include "transcript.inc" // Blake2b-512, its streaming absorber and the transcript lane of a proof (verify.hip)
#include "keccak.inc"     // Keccak-256, the EVM encoding's read and the transcript lane of such a proof (verify.hip)
#include "msm_plan.inc"   // the MSM's window choice, launch plans and workspace layouts (msm.hip, msm_small.hip)
#include "ntt_plan.inc"   // the NTT's call check, launch plan and twiddle table set (ntt.hip)
}

using namespace hm;

namespace {

template <class F>
Fe<F> load_ext(const uint64_t* p) {
  uint32_t w[8];
  std::memcpy(w, p, 32);
  return fe_from_ext<F>(w);
}
template <class F>
void store_ext(uint64_t* p, const Fe<F>& a) {
  uint32_t w[8];
  fe_to_ext(w, a);
  std::memcpy(p, w, 32);
}

template <class F>
void force_bounds(Fe<F>& a, double vb) {  // declare the class maximum regardless of the actual value
  a.vb = vb;
  a.lb = MASK29;
  a.tb = top_bound_from_value<F>(vb);
}

G1Jac load_jac(const uint64_t* p, int inf) {
  G1Jac r;
  r.x = load_ext<FqParams>(p);
  r.y = load_ext<FqParams>(p + 4);
  r.z = load_ext<FqParams>(p + 8);
  r.inf = inf != 0;
  return r;
}
void store_jac(uint64_t* p, int* inf, const G1Jac& r) {
  if (r.inf) {
    std::memset(p, 0, 96);
    *inf = 1;
    return;
  }
  store_ext(p, r.x);
  store_ext(p + 4, r.y);
  store_ext(p + 8, r.z);
  *inf = 0;
}
void at_class_max(G1Jac& p) {
  force_bounds(p.x, HM_G1_XB);
  force_bounds(p.y, HM_G1_YB);
  force_bounds(p.z, HM_G1_ZB);
}

template <class F>
void field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    Fe<F> x = load_ext<F>(a + 4 * i), y = load_ext<F>(b + 4 * i), r;
    switch (op) {
      case 0: r = fe_mul(x, y); break;
      case 1: r = fe_sqr(x); break;
      case 2: r = fe_norm(fe_add(x, y)); break;
      case 3: r = fe_norm(fe_sub<3, 29>(x, y)); break;
      case 4: {  // lazy chain: ((x + y) * (x - y + 3p)) + x*x, exercises unnormalised operands
        Fe<F> s = fe_add(x, y), d = fe_sub<3, 29>(x, y);
        r = fe_norm(fe_add(fe_mul(s, fe_norm(d)), fe_sqr(x)));
        break;
      }
      case 5: {  // x + 40*y accumulated lazily (value up to ~82 MOD), then the cheap reduction
        Fe<F> acc = x;
        for (int k = 0; k < 40; ++k) acc = fe_norm(fe_add(acc, y));
        r = fe_reduce_small(acc);
        break;
      }
      default: r = x;
    }
    store_ext(o + 4 * i, r);
  }
}

// ---- the GraphEvaluator on the host (graph.hip) ----
typedef Fe<FrParams> GFr;
GFr gr_reduce(const GFr& lazy) { return fe_reduce_small(fe_norm(lazy)); }                 // graph.hip: ge_reduce
GFr gr_from_ext(const uint32_t* p) {                                                      // graph.hip: ge_from_ext
  uint32_t w[8];
  std::memcpy(w, p, 32);
  return fe_mul(fe_unpack<FrParams>(w), fe_const<FrParams>(FrParams::EXT2INT));
}
GFr gr_from_internal(const uint32_t* p) {                                                 // graph.hip: ge_from_internal
  uint32_t w[8];
  std::memcpy(w, p, 32);
  GFr r = fe_unpack<FrParams>(w);
  HM_DECLARE(r, GE_COLUMN_BOUND);
  return r;
}
const char* g_graph_error = "";

// One row of the LOWERED program, as ge_run (graph_interp.h) runs it for a lane: THIS LOOP RESTATES THAT SWITCH, primitive for
// primitive and in its order.  fetch(src): ge_fetch;  slots: the lane's scratch;  tracked_bound[k]: the largest bound seen for
// calculation k's result.  -> the program's value, not yet reduced.
template <class Fetch>
GFr gr_run(const GraphLowered& low, std::vector<GFr>& slots, Fetch&& fetch, double* tracked_bound) {
  const size_t n = low.calcs.size();
  GFr prev = fe_zero<FrParams>();
  HM_DECLARE(prev, 3.0);
  for (size_t k = 0; k < n; ++k) {
    const GraphCalc cc = low.calcs[k];
    const uint32_t op = cc.op & 0xffu;
    auto src = [&](uint32_t word, uint32_t flag) -> GFr { return (cc.op & flag) ? prev : fetch(word); };
    const GFr a = src(cc.a, GF_A_PREV);
    GFr out;
    const bool lazy = (cc.op & GF_NO_REDUCE) != 0, wide = (cc.op & GF_SUB_WIDE) != 0;
    auto settle = [&](const GFr& t) -> GFr { return lazy ? fe_norm(t) : gr_reduce(t); };
    switch (op) {
      case GOP_ADD:
        out = settle(fe_add(a, src(cc.b, GF_B_PREV)));
        break;
      case GOP_SUB: {
        const GFr b = src(cc.b, GF_B_PREV);
        out = wide ? gr_reduce(fe_sub<20, 29>(a, b)) : settle(fe_sub<4, 29>(a, b));
        break;
      }
      case GOP_MUL:
        out = fe_mul(a, src(cc.b, GF_B_PREV));
        break;
      case GOP_SQUARE:
        out = fe_sqr(a);
        break;
      case GOP_DOUBLE:
        out = settle(fe_dbl(a));
        break;
      case GOP_NEGATE:
        out = wide ? gr_reduce(fe_sub<20, 29>(fe_zero<FrParams>(), a)) : settle(fe_sub<4, 29>(fe_zero<FrParams>(), a));
        break;
      case GOP_MULADD: {
        const GFr b = src(cc.b, GF_B_PREV);
        const GFr c = src(cc.c, GF_C_PREV);
        out = settle(fe_add(fe_mul(a, b), c));
        break;
      }
      default:
        out = a;
        break;
    }
    if (!(cc.op & GF_NO_STORE)) slots[cc.target] = out;
    if (out.vb > tracked_bound[k]) tracked_bound[k] = out.vb;
    prev = out;
  }
  GFr res = fe_zero<FrParams>();
  if (low.result_prev)
    res = prev;
  else if (n != 0 || gsrc_kind(low.result_src) != GSRC_INTER)
    res = fetch(low.result_src);
  return res;
}

}  // namespace

extern "C" {

// field: 0 = Fq, 1 = Fr.  op: 0 mul, 1 sqr, 2 add, 3 sub, 4 lazy chain.  external Montgomery in/out
void hc_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) {
  if (field == 0) field_op<FqParams>(op, a, b, o, n);
  else field_op<FrParams>(op, a, b, o, n);
}

// unpack/pack round trip and canonicalisation of raw (possibly non-canonical) 256-bit words
void hc_fr_reduce_raw(const uint64_t* a, uint64_t* o, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8];
    std::memcpy(w, a + 4 * i, 32);
    Fe<FrParams> x = fe_unpack<FrParams>(w);
    // x * 2^261 * 2^-261 = x mod r, canonical
    Fe<FrParams> y = fe_canonical(fe_mul(x, fe_const<FrParams>(FrParams::ONE)));
    fe_pack(w, y);
    std::memcpy(o + 4 * i, w, 32);
  }
}

void hc_g1_madd(const uint64_t* pj, int pinf, const uint64_t* q_aff, int neg, uint64_t* out, int* out_inf) {
  G1Jac p = load_jac(pj, pinf);
  G1Aff q;
  q.x = load_ext<FqParams>(q_aff);
  q.y = load_ext<FqParams>(q_aff + 4);
  store_jac(out, out_inf, g1_madd(p, q, neg != 0));
}
void hc_g1_add(const uint64_t* pj, int pinf, const uint64_t* qj, int qinf, uint64_t* out, int* out_inf) {
  store_jac(out, out_inf, g1_add(load_jac(pj, pinf), load_jac(qj, qinf)));
}
void hc_g1_double(const uint64_t* pj, int pinf, uint64_t* out, int* out_inf) {
  store_jac(out, out_inf, g1_double(load_jac(pj, pinf)));
}
// k chained madds of the same affine point followed by doublings: stresses class closure on data
void hc_g1_chain(const uint64_t* q_aff, int k, int dbl, uint64_t* out, int* out_inf) {
  G1Aff q;
  q.x = load_ext<FqParams>(q_aff);
  q.y = load_ext<FqParams>(q_aff + 4);
  G1Jac acc = g1_identity();
  for (int i = 0; i < k; ++i) acc = g1_madd(acc, q);
  for (int i = 0; i < dbl; ++i) acc = g1_double(acc);
  store_jac(out, out_inf, acc);
}

// the bucket accumulator's XYZZ chain: k mixed additions of q (alternating sign pattern given by the
// bits of `signs`), optionally starting from a doubling-triggering repeat, converted to Jacobian
void hc_g1x_chain(const uint64_t* q_affs, int k, uint64_t signs, uint64_t* out, int* out_inf) {
  G1Xyzz acc = g1x_identity();
  for (int i = 0; i < k; ++i) {
    G1Aff q;
    q.x = load_ext<FqParams>(q_affs + 8 * i);
    q.y = load_ext<FqParams>(q_affs + 8 * i + 4);
    acc = g1x_madd(acc, q, ((signs >> (i & 63)) & 1) != 0);
  }
  store_jac(out, out_inf, g1x_to_jac(acc));
}

// XYZZ class closure: madd with the accumulator DECLARED at its class maxima must land inside the
// class again, and its conversion to Jacobian inside the Jacobian class.
int hc_xyzz_bounds_closure(const uint64_t* pj, const uint64_t* q_aff, double* report) {
  G1Jac pjac = load_jac(pj, 0);
  G1Xyzz p = g1x_from_jac(pjac);
  force_bounds(p.x, HM_XYZZ_XB);
  force_bounds(p.y, HM_XYZZ_YB);
  force_bounds(p.zz, 2.0);
  force_bounds(p.zzz, 2.0);
  G1Aff q;
  q.x = load_ext<FqParams>(q_aff);
  q.y = load_ext<FqParams>(q_aff + 4);
  force_bounds(q.x, 2.0);
  force_bounds(q.y, 2.0);
  G1Xyzz r = p;
  if (!g1x_madd_fast(r, q, true)) return 0;
  {
    // the lockstep form of the hot kernel: every product's precondition is checked again inside it; the same limbs and
    // bounds within the class must come out
    G1Xyzz rl = p;
    if (!g1x_madd_fast<true>(rl, q, true)) return 0;
    for (int i = 0; i < 9; ++i)
      if (rl.x.l[i] != r.x.l[i] || rl.y.l[i] != r.y.l[i] || rl.zz.l[i] != r.zz.l[i] || rl.zzz.l[i] != r.zzz.l[i]) return 0;
    if (rl.x.vb > HM_XYZZ_XB || rl.y.vb > HM_XYZZ_YB || rl.zz.vb > 2.0 || rl.zzz.vb > 2.0) return 0;
  }
  const G1Jac j = g1x_to_jac(p);
  report[0] = r.x.vb; report[1] = r.y.vb; report[2] = r.zz.vb; report[3] = r.zzz.vb;
  report[4] = j.x.vb; report[5] = j.y.vb; report[6] = j.z.vb;
  int ok = 1;
  if (r.x.vb > HM_XYZZ_XB || r.y.vb > HM_XYZZ_YB || r.zz.vb > 2.0 || r.zzz.vb > 2.0) ok = 0;
  if (j.x.vb > HM_G1_XB || j.y.vb > HM_G1_YB || j.z.vb > HM_G1_ZB) ok = 0;
  return ok;
}

// Run every curve formula with inputs DECLARED at the class maxima; any precondition violation
// aborts.  Writes the resulting output bounds (x.vb, y.vb, z.vb per formula) for the report.
int hc_bounds_closure(const uint64_t* pj, const uint64_t* qj, const uint64_t* q_aff, double* report) {
  G1Jac p = load_jac(pj, 0), q2 = load_jac(qj, 0);
  at_class_max(p);
  at_class_max(q2);
  G1Aff q;
  q.x = load_ext<FqParams>(q_aff);
  q.y = load_ext<FqParams>(q_aff + 4);
  force_bounds(q.x, 2.0);
  force_bounds(q.y, 2.0);
  G1Jac r[3] = {g1_madd_nz(p, q, true), g1_add_nz(p, q2), g1_double_nz(p)};
  int ok = 1;
  for (int i = 0; i < 3; ++i) {
    report[3 * i + 0] = r[i].x.vb;
    report[3 * i + 1] = r[i].y.vb;
    report[3 * i + 2] = r[i].z.vb;
    if (r[i].x.vb > HM_G1_XB || r[i].y.vb > HM_G1_YB || r[i].z.vb > HM_G1_ZB) ok = 0;
    if (r[i].x.lb > MASK29 || r[i].y.lb > MASK29 || r[i].z.lb > MASK29) ok = 0;
  }
  return ok;
}

// The Fr vector formulas of ntt.hip / poly.hip / polyops.hip, each run once with its inputs DECLARED at the class
// maxima the kernels rely on (raw 256-bit words: value < 2^256; products: < 2r; reduced sums: < 3r).  Any
// precondition violation aborts; returns 1 when every result is inside the class its consumer expects.
// The GraphEvaluator's lazy classes (graph.hip: GE_CAP = 16, GE_COLUMN_BOUND = 6): every stored intermediate is a
// normalised element of value < 16 r.  Run every operation the interpreter has on operands DECLARED at the class
// maxima (the bound tracking asserts each primitive's precondition) and check the outputs are back inside the class.
int hc_graph_bounds_closure(const uint64_t* a_ext, double* report) {
  typedef Fe<FrParams> F;
  F x = load_ext<FrParams>(a_ext);
  const double CAP = 16.0;
  int ok = 1, r = 0;
  F c16 = x, c16b = x, c3 = x, col = x;
  force_bounds(c16, CAP);
  force_bounds(c16b, CAP);
  force_bounds(c3, 3.0);
  force_bounds(col, 6.0);
  // products of two class-maximum operands (and of column words) come out below 3r
  F m = fe_mul(c16, c16b);
  report[r++] = m.vb;
  ok &= m.vb <= 3.0;
  F q = fe_sqr(c16);
  ok &= q.vb <= 3.0;
  ok &= fe_mul(col, c16).vb <= 3.0;
  // lazy sum at the cap: 8 + 8 -> norm only; a sum past the cap is reduced (16 + 16)
  F h8 = x;
  force_bounds(h8, 8.0);
  F s16 = fe_norm(fe_add(h8, h8));
  report[r++] = s16.vb;
  ok &= s16.vb <= CAP;
  F red = fe_reduce_small(fe_norm(fe_add(c16, c16b)));
  ok &= red.vb <= 3.0;
  F dbl = fe_reduce_small(fe_norm(fe_dbl(c16)));
  ok &= dbl.vb <= 3.0;
  // narrow subtraction (subtrahend < 3r): lazy while minuend + 4 <= cap, reduced above
  F d12 = x;
  force_bounds(d12, 12.0);
  F sub_lazy = fe_norm(fe_sub<4, 29>(d12, c3));
  report[r++] = sub_lazy.vb;
  ok &= sub_lazy.vb <= CAP;
  ok &= fe_reduce_small(fe_norm(fe_sub<4, 29>(c16, c3))).vb <= 3.0;
  // wide subtraction (subtrahend up to the cap), always reduced; negation likewise
  F sub_wide = fe_reduce_small(fe_norm(fe_sub<20, 29>(c16, c16b)));
  report[r++] = sub_wide.vb;
  ok &= sub_wide.vb <= 3.0;
  ok &= fe_reduce_small(fe_norm(fe_sub<20, 29>(fe_zero<FrParams>(), c16))).vb <= 3.0;
  ok &= fe_norm(fe_sub<4, 29>(fe_zero<FrParams>(), c3)).vb <= CAP;
  // Horner step a * b + c: lazy while 3 + c <= cap
  F d13 = x;
  force_bounds(d13, 13.0);
  F ma = fe_norm(fe_add(fe_mul(c16, c16b), d13));
  report[r++] = ma.vb;
  ok &= ma.vb <= CAP;
  ok &= fe_reduce_small(fe_norm(fe_add(fe_mul(c16, c16b), c16))).vb <= 3.0;
  // the result leaves through a reduction, the conversion product and the canonical form
  (void)fe_canonical(fe_mul(fe_reduce_small(fe_norm(c16)), fe_const<FrParams>(FrParams::INT2EXT)));
  return ok;
}

// The GraphEvaluator without a GPU: validate and lower a program exactly as hm_graph_create / graph_run do (graph_lower.h is the
// code they run), then interpret the LOWERED program row by row as graph_evaluate_kernel does (gr_run above restates ge_run's switch);
// tests/test_graph_programs_gpu.py holds the two to the same words.
// Column loads, constants and PreviousValue enter at the class maxima the kernel declares; a value in a slot keeps the bound the
// tracker gave it (the kernel re-declares it at GE_CAP, which the caller checks against the static bound instead), and the slots keep
// their contents from row to row, as a lane's slots do in the grid-stride loop.
//   calcs5 ... n_intermediates: as hm_graph_create;  dyn_ext: the per-call constants;  columns[i]: column_rows[i] x 8 words;
//   values: (segments << log_segment) x 8 words, PreviousValue in, the program's value out;  flags: HM_GRAPH_COLUMNS_INTERNAL = 1.
//   lowered5 / static_bound / tracked_bound: room for n_calc calculations -- the lowered program, the lowering's static bound of each
//   result and the largest bound the tracker saw for it;  info: {lowered calculations, slots, result_src, result_prev, Stores of
//   constants removed, Stores of columns removed}.
// -> 0; -1: the program is refused (hc_graph_last_error); -2: a column read past column_rows.  A violated precondition aborts.
int hc_graph_replay(const uint32_t* calcs5, size_t n_calc, const uint64_t* constants_ext, size_t n_const_static, const uint64_t* dyn_ext,
                    size_t n_dynamic, const int32_t* rotations, size_t n_rot, const uint32_t* const* columns, const uint64_t* column_rows,
                    size_t n_columns, uint32_t n_intermediates, uint32_t log_segment, uint32_t segments, uint32_t flags, uint32_t* values,
                    uint32_t* lowered5, double* static_bound, double* tracked_bound, uint32_t* info) {
  g_graph_error = "";
  if (const char* why = graph_validate(calcs5, n_calc, n_const_static, n_dynamic, n_rot, n_columns, n_intermediates)) {
    g_graph_error = why;
    return -1;
  }
  if (flags & ~1u) { g_graph_error = "graph: unknown flag"; return -1; }
  if (log_segment > 30) { g_graph_error = "graph: log_size > 30"; return -1; }
  if (segments == 0 || ((uint64_t)segments << log_segment) > (1ull << 32)) { g_graph_error = "graph: segments must be >= 1 and rows <= 2^32"; return -1; }
  const bool internal_cols = (flags & 1u) != 0;
  GraphLowered low;
  graph_lower_host(calcs5, n_calc, n_intermediates, internal_cols, low);
  const size_t n = low.calcs.size();
  for (size_t k = 0; k < n; ++k) {
    const GraphCalc& c = low.calcs[k];
    const uint32_t w[5] = {c.op, c.a, c.b, c.c, c.target};
    std::memcpy(lowered5 + 5 * k, w, 20);
    static_bound[k] = low.bound[k];
    tracked_bound[k] = 0.0;
  }
  info[0] = (uint32_t)n, info[1] = low.n_slots, info[2] = low.result_src, info[3] = low.result_prev;
  info[4] = low.stores_of_constants_removed, info[5] = low.stores_of_columns_removed;
  // constants -> internal form, as graph_create and graph_run convert them
  std::vector<uint32_t> consts((n_const_static + n_dynamic + 1) * 9, 0);
  for (size_t i = 0; i < n_const_static; ++i) host::fr_to_internal9(host::fr_load(constants_ext + 4 * i), &consts[9 * i]);
  for (size_t i = 0; i < n_dynamic; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), &consts[9 * (n_const_static + i)]);
  // a slot that was never written holds SOMETHING on the device: here a recognisable element inside the class
  GFr stale;
  for (int i = 0; i < 9; ++i) stale.l[i] = 0x5a5a5a5u;
  stale.l[8] = 0x5a5u;
  HM_DECLARE(stale, GE_CAP);
  std::vector<GFr> slots(low.n_slots, stale);
  const uint64_t size = (uint64_t)segments << log_segment, mask = (1ull << log_segment) - 1;
  int rc = 0;
  for (uint64_t idx = 0; idx < size && rc == 0; ++idx) {
    uint32_t* vrow = values + idx * 8;
    auto fetch = [&](uint32_t src) -> GFr {                     // graph.hip: ge_fetch
      const uint32_t kind = gsrc_kind(src), index = gsrc_index(src);
      GFr r;
      if (kind == GSRC_INTER) {
        r = slots[index];
      } else if (kind == GSRC_CONST) {
        for (int i = 0; i < 9; ++i) r.l[i] = consts[(size_t)index * 9 + i];
        HM_DECLARE(r, 1.0);
      } else if (kind == GSRC_COLUMN) {
        uint64_t row = (idx & ~mask) | ((idx + (uint64_t)(int64_t)rotations[gsrc_rot(src)]) & mask);
        const uint32_t lr = gsrc_log_rows(src);
        if (lr != 0) row &= (1ull << lr) - 1ull;
        if (row >= column_rows[gsrc_column(src)]) {
          rc = -2;
          return fe_zero<FrParams>();
        }
        const uint32_t* cell = columns[gsrc_column(src)] + row * 8;
        r = internal_cols ? gr_from_internal(cell) : gr_from_ext(cell);
      } else {
        r = gr_from_ext(vrow);
      }
      return r;
    };
    const GFr res = gr_run(low, slots, fetch, tracked_bound);
    uint32_t w[8];
    fe_to_ext(w, gr_reduce(res));
    std::memcpy(vrow, w, 32);
  }
  return rc;
}
const char* hc_graph_last_error() { return g_graph_error; }

// graph_linear_shape (graph_lower.h) on a validated program: what hm_graph_evaluate_circuits_dev admits.  -> 0 and out = {factor
// source word, Horner steps}; -1: refused (hc_graph_last_error).
int hc_graph_linear_shape(const uint32_t* calcs5, size_t n_calc, size_t n_const_static, size_t n_dynamic, size_t n_rot, size_t n_columns,
                          uint32_t n_intermediates, uint32_t* out) {
  g_graph_error = "";
  const char* why = graph_validate(calcs5, n_calc, n_const_static, n_dynamic, n_rot, n_columns, n_intermediates);
  if (!why) why = graph_linear_shape(calcs5, n_calc, n_intermediates, &out[0], &out[1]);
  if (why) g_graph_error = why;
  return why ? -1 : 0;
}

// graph_circuits_kernel (graph.hip) without a GPU: per row, every circuit's program with PreviousValue = 0 (gr_run), the partial
// reduced as it is before it goes to LDS and RE-DECLARED at the class the kernel declares when it reads it back (< 3r), then the
// fold acc = ge_reduce(acc * f^T + partial) from the entry value, in the kernel's order.  Arguments as hc_graph_replay, and:
// circuits;  column_strides[i]: u32 words from circuit c's column i to circuit c + 1's (0: shared);  column_rows[i]: the rows ONE
// circuit's column holds.  fold_bound: {largest partial as reduced, largest accumulator entering the product, largest sum before
// its reduction, largest accumulator stored}.  -> 0; -1 refused; -2 a column read past column_rows.
int hc_graph_circuits_replay(const uint32_t* calcs5, size_t n_calc, const uint64_t* constants_ext, size_t n_const_static, const uint64_t* dyn_ext,
                             size_t n_dynamic, const int32_t* rotations, size_t n_rot, const uint32_t* const* columns,
                             const uint64_t* column_strides, const uint64_t* column_rows, size_t n_columns, size_t circuits,
                             uint32_t n_intermediates, uint32_t log_segment, uint32_t segments, uint32_t flags, uint32_t* values,
                             double* tracked_bound, double* fold_bound) {
  g_graph_error = "";
  const char* why = graph_validate(calcs5, n_calc, n_const_static, n_dynamic, n_rot, n_columns, n_intermediates);
  uint32_t factor_src = 0, steps = 0;
  if (!why) why = graph_linear_shape(calcs5, n_calc, n_intermediates, &factor_src, &steps);
  if (!why && (flags & ~1u)) why = "graph: unknown flag";
  if (!why && log_segment > 30) why = "graph: log_size > 30";
  if (!why && (segments == 0 || ((uint64_t)segments << log_segment) > (1ull << 32))) why = "graph: segments must be >= 1 and rows <= 2^32";
  if (!why && (circuits == 0 || circuits > (1ull << 32) / ((uint64_t)segments << log_segment))) why = "graph: circuits * rows > 2^32";
  if (why) {
    g_graph_error = why;
    return -1;
  }
  const bool internal_cols = (flags & 1u) != 0;
  GraphLowered low;
  graph_lower_host(calcs5, n_calc, n_intermediates, internal_cols, low);
  for (size_t k = 0; k < low.calcs.size(); ++k) tracked_bound[k] = 0.0;
  std::vector<uint32_t> consts((n_const_static + n_dynamic + 1) * 9, 0);
  for (size_t i = 0; i < n_const_static; ++i) host::fr_to_internal9(host::fr_load(constants_ext + 4 * i), &consts[9 * i]);
  for (size_t i = 0; i < n_dynamic; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), &consts[9 * (n_const_static + i)]);
  const uint32_t fi = gsrc_index(factor_src);
  const host::Fr4 f = host::fr_load(fi < n_const_static ? constants_ext + 4 * (size_t)fi : dyn_ext + 4 * (size_t)(fi - n_const_static));
  host::Fr4 f_pow = f;
  for (uint32_t i = 1; i < steps; ++i) f_pow = host::fr_mul(f_pow, f);
  GFr fold;
  host::fr_to_internal9(f_pow, fold.l);
  HM_DECLARE(fold, 1.0);
  GFr stale;
  for (int i = 0; i < 9; ++i) stale.l[i] = 0x5a5a5a5u;
  stale.l[8] = 0x5a5u;
  HM_DECLARE(stale, GE_CAP);
  std::vector<GFr> slots(low.n_slots, stale);
  const uint64_t size = (uint64_t)segments << log_segment, mask = (1ull << log_segment) - 1;
  for (int i = 0; i < 4; ++i) fold_bound[i] = 0.0;
  int rc = 0;
  for (uint64_t idx = 0; idx < size && rc == 0; ++idx) {
    uint32_t* vrow = values + idx * 8;
    GFr acc = gr_from_ext(vrow);
    for (size_t circuit = 0; circuit < circuits && rc == 0; ++circuit) {
      auto fetch = [&](uint32_t src) -> GFr {                     // graph.hip: ge_fetch over CircuitSource
        const uint32_t kind = gsrc_kind(src), index = gsrc_index(src);
        GFr r;
        if (kind == GSRC_INTER) {
          r = slots[index];
        } else if (kind == GSRC_CONST) {
          for (int i = 0; i < 9; ++i) r.l[i] = consts[(size_t)index * 9 + i];
          HM_DECLARE(r, 1.0);
        } else if (kind == GSRC_COLUMN) {
          uint64_t row = (idx & ~mask) | ((idx + (uint64_t)(int64_t)rotations[gsrc_rot(src)]) & mask);
          const uint32_t lr = gsrc_log_rows(src), col = gsrc_column(src);
          if (lr != 0) row &= (1ull << lr) - 1ull;
          if (row >= column_rows[col]) {
            rc = -2;
            return fe_zero<FrParams>();
          }
          const uint32_t* cell = columns[col] + column_strides[col] * circuit + row * 8;
          r = internal_cols ? gr_from_internal(cell) : gr_from_ext(cell);
        } else {
          r = fe_zero<FrParams>();                                // CircuitSource::previous
        }
        return r;
      };
      GFr part = gr_reduce(gr_run(low, slots, fetch, tracked_bound));
      if (part.vb > fold_bound[0]) fold_bound[0] = part.vb;
      HM_DECLARE(part, 3.0);                                      // as read back from LDS
      if (acc.vb > fold_bound[1]) fold_bound[1] = acc.vb;
      const GFr sum = fe_add(fe_mul(acc, fold), part);
      if (sum.vb > fold_bound[2]) fold_bound[2] = sum.vb;
      acc = gr_reduce(sum);
    }
    if (acc.vb > fold_bound[3]) fold_bound[3] = acc.vb;
    uint32_t w[8];
    fe_to_ext(w, acc);
    std::memcpy(vrow, w, 32);
  }
  return rc;
}

int hc_fr_vector_bounds_closure(const uint64_t* a_ext, const uint64_t* b_ext, double* report) {
  typedef Fe<FrParams> F;
  uint32_t wa[8], wb[8];
  std::memcpy(wa, a_ext, 32);
  std::memcpy(wb, b_ext, 32);
  F raw = fe_unpack<FrParams>(wa);                 // declared: any 256-bit word pattern
  raw.l[8] = (1u << 24) - 1;                       // and take the largest one for the run itself
  for (int i = 0; i < 8; ++i) raw.l[i] = MASK29;
  F z = load_ext<FrParams>(b_ext);                 // a product output
  force_bounds(z, 2.0);
  F k32 = fe_const<FrParams>(FrParams::EXT2INT);   // any canonical constant
  int ok = 1, r = 0;
  // 1. Horner step of eval_polynomial / kate_division: acc <- acc * z + raw, iterated at its fixed point
  F acc = fe_add(fe_mul(raw, z), raw);
  for (int k = 0; k < 4; ++k) acc = fe_add(fe_mul(acc, z), raw);
  report[r++] = acc.vb;
  F s = fe_reduce_small(fe_norm(acc));
  ok &= s.vb <= 3.0;
  // 2. scan step with a uniform multiplier: v <- reduce(v + w * y), v, w < 3r, y < 2r
  F v = s, w = s;
  force_bounds(v, 3.0);
  force_bounds(w, 3.0);
  F t = fe_reduce_small(fe_norm(fe_add(v, fe_mul(w, z))));
  report[r++] = t.vb;
  ok &= t.vb <= 3.0;
  // 3. chunk entry of kate_division: product + stored inclusive value, then the replay step and its canonical store
  F T = fe_add(fe_mul(v, z), w);
  F cur = fe_reduce_small(fe_norm(T));
  cur = fe_reduce_small(fe_norm(fe_add(fe_mul(cur, z), raw)));
  report[r++] = cur.vb;
  (void)fe_canonical(cur);
  // 4. products: factor = raw * K32, running product, scan product, conversion out
  F f = fe_mul(raw, k32);
  F p = fe_mul(z, f);
  p = fe_mul(p, p);
  report[r++] = p.vb;
  ok &= p.vb <= 2.0;
  (void)fe_canonical(p);
  (void)fe_canonical(fe_mul(p, fe_const<FrParams>(FrParams::INT2EXT)));
  F start = raw;                                    // the start value enters as raw words
  (void)fe_mul(p, start);
  // 5. linear combination: four product terms on a value < 3r between reductions
  F lc = v;
  for (int k = 0; k < 4; ++k) lc = fe_add(lc, fe_mul(raw, z));
  lc = fe_reduce_small(fe_norm(lc));
  report[r++] = lc.vb;
  ok &= lc.vb <= 3.0;
  // 6. NTT butterflies: stage 0 on raw inputs, a later trivial-twiddle stage on lazy outputs, a general stage
  F x0 = fe_add(raw, raw), x1 = fe_sub<6, 29>(raw, raw);
  F tt = fe_norm(x1);
  F y0 = fe_add(x0, tt), y1 = fe_sub<13, 29>(x0, tt);
  F g = fe_mul(fe_norm(y1), z);
  F b0 = fe_add(fe_norm(y0), g), b1 = fe_sub<3, 29>(fe_norm(y0), g);
  F o0 = fe_norm(b0), o1 = fe_norm(b1);
  report[r++] = o0.vb;
  report[r++] = o1.vb;
  (void)fe_canonical(fe_reduce_small(o0));
  (void)fe_canonical(fe_mul(o1, z));
  return ok;
}

// The SRS codec (g1_codec.inc) on n entries, the exact per-point code of its kernels.  op 0: compress (16 words in, 8 out);
// 1: decompress (8 words in, 16 out); 2: check (16 words in).  valid[i] = 1 / 0.  The tracked bounds are data-independent (every
// input enters through fe_unpack / fe_from_ext at the 2^256 class), so one valid point of each y parity proves them for all inputs.
void hc_g1_codec(int op, const uint32_t* in, uint32_t* out, int* valid, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t a[8], b[8], o1[8], o2[8];
    if (op == 1) {
      std::memcpy(a, in + 8 * i, 32);
      valid[i] = g1_decompress_one(a, o1, o2) ? 1 : 0;
      std::memcpy(out + 16 * i, o1, 32);
      std::memcpy(out + 16 * i + 8, o2, 32);
      continue;
    }
    std::memcpy(a, in + 16 * i, 32);
    std::memcpy(b, in + 16 * i + 8, 32);
    if (op == 0) {
      g1_compress_one(a, b, o1);
      std::memcpy(out + 8 * i, o1, 32);
      valid[i] = 1;
    } else {
      valid[i] = g1_check_one(a, b) ? 1 : 0;
    }
  }
}

// The batch verifier's read (verify_read.inc) on n slots, the exact per-slot code of its kernel.  kinds[i] != 0: a point slot, 8 words
// in, 24 out (x, y Montgomery, then the canonical words of y); 0: a scalar slot, 8 in, the first 8 of the 24 out.  valid[i] = 1 / 0.
// Every input enters at the 2^256 class, so one slot of each kind proves the bounds for all inputs.
void hc_verify_read(const uint8_t* kinds, const uint32_t* in, uint32_t* out, int* valid, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t a[8], o1[8] = {0}, o2[8] = {0}, o3[8] = {0};
    std::memcpy(a, in + 8 * i, 32);
    valid[i] = (kinds[i] ? proof_point_one(a, o1, o2, o3) : proof_scalar_one(a, o1)) ? 1 : 0;
    std::memcpy(out + 24 * i, o1, 32);
    std::memcpy(out + 24 * i + 8, o2, 32);
    std::memcpy(out + 24 * i + 16, o3, 32);
  }
}

// ... and its column sum: rows x cols Montgomery words -> cols sums over rows [lo, hi), by the kernel's step, join and finish (the rows
// dealt to `lanes` partial sums as the kernel deals them to its threads, then folded as its tree folds them).
int hc_verify_column_sum(const uint32_t* rows, size_t n_rows, uint32_t cols, size_t lo, size_t hi, uint32_t lanes, uint32_t* out) {
  if (lo > hi || hi > n_rows || lanes == 0 || (lanes & (lanes - 1))) return -1;
  for (uint32_t c = 0; c < cols; ++c) {
    std::vector<Fr> part(lanes, fe_zero<FrParams>());
    for (size_t r = lo; r < hi; ++r) {
      uint32_t w[8];
      std::memcpy(w, rows + (r * cols + c) * 8, 32);
      Fr& acc = part[(r - lo) % lanes];
      acc = colsum_step(acc, w);
    }
    for (uint32_t s = lanes / 2; s > 0; s >>= 1)
      for (uint32_t t = 0; t < s; ++t) {
        Fr o = part[t + s];
        HM_DECLARE(o, 3.0);
        part[t] = colsum_join(part[t], o);
      }
    uint32_t w[8];
    colsum_finish(part[0], w);
    std::memcpy(out + (size_t)c * 8, w, 32);
  }
  return 0;
}

// The per-proof sums (verify_sums.inc): proof b of a batch by the kernel's own lane functions -- `lanes` partial sums dealt as the
// kernel deals the terms to its threads, record `lanes` for L, the halving fold as a plain loop, the two finishing lanes -- with every
// accumulator re-declared at the Jacobian class maxima where the kernel reads it back from LDS.  Arguments as
// hm_verify_proof_sums_dev's (all host memory); pairs: the proof's 2 rows of 16 words.  fold_doublings (may be null): how many steps
// of the fold added two equal points -- g1_add then returns g1_double_nz of its first operand, limb for limb -- so that a test can
// tell that its rows reach that branch.
static bool same_limbs(const G1Jac& a, const G1Jac& b) {
  for (int i = 0; i < 9; ++i)
    if (a.x.l[i] != b.x.l[i] || a.y.l[i] != b.y.l[i] || a.z.l[i] != b.z.l[i]) return false;
  return a.inf == b.inf;
}
int hc_verify_proof_sums(const uint32_t* bases, size_t n_proofs, uint32_t own_points, uint32_t shared_points, const uint32_t* own,
                         const uint32_t* shared, const uint32_t* h2_r, const uint32_t* h2_l, const uint32_t* bad, size_t b, uint32_t lanes,
                         uint32_t* pairs, uint32_t* fold_doublings) {
  if (fold_doublings) *fold_doublings = 0;
  if (b >= n_proofs || lanes < 2 || (lanes & (lanes - 1))) return -1;
  if (bad[b]) {
    std::memset(pairs, 0, 2 * VS_ROW_WORDS * 4);
    return 0;
  }
  const VsArgs a{bases, own, shared, h2_r, h2_l, (uint64_t)n_proofs, own_points, shared_points};
  std::vector<uint32_t> tree((size_t)(lanes + 1) * VS_ACC_WORDS, 0u);
  uint32_t* left = tree.data() + (size_t)lanes * VS_ACC_WORDS;
  for (uint32_t t = 0; t < lanes; ++t) vs_lane(a, b, t, lanes, tree.data() + (size_t)t * VS_ACC_WORDS, left);
  for (uint32_t off = lanes / 2; off > 0; off >>= 1)
    for (uint32_t t = 0; t < off; ++t) {
      const G1Jac x = vs_load_acc(tree.data() + (size_t)t * VS_ACC_WORDS), y = vs_load_acc(tree.data() + (size_t)(t + off) * VS_ACC_WORDS);
      if (fold_doublings && !x.inf && !y.inf && same_limbs(g1_add(x, y), g1_double_nz(x))) ++*fold_doublings;
      vs_fold_step(tree.data(), t, off);
    }
  vs_finish(tree.data(), true, pairs + VS_ROW_WORDS);
  vs_finish(left, false, pairs);
  return 0;
}

// The two double-and-add loops of g1_mul.h on one affine base (16 Montgomery words, not the identity) and one 256-bit integer (8
// words): 1 when g1_mul_words and g1_mul_words_by_field give the same limbs and flag; row: the product as vs_finish writes it.
int hc_g1_mul_words_pair(const uint32_t* base, const uint32_t* e_words, uint32_t* row) {
  const G1Jac p = vs_load_base(base);
  if (p.inf) return -1;
  uint32_t e[8];
  std::memcpy(e, e_words, 32);
  const G1Jac whole = g1_mul_words(p, e), by_field = g1_mul_words_by_field(p, e);
  uint32_t record[VS_ACC_WORDS];
  vs_store_acc(record, by_field.inf ? g1_identity() : by_field);
  vs_finish(record, false, row);
  return (whole.inf && by_field.inf) || same_limbs(whole, by_field) ? 1 : 0;
}

// The pairing operands of one user's ledger opening (ledger.inc): ld_pair, the kernel's own lane function, on host memory.  gamma,
// omega: 8 Montgomery words each; c_gamma, opening: 16 affine words; id: 8 words; balances: assets x 8 words; rows: 32 words.
// Returns the user's flag, -1 for arguments the C entry refuses.
int hc_ledger_pair(const uint32_t* gamma, const uint32_t* omega, const uint32_t* c_gamma, uint32_t log_n, uint32_t assets,
                   const uint32_t* opening, uint32_t index, const uint32_t* id, const uint32_t* balances, uint32_t* rows) {
  if (log_n > 28 || assets > LD_MAX_ASSETS) return -1;
  LdShared s;
  std::memcpy(s.gamma, gamma, 32);
  std::memcpy(s.omega, omega, 32);
  std::memcpy(s.c_gamma, c_gamma, 64);
  s.k = log_n;
  s.assets = assets;
  return (int)ld_pair(s, opening, index, id, balances, rows);
}

// Blake2b and the transcripts (transcript.inc), the exact lane code of its kernels on a block of 32 host words.
//   hc_blake2b_compress: h <- F(h, the 128 bytes of `block`, t, last).
//   hc_blake2b: n messages at a byte stride -> n x 64 digest bytes; personal16 null or 16 bytes.
//   hc_transcript_stream: ops[i] = 0 a squeeze (prefix byte 0, then a digest of a COPY: 64 bytes to `digests`), 1 a 65-byte record
//     (prefix 1 and 16 words of `data`), 2 a 33-byte record (prefix 2 and 8 words); positions[i] = the bytes in the block after op i.
//   hc_fr_from_wide: n digests of 64 bytes -> n x 8 Montgomery words of the little-endian integer mod r.
//   hc_verify_transcript: tr_proof_one on proof b of a batch, arguments as hm_verify_transcript_dev's (all host memory).
void hc_blake2b_compress(uint64_t* h, const uint8_t* block, uint64_t t, int last) {
  uint64_t hh[8], m[16];
  std::memcpy(hh, h, 64);
  std::memcpy(m, block, 128);
  blake2b_compress(hh, m, t, last != 0);
  std::memcpy(h, hh, 64);
}
void hc_blake2b(const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t n, const uint8_t* personal16, uint8_t* out) {
  uint64_t personal[2] = {0, 0};
  if (personal16) std::memcpy(personal, personal16, 16);
  for (size_t i = 0; i < n; ++i) {
    uint32_t block[32] = {0}, digest[16];
    b2_hash_lane(B2Buf{block, 1}, msgs + i * stride, lens[i], personal[0], personal[1], digest);
    std::memcpy(out + 64 * i, digest, 64);
  }
}
void hc_transcript_stream(const uint8_t* ops, size_t n_ops, const uint32_t* data, uint8_t* digests, uint32_t* positions) {
  uint32_t block[32] = {0};
  const B2Buf buf{block, 1};
  B2State s;
  b2_init(s, TR_PERSONAL_LO, TR_PERSONAL_HI);
  for (size_t i = 0; i < n_ops; ++i) {
    const uint32_t words = ops[i] == 0 ? 0 : ops[i] == 1 ? 16 : 8;
    b2_push(s, buf, ops[i], 1);
    for (uint32_t k = 0; k < words; ++k) b2_push(s, buf, *data++, 4);
    if (words == 0) {
      uint64_t d[8];
      b2_final(s, buf, d);
      std::memcpy(digests, d, 64);
      digests += 64;
    }
    positions[i] = s.pos;
  }
}
void hc_fr_from_wide(const uint8_t* digests, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) {
    uint64_t d[8];
    uint32_t w[8];
    std::memcpy(d, digests + 64 * i, 64);
    fr_from_wide(d, w);
    std::memcpy(out + 8 * i, w, 32);
  }
}
void hc_verify_transcript(size_t b, const uint32_t* proofs, const uint32_t* slot_table, uint32_t slots, uint32_t points, const uint32_t* ybytes,
                          const uint32_t* preamble, const uint32_t* counts, uint32_t stride, const uint32_t* schedule, uint32_t n_pairs,
                          uint32_t* bad, uint32_t* records, uint32_t record_elems) {
  uint32_t block[B2_BLOCK_WORDS + TR_STAGE_WORDS] = {0};
  tr_proof_one(B2Buf{block, 1}, b, proofs, slot_table, slots, points, ybytes, preamble, counts, stride, schedule, n_pairs, bad, records,
               record_elems);
}
const char* hc_transcript_schedule_problem(const uint32_t* schedule, size_t n_pairs, uint32_t slots, uint32_t record_elems) {
  return tr_schedule_problem(schedule, n_pairs, slots, record_elems);
}

// Keccak-256 and the EVM encoding (keccak.inc), the exact lane code of its kernels on a block of 34 host words.
//   hc_keccak256: n messages at a byte stride -> n x 32 digest bytes, with the padding's domain byte as given (0x01 Keccak, 0x06 SHA-3).
//   hc_keccak_stream: ops[i] = 0 a squeeze (kc_squeeze_restart: 32 digest bytes to `digests`), 1 a word of 32 bytes absorbed (8 words
//     of `data`); positions[i] = the bytes in the block after op i.
//   hc_keccak_challenge: n digests of 32 bytes -> n x 8 Montgomery words of the big-endian integer mod r.
//   hc_evm_read: evm_read_slot on every slot of one proof -> 1 when every slot was read, 0 otherwise.
//   hc_verify_transcript_evm: evm_proof_one on proof b of a batch, arguments as hm_verify_transcript_evm_dev's (all host memory).
void hc_keccak256(const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t n, uint32_t domain, uint8_t* out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t block[KC_BLOCK_WORDS] = {0}, digest[8];
    kc_hash_lane(KcBuf{block, 1}, msgs + i * stride, lens[i], domain, digest);
    std::memcpy(out + 32 * i, digest, 32);
  }
}
void hc_keccak_stream(const uint8_t* ops, size_t n_ops, const uint32_t* data, uint8_t* digests, uint32_t* positions) {
  uint32_t block[KC_BLOCK_WORDS] = {0};
  const KcBuf buf{block, 1};
  KcState s;
  kc_init(s);
  for (size_t i = 0; i < n_ops; ++i) {
    if (ops[i]) {
      for (int k = 0; k < 8; ++k) kc_push_word(s, buf, *data++);
    } else {
      uint32_t d[8];
      kc_squeeze_restart(s, buf, d);
      std::memcpy(digests, d, 32);
      digests += 32;
    }
    positions[i] = s.pos;
  }
}
void hc_keccak_challenge(const uint8_t* digests, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t d[8], w[8];
    std::memcpy(d, digests + 32 * i, 32);
    kc_challenge(d, w);
    std::memcpy(out + 8 * i, w, 32);
  }
}
int hc_evm_read(const uint32_t* proof, const uint32_t* slot_table, uint32_t slots, uint32_t own_points, uint32_t scalars, uint32_t* points,
                uint32_t* tail, uint32_t* out_scalars) {
  int ok = 1;
  for (uint32_t s = 0; s < slots; ++s)
    if (!evm_read_slot(proof, s, slots, slot_table[s], own_points, scalars, points, tail, out_scalars)) ok = 0;
  return ok;
}
void hc_verify_transcript_evm(size_t b, const uint32_t* proofs, uint32_t slots, const uint32_t* preamble, const uint32_t* counts, uint32_t stride,
                              const uint32_t* schedule, uint32_t n_pairs, uint32_t* bad, uint32_t* records, uint32_t record_elems) {
  uint32_t block[KC_BLOCK_WORDS] = {0};
  evm_proof_one(KcBuf{block, 1}, b, proofs, slots, preamble, counts, stride, schedule, n_pairs, bad, records, record_elems);
}

// The batch verifier's terms (verify_terms.inc) for ONE proof, the exact lane code of its kernel on a workspace of one lane: phase a,
// then -- the interpreter's run is hc_graph_replay's business -- the numerator as the caller gives it (4 Montgomery words), then
// phase b.  vals: the value row as phase a left it (n_vals x 8 words, h(x) filled in by phase b).  -> 1 / 0: the lane's ok flag; -1
// with *why set when the plan fails its check.
int hc_verify_terms(const uint32_t* plan, size_t n_words, size_t n_columns, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst,
                    const uint32_t* numerator, uint32_t* vals, uint32_t* own, uint32_t* shared, uint32_t* h2r, uint32_t* h2l, const char** why) {
  *why = vt_plan_problem(plan, n_words, n_columns);
  if (*why) return -1;
  std::vector<uint32_t> ws((size_t)vt_ws_program(plan) * 9, 0);
  const VtMem m{ws.data(), 1, 0};
  bool ok = vt_phase_a(plan, m, rec, evals, inst);
  Fr num = vt_from_ext(numerator);
  ok = vt_phase_b(plan, m, num, own, shared, h2r, h2l) && ok;
  for (uint32_t s = 0; s < plan[VT_N_VALS]; ++s) vt_to_ext(vals + 8 * (size_t)s, vt_load(m, s));
  return ok ? 1 : 0;
}
// The terms of ONE proof that ends in the GWC multiopen: the lane code of verify_terms_gwc_kernel on a workspace of one lane, as
// hc_verify_terms.  rec: 8 elements (theta, beta, gamma, y, x, v, u, r_b); w_left: q x 8 words.  -> 1 / 0: the lane's ok flag (all
// rows zero on 0, as the kernel leaves them); -1 with *why set when the plan fails vg_plan_problem.
int hc_verify_terms_gwc(const uint32_t* plan, size_t n_words, size_t n_columns, const uint32_t* rec, const uint32_t* evals, const uint32_t* inst,
                        const uint32_t* numerator, uint32_t* vals, uint32_t* own, uint32_t* shared, uint32_t* w_left, const char** why) {
  *why = vg_plan_problem(plan, n_words, n_columns);
  if (*why) return -1;
  std::vector<uint32_t> ws((size_t)vt_ws_program(plan) * 9, 0);
  const VtMem m{ws.data(), 1, 0};
  vg_zero_lane(plan, own, shared, w_left);
  const bool ok = vg_phase_a(plan, m, rec, evals, inst);
  vg_phase_b(plan, m, vt_from_ext(numerator), own, shared, w_left);
  for (uint32_t s = 0; s < plan[VT_N_VALS]; ++s) vt_to_ext(vals + 8 * (size_t)s, vt_load(m, s));
  if (!ok) vg_zero_lane(plan, own, shared, w_left);
  return ok ? 1 : 0;
}
// The terms of ONE multi-circuit proof (verify_terms.inc): the lane code of verify_terms_multi_kernel on a workspace of
// 64 lanes, lane c = circuit c, with the two cross-lane folds as plain loops over the lanes.  plan: the multi plan; evals: the proof's
// scalars in the proof's order; inst: circuits rows; numerators: N_c of every circuit (circuits x 4 Montgomery words), as
// hc_verify_terms is given its one; vals: circuits x n_vals x 8 words, every lane's value row.  -> 1 / 0: no lane failed / one did
// (all rows zero then, as the kernel leaves them); -1 with *why set when the plan fails its check.
int hc_verify_terms_multi(const uint32_t* plan, size_t n_words, size_t n_columns, uint32_t circuits, const uint32_t* rec, const uint32_t* evals,
                          const uint32_t* inst, const uint32_t* numerators, uint32_t* vals, uint32_t* own, uint32_t* shared, uint32_t* h2r,
                          uint32_t* h2l, const char** why) {
  *why = vtm_plan_problem(plan, n_words, n_columns, circuits);
  if (*why) return -1;
  const uint32_t* lp = vtm_lane_plan(plan);
  const uint32_t T = VM_MAX_CIRCUITS;
  std::vector<uint32_t> ws((size_t)vt_ws_program(lp) * 9 * T, 0);
  for (uint32_t c = 0; c < T; ++c) vt_zero_lane(lp, VtmLane{plan, c}, own, shared, h2r, h2l);
  bool ok = true;
  Fr num = fe_zero<FrParams>();
  HM_DECLARE(num, 3.0);
  for (uint32_t c = 0; c < circuits; ++c) {
    const VtMem m{ws.data(), T, c};
    ok = vtm_phase_a(plan, m, c, rec, evals, inst + 8 * (size_t)c * lp[VT_INST_ELEMS]) && ok;
    num = vt_add(num, vtm_numerator_term(plan, m, c, vt_from_ext(numerators + 8 * (size_t)c)));
  }
  Fr r_outer = fe_zero<FrParams>();
  HM_DECLARE(r_outer, 3.0);
  VtmShare first{};
  for (uint32_t c = 0; c < circuits; ++c) {
    const VtMem m{ws.data(), T, c};
    const VtmShare mine = vt_set_walk(lp, m, VtmLane{plan, c}, num, own, shared);
    ok = ok && mine.ok;
    r_outer = vt_add(r_outer, mine.r_outer);
    if (c == 0) first = mine;
    for (uint32_t s = 0; s < lp[VT_N_VALS]; ++s) vt_to_ext(vals + 8 * ((size_t)c * lp[VT_N_VALS] + s), vt_load(m, s));
  }
  if (ok) {
    vt_finish(lp, plan[VM_N_OWN], VtMem{ws.data(), T, 0}, r_outer, first, own, shared, h2r, h2l);
  } else {
    for (uint32_t c = 0; c < T; ++c) vt_zero_lane(lp, VtmLane{plan, c}, own, shared, h2r, h2l);
  }
  return ok ? 1 : 0;
}
// Phase a alone: the nine record slots as the lane's workspace holds them, limb by limb (9 x 9 words).  ge_run reads four of them as
// constants, which it takes for canonical: below r, where everything else kept in the workspace is merely below 3r.
int hc_verify_terms_record(const uint32_t* plan, size_t n_words, size_t n_columns, const uint32_t* rec, const uint32_t* evals,
                           const uint32_t* inst, uint32_t* limbs) {
  if (vt_plan_problem(plan, n_words, n_columns)) return -1;
  std::vector<uint32_t> ws((size_t)vt_ws_program(plan) * 9, 0);
  const VtMem m{ws.data(), 1, 0};
  const bool ok = vt_phase_a(plan, m, rec, evals, inst);
  for (uint32_t j = 0; j < VT_REC * 9; ++j) limbs[j] = ws[(size_t)plan[VT_N_VALS] * 9 + j];
  return ok ? 1 : 0;
}

// Poseidon (poseidon.inc) on n messages, the exact per-hash code of its kernels.  consts: the spec's block as the library lays it out
// on the device (rc, mds, capacity word; 9 limbs each, canonical internal form).  op 0: n x (width - 1) elements -> n digests;
// op 1 (width 5 only): n x 4 elements (hash, balance, hash, balance) -> n x 2 (hash, balance), a Merkle sum tree node.
// The tracked bounds are data-independent: one message proves the 64-round chain for all inputs.
int hc_poseidon(int op, uint32_t width, const uint32_t* consts, uint32_t r_f, uint32_t r_p, const uint32_t* in, uint32_t* out, size_t n) {
  if ((width != 3 && width != 5) || (op == 1 && width != 5) || (op != 0 && op != 1)) return -1;
  for (size_t i = 0; i < n; ++i) {
    if (width == 3) {
      uint32_t msg[2][8], d[8];
      std::memcpy(msg, in + 16 * i, 64);
      poseidon_hash_one<3>(msg, consts, r_f, r_p, d);
      std::memcpy(out + 8 * i, d, 32);
    } else {
      uint32_t msg[4][8], d[8], b[8];
      std::memcpy(msg, in + 32 * i, 128);
      if (op == 0) {
        poseidon_hash_one<5>(msg, consts, r_f, r_p, d);
        std::memcpy(out + 8 * i, d, 32);
      } else {
        merkle_sum_node_one(msg, consts, r_f, r_p, d, b);
        std::memcpy(out + 16 * i, d, 32);
        std::memcpy(out + 16 * i + 8, b, 32);
      }
    }
  }
  return 0;
}

// The SHPLONK set quotient (shplonk.inc), what of it runs without a GPU.
//   hc_shplonk_plan: plan[0..2] = B, G, lanes and plan[3] = the scratch words of one point, for n rows.
//   hc_shplonk_coefficients: d[l] = scale / prod_{l' != l} (pts[l] - pts[l']) (external words) -> 0; -1 when the set is refused
//     (t out of range, two equal points, a word not below r).
//   hc_shplonk_row_bounds: the row formula with t = SHQ_T_MAX terms, every quotient value DECLARED at its class maximum (< 3r), the
//     coefficients at the class of a converted constant and the accumulated word at the raw 2^256 class -> 1 when the result is inside
//     the class the canonical store expects; report[0] = its bound.  A violated precondition aborts.
void hc_shplonk_plan(uint64_t n, uint64_t* plan) {
  const ShqPlan p = shq_plan(n);
  plan[0] = p.B, plan[1] = p.G, plan[2] = p.lanes, plan[3] = shq_scan_words(p);
}
int hc_shplonk_coefficients(uint32_t t, const uint64_t* pts_ext, const uint64_t* scale_ext, uint64_t* d_ext) {
  if (t > (uint32_t)SHQ_T_MAX) return -1;
  host::Fr4 pts[SHQ_T_MAX], d[SHQ_T_MAX];
  for (uint32_t l = 0; l < t; ++l) pts[l] = host::fr_load(pts_ext + 4 * l);
  if (!shq_coefficients(t, pts, host::fr_load(scale_ext), d)) return -1;
  for (uint32_t l = 0; l < t; ++l) std::memcpy(d_ext + 4 * l, d[l].l, 32);
  return 0;
}
// hm_graph_evaluate_proofs_dev's address rule (graph_lower.h: graph_proofs_*), as the kernel applies it to one lane and one column
// source: out = { proof, row of the proof, the row the source reads, the cell's u32 word behind the column base, the word of the
// constant table for `word` of that proof }
void hc_graph_proofs_address(uint64_t lane, uint64_t rows, uint32_t log_segment, int64_t rotation, uint32_t log_rows, uint64_t stride_words,
                             uint32_t n_dynamic, uint32_t word, uint64_t* out) {
  const uint64_t proof = graph_proofs_proof(lane, rows), idx = lane - proof * rows;
  const uint64_t row = graph_source_row(idx, rotation, ((uint64_t)1 << log_segment) - 1, log_rows);
  out[0] = proof, out[1] = idx, out[2] = row, out[3] = graph_proofs_cell(proof, row, stride_words), out[4] = graph_proofs_dyn(proof, n_dynamic, word);
}
// The evaluator's call check and launch plan (graph_lower.h), as graph_run asks them.  Addresses travel as integers: bases, and strides
// unless null (the single kind), hold n_columns words.  -> the reason, or null for an admitted call.
const char* hc_graph_check_call(uint32_t kind, uint64_t n_columns, uint64_t units, uint64_t n_dyn, uint32_t log_size, uint32_t segments,
                                uint32_t flags, uint64_t values, uint64_t values_stride, const uint64_t* bases, const uint64_t* strides,
                                uint64_t program_columns, uint64_t program_dynamic) {
  static_assert(sizeof(void*) == sizeof(uint64_t), "bases are read as pointers");
  const GraphCall c{(GraphCallKind)kind, (size_t)n_columns, (size_t)units, (size_t)n_dyn, log_size, segments, flags, (const void*)(uintptr_t)values,
                    values_stride, reinterpret_cast<const void* const*>(bases), strides, nullptr};
  return graph_check_call(c, (size_t)program_columns, (size_t)program_dynamic);
}
// out = { size, lanes, blocks, T, log_c, rows_per, scratch_bytes, args_bytes }
void hc_graph_launch_plan(uint32_t kind, uint64_t size, uint64_t units, uint32_t n_slots, uint64_t n_dyn, uint32_t max_blocks, uint64_t* out) {
  const GraphPlan p = graph_launch_plan((GraphCallKind)kind, size, units, n_slots, (size_t)n_dyn, max_blocks);
  out[0] = p.size, out[1] = p.lanes, out[2] = p.blocks, out[3] = p.T, out[4] = p.log_c, out[5] = p.rows_per, out[6] = p.scratch_bytes, out[7] = p.args_bytes;
}
// The NTT's call check and launch plan (ntt_plan.inc), as ntt_run asks them.  call = { log_n, batch, fwd_cosets, inv_cosets, log_z,
// fused, in_place, in, out } (addresses as integers).  hc_ntt_check_call -> the reason, or null for an admitted call.  hc_ntt_plan, for
// an admitted call: head = { passes, digits[3], arrays, lds_bytes, scratch_bytes, tail, tail_grid[2], table bytes, tables };
// passes = 3 rows of { the 13 words of NttPassHead, variant, grid[3], src, dst, stage, tw_lo, tw_hi (table indices, -1: none) };
// tables = NTT_TABLES_MAX rows of { role, count, shift }.
static NttCall hc_ntt_call(const uint64_t* call) {
  return NttCall{(uint32_t)call[0], call[1], (uint32_t)call[2], (uint32_t)call[3], (uint32_t)call[4], (uint32_t)call[5], call[6] != 0,
                 (uintptr_t)call[7], (uintptr_t)call[8]};
}
const char* hc_ntt_check_call(const uint64_t* call) { return ntt_check_call(hc_ntt_call(call)); }
void hc_ntt_plan(const uint64_t* call, uint64_t* head, int64_t* passes, uint64_t* tables) {
  const NttPlan p = ntt_plan(hc_ntt_call(call));
  const uint64_t h[12] = {p.passes, p.digits[0], p.digits[1], p.digits[2], p.arrays, p.lds_bytes, p.scratch_bytes, p.tail, p.tail_grid[0], p.tail_grid[1],
                          p.tables.bytes, p.tables.n_tables};
  std::memcpy(head, h, sizeof h);
  for (int i = 0; i < 3; ++i) {
    const NttPassPlan& q = p.pass[i];
    const NttPassHead& s = q.head;
    const int64_t row[22] = {s.log_n, s.s, s.log_stride, s.log_c, s.last, s.log_r0, s.log_rows, s.log_lb, s.fin_mode, s.has_coset, s.direct_tw, s.log_z,
                             s.has_table, q.variant, q.grid[0], q.grid[1], q.grid[2], q.src, q.dst, q.stage, q.tw_lo, q.tw_hi};
    std::memcpy(passes + 22 * i, row, sizeof row);
  }
  for (int i = 0; i < NTT_TABLES_MAX; ++i) {
    const uint64_t row[3] = {p.tables.table[i].role, p.tables.table[i].count, p.tables.table[i].shift};
    std::memcpy(tables + 3 * i, row, sizeof row);
  }
}
int hc_ntt_extending_applies(uint32_t log_n, uint32_t log_z) { return ntt_extending_applies(log_n, log_z) ? 1 : 0; }
int hc_shplonk_row_bounds(const uint64_t* a_ext, double* report) {
  typedef Fe<FrParams> F;
  uint32_t wa[8];
  std::memcpy(wa, a_ext, 32);
  F raw = fe_unpack<FrParams>(wa);                 // declared: any 256-bit word pattern; run at the largest one
  raw.l[8] = (1u << 24) - 1;
  for (int i = 0; i < 8; ++i) raw.l[i] = MASK29;
  F q[SHQ_T_MAX], d[SHQ_T_MAX];
  for (int l = 0; l < SHQ_T_MAX; ++l) {
    q[l] = load_ext<FrParams>(a_ext);
    force_bounds(q[l], 3.0);
    d[l] = load_ext<FrParams>(a_ext);
    force_bounds(d[l], 1.0);
  }
  const F row = shq_row<SHQ_T_MAX>(q, d, true, raw);
  report[0] = row.vb;
  (void)fe_canonical(row);
  return row.vb <= 3.0 ? 1 : 0;
}

}  // extern "C"

// The witnesses of the three circuits (poseidon.inc) of m users / messages on host memory: the lane functions their kernels run, lane
// by lane, so that the limb bounds of the traced permutation and of the less-than arithmetic are proven on the code the GPU executes.
// E = 2 MerkleSumTree, 1 MerkleTreeV3, 0 the Poseidon circuit.  advice must be cleared by the caller, as on the device.
static int hc_witness_args(uint32_t E, const uint32_t* consts, uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, size_t m,
                           const uint32_t* leaves, uint32_t* advice, uint32_t* instance, WitnessArgs& a) {
  if ((E && (depth == 0 || depth > 32)) || (r_f & 1) || (r_p & 1)) return -1;
  if (((uint64_t)1 << log_n) < (uint64_t)witness_layout(E, depth, r_f, r_p).rows_used + 6) return -1;
  a = WitnessArgs{};
  a.leaves = leaves, a.advice = advice, a.instance = instance, a.consts = consts;
  a.m = m, a.depth = depth, a.log_n = log_n, a.r_f = r_f, a.r_p = r_p;
  return 0;
}
template <int E>
static void hc_merkle_lanes(WitnessArgs& a, const uint32_t* siblings, const uint64_t* indices, const uint32_t* nodes, uint32_t* run) {
  a.siblings = siblings, a.indices = indices, a.nodes = nodes, a.run = nodes ? nullptr : run;
  for (size_t u = 0; u < a.m; ++u) {
    if (!nodes) merkle_chain_lane<E>(a, u, run);
    for (uint32_t l = 0; l < a.depth; ++l) merkle_witness_lane<E>(a, u, l);
  }
}

extern "C" {
// run: m x (depth - 1) x 16 words of scratch (used when nodes is null)
int hc_merkle_sum_witness(const uint32_t* consts, uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, size_t m, const uint32_t* leaves,
                          const uint32_t* siblings, const uint64_t* indices, const uint32_t* assets, const uint32_t* nodes, uint32_t* run,
                          uint32_t* advice, uint32_t* instance) {
  WitnessArgs a;
  if (int rc = hc_witness_args(2, consts, r_f, r_p, depth, log_n, m, leaves, advice, instance, a)) return rc;
  std::memcpy(a.assets, assets, 32);
  hc_merkle_lanes<2>(a, siblings, indices, nodes, run);
  return 0;
}

// run: m x (depth - 1) x 8 words of scratch (used when nodes is null)
int hc_merkle_witness(const uint32_t* consts, uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, size_t m, const uint32_t* leaves,
                      const uint32_t* siblings, const uint64_t* indices, const uint32_t* nodes, uint32_t* run, uint32_t* advice,
                      uint32_t* instance) {
  WitnessArgs a;
  if (int rc = hc_witness_args(1, consts, r_f, r_p, depth, log_n, m, leaves, advice, instance, a)) return rc;
  hc_merkle_lanes<1>(a, siblings, indices, nodes, run);
  return 0;
}

int hc_poseidon_witness(const uint32_t* consts, uint32_t r_f, uint32_t r_p, uint32_t log_n, size_t m, const uint32_t* msgs, uint32_t* advice,
                        uint32_t* instance) {
  WitnessArgs a;
  if (int rc = hc_witness_args(0, consts, r_f, r_p, 0, log_n, m, msgs, advice, instance, a)) return rc;
  for (size_t u = 0; u < m; ++u) poseidon_witness_lane(a, u);
  return 0;
}

// the lanes of range_witness_kernel, one after the other; over: m counters
int hc_range_witness(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* values, uint32_t* advice,
                     uint32_t* over) {
  if (max_bits == 0 || max_bits > RANGE_MAX_BITS || acc_cols == 0 || max_bits * acc_cols > RANGE_MAX_VALUE_BITS || log_n > 24 || rows == 0 ||
      rows > ((uint64_t)1 << log_n))
    return -1;
  const RangeArgs a{values, advice, over, (uint64_t)m << log_n, max_bits, acc_cols, log_n, rows};
  for (size_t c = 0; c < m; ++c) over[c] = 0;
  for (uint64_t idx = 0; idx < a.lanes; ++idx) over[idx >> log_n] += range_witness_lane(a, idx) ? 1u : 0u;
  return 0;
}

// the lanes of sorted_witness_kernel, one after the other; over: m counters
int hc_sorted_witness(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* ids, uint32_t* advice,
                      uint32_t* over) {
  if (max_bits == 0 || max_bits > RANGE_MAX_BITS || acc_cols == 0 || max_bits * acc_cols + log_n > RANGE_MAX_VALUE_BITS || log_n > 24 ||
      rows == 0 || rows > ((uint64_t)1 << log_n))
    return -1;
  const SortedArgs a{ids, advice, over, (uint64_t)m << log_n, max_bits, acc_cols, log_n, rows};
  for (size_t c = 0; c < m; ++c) over[c] = 0;
  for (uint64_t idx = 0; idx < a.lanes; ++idx) over[idx >> log_n] += sorted_witness_lane(a, idx) ? 1u : 0u;
  return 0;
}

// sorted_record_less on two records of 9 words: the order the argsort's network sorts by
int hc_sorted_record_less(const uint32_t* a, const uint32_t* b) {
  uint32_t x[9], y[9];
  std::memcpy(x, a, 36);
  std::memcpy(y, b, 36);
  return sorted_record_less(x, y) ? 1 : 0;
}

// The accumulator witness with the rows of a circuit one after the other: what accumulator.hip's four launches compute, S_(r-1)
// carried from row to row instead of scanned.  initial: m x acc_cols plain limbs; finals: the same shape; over: m counters.
int hc_accumulator_witness(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint32_t* values,
                           const uint64_t* initial, uint32_t* advice, uint64_t* finals, uint32_t* over) {
  if (max_bits == 0 || max_bits > ACC_MAX_BITS || acc_cols < 2 || max_bits * acc_cols > ACC_MAX_WIDTH || log_n > 24 || rows == 0 ||
      (uint64_t)rows + 1 > ((uint64_t)1 << log_n))
    return -1;
  uint64_t inverses[15 * 4];
  host::fr_small_inverses((1u << max_bits) - 1, inverses);
  const AccArgs a{values, initial, (const uint32_t*)inverses, advice, finals, max_bits, acc_cols, log_n, rows};
  const uint64_t n = (uint64_t)1 << log_n, col_words = n * 8;
  const uint32_t n_cols = 2 + 2 * acc_cols;
  for (size_t c = 0; c < m; ++c) {
    uint32_t* base = advice + c * n_cols * col_words;
    uint64_t s;
    over[c] = acc_initial_state(a, c, s) ? 1u : 0u;
    acc_zero_cells(base, col_words, 0, 2 + acc_cols);
    for (uint32_t i = 0; i < acc_cols; ++i) acc_initial_cell(a, c, i);
    for (uint64_t t = 1; t <= rows; ++t) {
      uint32_t w[8];
      ps_get_words(values + (c * rows + (t - 1)) * 8, w);
      uint64_t s_new;
      over[c] += accumulator_row(a, base + t * 8, s, w, s_new) ? 1u : 0u;
      s = s_new;
    }
    acc_write_finals(a, c, s);
    for (uint64_t t = (uint64_t)rows + 1; t < n; ++t) acc_zero_cells(base + t * 8, col_words, 0, n_cols);
  }
  return 0;
}

// The multiplicity column of ONE logUp argument with the rows one after the other (logup.inc: lu_key, lu_find, lu_count_ext): the table's
// keys in (key, row) order by std::sort in the place of the device's network or its value bins, every input key searched in them, the
// counter of the first row holding it raised.  inputs: c x rows x 8 words.  -> 1 when an input key is not in the table, -1 refused.
int hc_logup_multiplicities(const uint32_t* table, const uint32_t* inputs, uint32_t c, uint64_t rows, uint32_t* m) {
  if (rows == 0 || c == 0 || (uint64_t)c * rows >= ((uint64_t)1 << 32)) return -1;
  std::vector<uint32_t> plain(rows * 8), keys(rows * 8), counters(rows, 0u);
  std::vector<uint64_t> order(rows);
  for (uint64_t i = 0; i < rows; ++i) {
    uint32_t key[8];
    (void)lu_key(table + i * 8, 1u, key);
    std::memcpy(&plain[i * 8], key, 32);
    order[i] = i;
  }
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    const int cmp = mock_key_cmp(&plain[a * 8], &plain[b * 8]);
    return cmp != 0 ? cmp < 0 : a < b;
  });
  for (uint64_t i = 0; i < rows; ++i) std::memcpy(&keys[i * 8], &plain[order[i] * 8], 32);
  int missing = 0;
  for (uint64_t j = 0; j < (uint64_t)c * rows; ++j) {
    uint32_t key[8];
    (void)lu_key(inputs + j * 8, 1u, key);
    const uint64_t at = lu_find(keys.data(), rows, key);
    if (at < rows) counters[order[at]] += 1;
    else missing = 1;
  }
  LuFr to_mont;
  const host::Fr4 r2 = {{0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL}};   // 2^512 mod r as words = the element 2^256
  host::fr_to_internal9(r2, to_mont.l);
  for (uint64_t i = 0; i < rows; ++i) {
    uint32_t w[8];
    lu_count_ext(counters[i], to_mont, w);
    ps_put_words(m + i * 8, w);
  }
  return missing;
}

// out[i] = the sum of terms[0 .. i) mod r, carried from row to row with the addition logup.hip's scan adds with
int hc_grand_sum(const uint32_t* terms, uint64_t n, uint32_t* out) {
  uint32_t run[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t w[8];
    ps_get_words(terms + i * 8, w);
    ps_put_words(out + i * 8, run);
    lu_add_mod(run, w);
  }
  return 0;
}

// logup.inc's LU_COUNT_BITS: table keys below 2^this are counted in value bins
uint32_t hc_logup_count_bits() { return LU_COUNT_BITS; }

// The plan of a tree update (poseidon.inc: merkle_update_key / _owned / _count, the arithmetic its kernels run) on m host indices,
// with std::sort in the place of the device's sorting network.  counts: depth + 1 words.
int hc_merkle_update_plan(uint32_t depth, const uint64_t* indices, size_t m, uint32_t* counts) {
  if (depth == 0 || depth > 30 || m > ((size_t)1 << 31)) return -1;
  std::vector<uint64_t> keys(m);
  for (size_t p = 0; p < m; ++p) keys[p] = merkle_update_key(indices[p], (uint32_t)p, depth);
  std::sort(keys.begin(), keys.end());
  uint32_t hist[MU_BINS] = {};
  for (size_t p = 0; p < m; ++p) {
    const uint32_t d = merkle_update_owned(p ? keys[p - 1] : 0, keys[p], p == 0, depth);
    if (d >= MU_BINS) return -2;
    if (d) ++hist[d];
  }
  for (uint32_t l = 0; l <= depth; ++l) counts[l] = merkle_update_count(hist, l);
  return 0;
}

// the roots of m paths, lane by lane (merkle_root_lane<E>, the code of the roots kernel); width 5 -> E = 2, 3 -> E = 1
int hc_merkle_roots(uint32_t width, const uint32_t* consts, uint32_t r_f, uint32_t r_p, uint32_t depth, size_t m, const uint32_t* leaves,
                    const uint32_t* siblings, const uint64_t* indices, uint32_t* roots) {
  if ((width != 3 && width != 5) || depth == 0 || depth > 30) return -1;
  for (size_t u = 0; u < m; ++u) {
    if (width == 5)
      merkle_root_lane<2>(leaves, siblings, indices, depth, consts, r_f, r_p, u, roots);
    else
      merkle_root_lane<1>(leaves, siblings, indices, depth, consts, r_f, r_p, u, roots);
  }
  return 0;
}

// The permutation assembly (keygen.inc: perm_key / perm_link, the arithmetic its kernels run) on m host copies: a sequential
// union-find that hooks the larger root under the smaller, as the device's does, and std::sort in the place of the sorting network.
// sigma_cells: columns * 2^k words; *dropped: the pairs with an id out of range.
int hc_permutation_assemble(const uint32_t* copies, size_t m, uint32_t columns, uint32_t k, uint32_t* sigma_cells, uint32_t* dropped) {
  if (columns == 0 || k > 32 || ((uint64_t)columns << k) > ((uint64_t)1 << 32) || m > ((size_t)1 << 30)) return -1;
  const uint64_t cells = (uint64_t)columns << k;
  for (uint64_t c = 0; c < cells; ++c) sigma_cells[c] = (uint32_t)c;
  uint32_t* parent = sigma_cells;                       // the forest lives in the output, as on the device
  const auto find = [&](uint32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  std::vector<uint64_t> keys;
  keys.reserve(2 * m);
  *dropped = 0;
  for (size_t t = 0; t < m; ++t) {
    const uint32_t a = copies[2 * t], b = copies[2 * t + 1];
    if (a >= cells || b >= cells) {
      ++*dropped;
      continue;
    }
    const uint32_t ra = find(a), rb = find(b);
    if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
  }
  for (size_t t = 0; t < 2 * m; ++t)
    if (copies[t] < cells && copies[t ^ 1] < cells) keys.push_back(perm_key(find(copies[t]), copies[t]));
  std::sort(keys.begin(), keys.end());
  for (size_t p = 0; p < keys.size(); ++p) {
    uint32_t cell, target;
    if (perm_link(keys[p], p + 1 < keys.size() ? keys[p + 1] : PERM_PAD, cell, target)) sigma_cells[cell] = target;
  }
  return 0;
}

// The witness checker's rules (mock_check.h): found[i] / at[i] = whether and where (lower bound) keys[i] lies in `sorted` (n ascending
// 256-bit keys); the canonical key of Montgomery words as graph_check_kernel makes it of a lane's value (conversion, reduction, one
// product); a record packed and taken apart again.
int hc_mock_key_search(const uint32_t* sorted, uint64_t n, const uint32_t* keys, size_t count, uint8_t* found, uint64_t* at) {
  for (size_t i = 0; i < count; ++i) {
    found[i] = mock_key_found(sorted, n, keys + 8 * i) ? 1 : 0;
    at[i] = mock_key_lower_bound(sorted, n, keys + 8 * i);
  }
  return 0;
}
int hc_mock_value_key(const uint32_t* ext, uint32_t* key) {
  uint32_t w[8], out[8];
  std::memcpy(w, ext, sizeof w);
  const Fr x = fe_from_ext<FrParams>(w);
  mock_value_key(out, fe_reduce_small(fe_norm(x)));
  std::memcpy(key, out, sizeof out);
  return 0;
}
uint64_t hc_mock_record(uint32_t user, uint32_t index, uint32_t* user_back, uint32_t* index_back) {
  const uint64_t rec = mock_record(user, index);
  *user_back = mock_record_user(rec);
  *index_back = mock_record_index(rec);
  return rec;
}

// The pairing (pairing.inc): an Fq12 travels as 48 u64, the canonical Montgomery words of its 12 Fq in pairing.py's coefficient order,
// and stands in a slot of a one-lane workspace while the device's own functions run on it under bound tracking.
namespace {
void pf_slot_from_ext(const PfRef& d, const uint64_t* w) {
  for (uint32_t c = 0; c < 12; ++c) pf_store(d, c * 8u, load_ext<FqParams>(w + 4 * c));
}
void pf_slot_to_ext(uint64_t* w, const PfRef& a) {
  for (uint32_t c = 0; c < 12; ++c) store_ext(w + 4 * c, pf_load(a, c * 8u));
}
Fq2 f2_from_ext(const uint64_t* w) { return Fq2{load_ext<FqParams>(w), load_ext<FqParams>(w + 4)}; }
}  // namespace

// op 0: a b; 1: a^2; 2: a times the line b (only b's w^0, w^1, w^3 are read); 3: conj a; 4 / 5 / 6: a^p, a^(p^2), a^(p^3); 7: 1 / a;
// 8: a b over b's even powers (with a's odd powers zero: the Fq6 product); 9: a^x and 11: a^2 for a in the cyclotomic subgroup; 10: the
// final exponentiation of a.  -1: no such op.
int hc_f12_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  std::vector<uint32_t> ws((size_t)PF_CHECK_SLOTS * PF_WORDS, 0);
  const PfLane lane{ws.data(), 1};
  const PfRef x = lane.slot(0), y = lane.slot(1), d = lane.slot(2);
  pf_slot_from_ext(x, a);
  if (b) pf_slot_from_ext(y, b);
  PfRef r = d;
  switch (op) {
    case 0: f12_mul<false>(d, x, y); break;
    case 1: f12_mul<true>(d, x, x); break;
    case 2: f12_mul<false>(d, x, y, PF_LINE_MASK); break;
    case 3: f12_conj(x); r = x; break;
    case 4: f12_frob<1>(d, x); break;
    case 5: f12_frob<2>(d, x); break;
    case 6: f12_frob<3>(d, x); break;
    case 7: f12_inv(d, x, lane.slot(9), lane.slot(10)); break;
    case 8: f12_mul<false>(d, x, y, 0x15u); break;
    case 9: f12_pow_x(d, x, lane.slot(10)); break;
    case 10: pf_final_exponentiation(lane); r = lane.slot(PF_RESULT); break;
    case 11: f12_cyc_sqr(d, x); break;
    default: return -1;
  }
  pf_slot_to_ext(out, r);
  return 0;
}

// Fq2 on 8 u64 (c0, c1).  op 0: a b; 1: a^2; 2: 1 / a; 3: (9 + u) a; 4: a + b; 5: a - b; 6: conj a
int hc_f2_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const Fq2 x = f2_from_ext(a), y = b ? f2_from_ext(b) : f2_zero();
  Fq2 r;
  switch (op) {
    case 0: r = f2_mul(x, y); break;
    case 1: r = f2_sqr(x); break;
    case 2: r = f2_inv(x); break;
    case 3: r = f2_mul_xi(x); break;
    case 4: r = f2_add(x, y); break;
    case 5: r = f2_sub(x, y); break;
    case 6: r = f2_conj(x); break;
    default: return -1;
  }
  store_ext(out, r.c0);
  store_ext(out + 4, r.c1);
  return 0;
}

// the compiled-in constants: 36 Frobenius factors (map n = 1 .. 3, power k = 0 .. 5, component c0 / c1), then b' of the twist: 38 x 4 u64
void hc_pairing_constants(uint64_t* out) {
  for (int i = 0; i < 36; ++i) store_ext(out + 4 * i, fe_const<FqParams>(PairingParams::FROB[i]));
  store_ext(out + 144, fe_const<FqParams>(PairingParams::TWIST_B0));
  store_ext(out + 148, fe_const<FqParams>(PairingParams::TWIST_B1));
}

// One whole check on host memory by the lane functions of the two kernels, in the kernels' layout (lane-minor, stride n_pairs):
// g1 n_pairs x 8 u64, g2 n_pairs x 16 u64 -> the status (0 / 1 / 2) and the GT value (48 u64).
int hc_pairing_product(const uint64_t* g1, const uint64_t* g2, size_t n_pairs, uint64_t* gt) {
  std::vector<uint32_t> pair_ws((size_t)PF_PAIR_SLOTS * PF_WORDS * (n_pairs + 1), 0), flags(n_pairs + 1, 0);
  std::vector<uint32_t> check_ws((size_t)PF_CHECK_SLOTS * PF_WORDS, 0);
  for (size_t i = 0; i < n_pairs; ++i) {
    uint32_t p[16], q[32];
    std::memcpy(p, g1 + 8 * i, sizeof p);
    std::memcpy(q, g2 + 16 * i, sizeof q);
    flags[i] = pf_miller_lane(p, q, PfLane{pair_ws.data() + i, n_pairs});
  }
  uint32_t w[PF_WORDS];
  const uint32_t status = pf_finish_lane(0, n_pairs, n_pairs, PfLane{pair_ws.data(), n_pairs}, flags.data(), PfLane{check_ws.data(), 1}, w);
  std::memcpy(gt, w, sizeof w);
  return (int)status;
}

// The MSM's host side (msm_plan.inc).  knobs: window override, then the three switches (-1 unset, 0, 1).
namespace {
MsmKnobs msm_knobs_from(const int64_t* k) {
  MsmKnobs r;
  r.window_override = (int)k[0];
  r.digits_count = (int)k[1];
  r.k3b_copy = (int)k[2];
  r.k4_wave_sums = (int)k[3];
  return r;
}
}  // namespace

// out[0] = msm_window, out[1] = the five-launch chain's window (0: it does not apply), out[2] = msm_precomp_window(n),
// out[3] = msm_table_group_max(n, precomp_c)
void hc_msm_window(uint64_t n, uint32_t precomp_c, uint64_t live_rows, const int64_t* knobs, uint64_t* out) {
  const MsmKnobs k = msm_knobs_from(knobs);
  out[0] = msm_window((size_t)n, precomp_c, (size_t)live_rows, k);
  out[1] = plan_small_window((size_t)n, precomp_c, (size_t)live_rows, k);
  out[2] = plan_precomp_window((size_t)n);
  out[3] = plan_table_group_max((size_t)n, precomp_c);
}

// msm_plan as flat u64: HC_MSM_SCALARS scalars in the order of tests/test_msm_plan_host.py's PLAN_FIELDS, then (offset, bytes) of
// every region, then (gx, gy, block, lds, lds_cap) of every launch.  Returns the plan's error code.
int hc_msm_plan(uint64_t n, uint32_t group, uint32_t precomp_c, const int64_t* knobs, uint64_t* out, uint32_t* counts) {
  const MsmPlan p = msm_plan((size_t)n, group, precomp_c, msm_knobs_from(knobs));
  const uint64_t scalars[] = {
      (uint64_t)p.route, p.single_set, p.group, p.c, p.W, p.n_wide, p.SW, p.sn, p.NB, p.NBP, p.NBT, p.pairs_max, p.L, p.G, p.chunk, p.T_max,
      p.SEG, p.nseg, p.k4_m, p.k4_h, p.RW, p.res_stride, p.ib, p.fb, p.cb, p.NC, p.ps_G, p.ps_gpc, p.ps_nsc, p.sbits, p.br_big, p.br_slice,
      p.br_capacity, p.coop_sort, p.direct_buckets, (uint64_t)p.digits, (uint64_t)p.first_level, (uint64_t)p.p1_scatter,
      (uint64_t)p.p2_scatter, (uint64_t)p.item, (uint64_t)p.tasks, (uint64_t)p.reduction, p.sum_levels, p.sum_count[0], p.sum_count[1],
      0, 0, p.region[MR_RES].bytes, p.ws_bytes};      // (two retired columns: the levels of segment sums a plan never had)
  const uint32_t ns = (uint32_t)(sizeof scalars / sizeof scalars[0]);
  counts[0] = ns, counts[1] = MR_COUNT, counts[2] = ML_COUNT + 2;
  uint64_t* o = out;
  for (uint32_t i = 0; i < ns; ++i) *o++ = scalars[i];
  for (uint32_t r = 0; r < MR_COUNT; ++r) *o++ = p.region[r].off, *o++ = p.region[r].bytes;
  for (uint32_t l = 0; l < ML_COUNT; ++l) {
    if (l == ML_TO_EXT)      // the rows keep the two launch slots of those levels, never made
      for (int k = 0; k < 2; ++k) *o++ = 0, *o++ = 1, *o++ = 0, *o++ = 0, *o++ = MSM_LDS_DEFAULT;
    const MsmLaunch& q = p.launch[l];
    *o++ = q.gx, *o++ = q.gy, *o++ = q.block, *o++ = q.lds, *o++ = q.lds_cap;
  }
  return p.err;
}

// msm_small_plan the same way: scalars in the order of SMALL_FIELDS, the regions, then (gx, gy, gz) of the five launches
int hc_msm_small_plan(uint64_t n, uint32_t group, uint32_t c, uint64_t* out, uint32_t* counts) {
  const MsmSmallPlan p = msm_small_plan((size_t)n, group, c);
  const uint64_t scalars[] = {p.group, p.W,   p.wide, p.n_wide, p.NB,    p.pairs_max, p.H,         p.NBh,        p.V,        p.L,
                              p.SEG,   p.nseg, p.G1n,  p.T_max,  p.ws_stride, p.res_stride, p.ws_bytes, p.launch[MSL_SORT].lds, p.launch[MSL_SORT].lds_cap};
  const uint32_t ns = (uint32_t)(sizeof scalars / sizeof scalars[0]);
  counts[0] = ns, counts[1] = MSR_COUNT, counts[2] = MSL_COUNT;
  uint64_t* o = out;
  for (uint32_t i = 0; i < ns; ++i) *o++ = scalars[i];
  for (uint32_t r = 0; r < MSR_COUNT; ++r) *o++ = p.region[r].off, *o++ = p.region[r].bytes;
  for (uint32_t l = 0; l < MSL_COUNT; ++l) *o++ = p.launch[l].gx, *o++ = p.launch[l].gy, *o++ = p.launch[l].gz;
  return p.err;
}

// the constants the plan shares with the kernels, for the test's own formulas
void hc_msm_constants(uint64_t* out) {
  const uint64_t v[] = {PT_WORDS, ACC_THREADS, WIN_THREADS, TARGET_TASKS, SORT_THREADS, P1_IPT_DEFAULT, P1_BIG_IPT, P2_TILE, PS_MAX_SC, SCAN_BLOCK,
                        TASK_KEYS, FINALIZE_SERIAL, FINALIZE_SLICE, SUM_SPAN, SA_THREADS, S_TASK_KEYS, S_MAX_L, MSM_GROUP_MAX, MSM_LDS_DEFAULT,
                        MSM_LDS_FINE, MSM_LDS_ALL};
  for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
}

}  // extern "C"
