// shplonk.inc -- the set quotient of the SHPLONK multiopen (DESIGN.md section 17): for one rotation set with the distinct points
// p_1..p_t and the combined polynomial N(X) = sum_j w_j P_j(X),
//     out (+)= scale * (N - R) / Z_S,      Z_S = prod_l (X - p_l),  deg R < t,  R(p_l) = N(p_l),
// which upstream (poly/kzg/multiopen/shplonk/prover.rs) reaches by interpolating R, subtracting it and dividing t times.  For distinct
// points
//     (N - R) / Z_S = sum_l c_l * kate(N, p_l),      c_l = 1 / prod_{l' != l} (p_l - p_l'),
// where kate(N, p) is kate_division (the remainder dropped): the partial fractions of 1 / Z_S.  So the t divisions are t independent
// first-order suffix scans over the SAME input -- the scans of fr_kate_chunks / _join / _replay_kernel with t multipliers per lane -- and
// neither R nor an evaluation nor an intermediate quotient is ever formed.  The sum has degree n - 1 - t: rows n - t .. n - 1 are zero.
// The final division of the multiopen by (X - u) is the case t = 1, c_1 = 1.
//
// The host-testable parts -- the limit on t, the plan, the coefficients d_l = scale * c_l, the row formula -- stand here and
// host_check.cpp runs them; the kernels are in polyops.hip.  Included inside namespace hm, after ff29.h and host_fr.h.
constexpr int SHQ_T_MAX = 4;                 // HM_SHPLONK_MAX_POINTS of the header
constexpr uint32_t SHQ_THREADS = 256;        // = PO_THREADS: the scans share polyops.hip's workgroup
constexpr uint32_t SHQ_MAX_LANES = 65536;    // = PO_MAX_LANES: one joining workgroup

// Lane L owns rows [L B, (L + 1) B); G workgroups of 256 lanes.  The rule of polyops.hip's po_plan, stated once more for the host.
struct ShqPlan {
  uint32_t B, G;
  uint64_t lanes;
};
HM_HD ShqPlan shq_plan(uint64_t n) {
  ShqPlan p;
  p.B = (uint32_t)((n + SHQ_MAX_LANES - 1) / SHQ_MAX_LANES);
  if (p.B < 4) p.B = n >= 4 ? 4 : 1;
  p.lanes = (n + p.B - 1) / p.B;
  p.G = (uint32_t)((p.lanes + SHQ_THREADS - 1) / SHQ_THREADS);
  return p;
}

// words of a scan's scratch per point: the inclusive values of G * 256 lanes and a guard lane, G workgroup totals, G carries
HM_HD uint64_t shq_scan_words(const ShqPlan& p) { return ((uint64_t)p.G * SHQ_THREADS + 1 + 2 * (uint64_t)p.G) * 9; }

inline bool shq_fr_canonical(const host::Fr4& a) {
  for (int i = 3; i >= 0; --i)
    if (a.l[i] != host::FR_MOD[i]) return a.l[i] < host::FR_MOD[i];
  return false;
}

// d_l = scale / prod_{l' != l} (p_l - p_l') in external Montgomery words; false when t is out of range, a word is not canonical or two
// points are equal (the set has no quotient then)
inline bool shq_coefficients(uint32_t t, const host::Fr4* pts, const host::Fr4& scale, host::Fr4* d) {
  if (t == 0 || t > (uint32_t)SHQ_T_MAX || !shq_fr_canonical(scale)) return false;
  for (uint32_t l = 0; l < t; ++l)
    if (!shq_fr_canonical(pts[l])) return false;
  for (uint32_t l = 0; l < t; ++l) {
    host::Fr4 den = host::FR_ONE;
    for (uint32_t k = 0; k < t; ++k) {
      if (k == l) continue;
      const host::Fr4 diff = host::fr_sub(pts[l], pts[k]);
      if (host::fr_is_zero(diff)) return false;
      den = host::fr_mul(den, diff);
    }
    d[l] = host::fr_mul(scale, host::fr_inv(den));
  }
  return true;
}

// One output row: sum_l d_l * q_l (+ the row's old raw words).  q_l: the quotients' running values (< 3r, "external read as
// internal"), d_l: true internal -> a canonical-ready value < 3r.  At most four products below 2r and one raw word pattern.
template <int T>
HM_HD Fe<FrParams> shq_row(const Fe<FrParams> (&q)[T], const Fe<FrParams> (&d)[T], bool accumulate, const Fe<FrParams>& old_raw) {
  Fe<FrParams> s = fe_mul(q[0], d[0]);
#pragma unroll
  for (int l = 1; l < T; ++l) s = fe_add(s, fe_mul(q[l], d[l]));
  if (accumulate) s = fe_add(s, old_raw);
  return fe_reduce_small(fe_norm(s));
}
