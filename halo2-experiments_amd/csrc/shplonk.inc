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
// The host-testable parts -- the limit on t, the plan, the coefficients d_l = scale * c_l, the row formula -- stand here outside the
// HIP-only block; host_check.cpp runs them.  Included inside namespace hm, after ff29.h and host_fr.h.
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

#if defined(__HIPCC__)
// f(integral_constant<l>) for l = 0 .. T - 1, spelled out: the per-point state lives in arrays that must stay in registers, and the
// loops around a workgroup scan or a square-and-multiply are not unrolled by the pragma
template <int I, int T, class F>
__device__ __forceinline__ void shq_each(F&& f) {
  if constexpr (I < T) {
    f(std::integral_constant<int, I>{});
    shq_each<I + 1, T>(f);
  }
}

struct ShqArgs {
  PoFr z[SHQ_T_MAX];       // the points, true internal form
  PoFr d[SHQ_T_MAX];       // scale * c_l, true internal form
};

// S_L of every point from ONE read of the lane's chunk, then one workgroup scan per point (the LDS planes are reused: the scan's last
// barrier follows its last read).  Scratch of point l: incl + l * (G * 256 + 1) * 9, wg_total + l * G * 9 -- the layout
// fr_kate_join_kernel expects of its columns.
template <int T>
__device__ __forceinline__ void shq_chunks_body(uint32_t* lds, const uint32_t* __restrict__ a, uint64_t n, const ShqArgs& args, uint32_t B,
                                                uint32_t* __restrict__ incl, uint32_t* __restrict__ wg_total) {
  const uint32_t t = threadIdx.x;
  const uint64_t L = (uint64_t)blockIdx.x * PO_THREADS + t;
  const uint64_t lo = L * B, hi = lo + B < n ? lo + B : n;
  Fr z[T], acc[T];
#pragma unroll
  for (int l = 0; l < T; ++l) {
    z[l] = po_arg(args.z[l]);
    acc[l] = fe_zero<FrParams>();
    HM_DECLARE(acc[l], 0.0);
  }
  for (uint64_t j = hi; j > lo; --j) {
    const Fr raw = po_load_raw(a, j - 1);
#pragma unroll
    for (int l = 0; l < T; ++l) acc[l] = fe_add(fe_mul(acc[l], z[l]), raw);
  }
  const size_t lanes = (size_t)gridDim.x * PO_THREADS + 1;
  shq_each<0, T>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    Fr s = fe_reduce_small(fe_norm(acc[l]));
    s = po_suffix_scan_uniform(lds, s, po_pow_small(z[l], B));
    po_store9(incl + ((size_t)l * lanes + L) * 9, s);
    if (t == 0) po_store9(wg_total + ((size_t)l * gridDim.x + blockIdx.x) * 9, s);
  });
}
template <int T>
__global__ __launch_bounds__(PO_THREADS) void fr_shq_chunks_kernel(const uint32_t* __restrict__ a, uint64_t n, ShqArgs args, uint32_t B,
                                                                   uint32_t* __restrict__ incl, uint32_t* __restrict__ wg_total) {
  __shared__ uint32_t lds[9 * PO_THREADS];
  shq_chunks_body<T>(lds, a, n, args, B, incl, wg_total);
}

// Every lane replays its chunk for all T points at once and writes the combined row.  Rows at and above n - T are zero in the sum:
// written as zero, or left alone when accumulating.
template <int T>
__device__ __forceinline__ void shq_replay_body(const uint32_t* __restrict__ a, uint64_t n, const ShqArgs& args, uint32_t B,
                                                const uint32_t* __restrict__ incl, const uint32_t* __restrict__ carry,
                                                uint32_t* __restrict__ out, int accumulate) {
  const uint32_t t = threadIdx.x;
  const uint64_t L = (uint64_t)blockIdx.x * PO_THREADS + t;
  const uint64_t lo = L * B;
  if (lo >= n) return;
  const uint64_t hi = lo + B < n ? lo + B : n;
  const size_t lanes = (size_t)gridDim.x * PO_THREADS + 1;
  Fr z[T], d[T], cur[T];
  shq_each<0, T>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    z[l] = po_arg(args.z[l]);
    d[l] = po_arg(args.d[l]);
    // T_L = (inclusive value of the next lane in this workgroup) + y^(255 - t) * E_g, as in fr_kate_replay_kernel
    Fr Tl = fe_mul(po_load9(carry + ((size_t)l * gridDim.x + blockIdx.x) * 9, 3.0), po_pow_small(po_pow_small(z[l], B), PO_THREADS - 1 - t));
    if (t + 1 < PO_THREADS) Tl = fe_add(Tl, po_load9(incl + ((size_t)l * lanes + L + 1) * 9, 3.0));
    cur[l] = fe_reduce_small(fe_norm(Tl));                  // Q_l[hi - 1]
  });
  const auto emit = [&](uint64_t i) {
    if (i + T < n) {
      Fr old = fe_zero<FrParams>();
      if (accumulate) old = po_load_raw(out, i);
      po_store_canonical(out, i, shq_row<T>(cur, d, accumulate != 0, old));
    } else if (!accumulate) {
      uint4* dst = reinterpret_cast<uint4*>(out + i * 8);
      dst[0] = make_uint4(0, 0, 0, 0);
      dst[1] = make_uint4(0, 0, 0, 0);
    }
  };
  emit(hi - 1);
  for (uint64_t i = hi - 1; i > lo; --i) {                  // Q_l[i - 1] = a[i] + p_l Q_l[i]
    const Fr raw = po_load_raw(a, i);
#pragma unroll
    for (int l = 0; l < T; ++l) cur[l] = fe_reduce_small(fe_norm(fe_add(fe_mul(cur[l], z[l]), raw)));
    emit(i - 1);
  }
}
template <int T>
__global__ __launch_bounds__(PO_THREADS) void fr_shq_replay_kernel(const uint32_t* __restrict__ a, uint64_t n, ShqArgs args, uint32_t B,
                                                                   const uint32_t* __restrict__ incl, const uint32_t* __restrict__ carry,
                                                                   uint32_t* __restrict__ out, int accumulate) {
  shq_replay_body<T>(a, n, args, B, incl, carry, out, accumulate);
}

// ---- the same chain for a batch of independent proofs (hm_shplonk_set_quotient_batch_bn256_fr_dev): blockIdx.y = the proof ----
// Proof b's combined polynomial N_b is row b of `a` (n x 8 words each), its points and coefficients entry b of a device table that was
// uploaded with the call (wave-uniform: scalar loads), its scans' scratch the b-th block of `scan_stride` words (the single chain's
// layout inside: incl, wg_total, carry), its output outs[b].  The bodies are the single chain's, so are the bounds.
template <int T>
__global__ __launch_bounds__(PO_THREADS) void fr_shq_chunks_batch_kernel(const uint32_t* __restrict__ a, uint64_t n,
                                                                         const ShqArgs* __restrict__ table, uint32_t B,
                                                                         uint32_t* __restrict__ scan, uint64_t scan_stride) {
  __shared__ uint32_t lds[9 * PO_THREADS];
  const size_t b = blockIdx.y;
  uint32_t* incl = scan + b * scan_stride;
  uint32_t* wg_total = incl + (size_t)T * ((size_t)gridDim.x * PO_THREADS + 1) * 9;
  shq_chunks_body<T>(lds, a + b * n * 8, n, table[b], B, incl, wg_total);
}
template <int T>
__global__ __launch_bounds__(PO_THREADS) void fr_shq_replay_batch_kernel(const uint32_t* __restrict__ a, uint64_t n,
                                                                         const ShqArgs* __restrict__ table, uint32_t B,
                                                                         const uint32_t* __restrict__ scan, uint64_t scan_stride,
                                                                         uint32_t* const* __restrict__ outs, int accumulate) {
  const size_t b = blockIdx.y;
  const uint32_t* incl = scan + b * scan_stride;
  const uint32_t* carry = incl + (size_t)T * ((size_t)gridDim.x * PO_THREADS + 1) * 9 + (size_t)T * gridDim.x * 9;
  shq_replay_body<T>(a + b * n * 8, n, table[b], B, incl, carry, outs[b], accumulate);
}
// the joins: blockIdx.x = the point, blockIdx.y = the proof
__global__ __launch_bounds__(PO_THREADS) void fr_shq_join_batch_kernel(uint32_t* __restrict__ scan, uint64_t scan_stride, uint32_t G, uint32_t t_points,
                                                                       const ShqArgs* __restrict__ table, uint32_t B) {
  __shared__ uint32_t lds[9 * PO_THREADS];
  uint32_t* wg_total = scan + (size_t)blockIdx.y * scan_stride + (size_t)t_points * ((size_t)G * PO_THREADS + 1) * 9;
  uint32_t* carry = wg_total + (size_t)t_points * G * 9;
  po_kate_join_body(lds, wg_total + (size_t)blockIdx.x * G * 9, G, po_arg(table[blockIdx.y].z[blockIdx.x]), B, carry + (size_t)blockIdx.x * G * 9);
}
#endif
