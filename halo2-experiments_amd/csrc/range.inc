// range.inc -- the witness of the OverflowCheckV2 range-check circuit (circuits.overflow_check_v2, synthesis.RangeCheckLayout;
// DESIGN.md section 25).  Included after poseidon.inc (Fr, ps_get_words / ps_put_words) by range.hip, which holds the kernel and its
// driver, and by host_check.cpp, which runs the same lane function under -DHM_BOUNDS.
//
// Column 0 of a circuit is the value as given, columns 1 .. acc_cols its limbs of max_bits bits, most significant first; one lane
// per (circuit, row) writes its row of every column, 32 bytes per column: a wave's 64 rows are 2 KiB contiguous in each column.
// The value comes out of Montgomery form once (one product by the plain integer 32: w * 32 * 2^-261 = w * 2^-256); the limbs are cut
// from the low words of that integer, which is then shifted down by max_bits -- no register is indexed by a runtime number, so
// nothing goes to scratch; a limb l < 2^16 goes back into Montgomery form as l * (2^256 mod r) - q * r with q from one 32-bit
// multiply (range_limb_ext): 18 narrow multiply-adds against the 162 of a Montgomery product.  A 2^max_bits-entry LDS table of the
// limbs' Montgomery forms would be 2 MiB at max_bits = 16, the shape the solvency statement uses, so there is none.

constexpr uint32_t RANGE_MAX_BITS = 16, RANGE_MAX_VALUE_BITS = 253;

struct RangeArgs {
  const uint32_t* values;   // m x rows x 8 words, canonical Montgomery
  uint32_t* advice;         // m x (1 + acc_cols) x 2^log_n x 8 words, every word written
  uint32_t* over;           // m counters, zeroed by the caller; or null
  uint64_t lanes;           // m << log_n
  uint32_t max_bits, acc_cols, log_n, rows;
};

// the plain integer of a canonical Montgomery element, as 8 x 32-bit words
HM_HD void range_plain(const uint32_t (&w)[8], uint32_t (&p)[8]) {
  Fr c = fe_zero<FrParams>();
  c.l[0] = 32u;
#ifdef HM_BOUNDS
  set_bounds(c, 1.0, 32, 0);
#endif
  fe_pack(p, fe_canonical(fe_mul(fe_unpack<FrParams>(w), c)));   // the constant is the scanned operand: its zero limbs fold away
}

// l < 2^16 -> the canonical Montgomery words of l: l * INT2EXT - q * MOD, q = floor(l * INT2EXT / MOD) or one less (EXTQ32 is the
// ratio rounded down to 32 fractional bits: the estimate is short by less than l * 2^-32 < 2^-16), so the difference is below 2 MOD
HM_HD void range_limb_ext(uint32_t l, uint32_t (&w)[8]) {
#ifdef HM_BOUNDS
  HM_CHECK(l < (1u << RANGE_MAX_BITS), "range_limb_ext: the limb must be below 2^16");
#endif
  const uint32_t q = (uint32_t)(((uint64_t)l * FrParams::EXTQ32) >> 32);
  Fr r;
  int64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t t = (int64_t)((uint64_t)l * FrParams::INT2EXT[i]) - (int64_t)((uint64_t)q * FrParams::MOD[i]) + carry;
    r.l[i] = (uint32_t)t & MASK29;
    carry = t >> 29;
  }
  r.l[8] = (uint32_t)((int64_t)((uint64_t)l * FrParams::INT2EXT[8]) - (int64_t)((uint64_t)q * FrParams::MOD[8]) + carry);
#ifdef HM_BOUNDS
  set_bounds(r, 2.0, MASK29, top_bound_from_value<FrParams>(2.0));
  HM_CHECK(r.l[8] <= r.tb, "range_limb_ext result exceeds 2 MOD");
#endif
  fe_pack(w, fe_canonical(r));
}

// row (idx mod 2^log_n) of circuit (idx >> log_n); -> the value has bits at or above max_bits * acc_cols
HM_HD bool range_witness_lane(const RangeArgs& a, uint64_t idx) {
  const uint64_t c = idx >> a.log_n, row = idx & (((uint64_t)1 << a.log_n) - 1);
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* out = a.advice + c * (1 + a.acc_cols) * col_words + row * 8;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row >= a.rows) {
    for (uint32_t j = 0; j <= a.acc_cols; ++j) ps_put_words(out + j * col_words, w);
    return false;
  }
  ps_get_words(a.values + (c * a.rows + row) * 8, w);
  ps_put_words(out, w);
  uint32_t p[8], lw[8];
  range_plain(w, p);
  const uint32_t b = a.max_bits, mask = (1u << b) - 1u;
  for (uint32_t j = a.acc_cols; j >= 1; --j) {             // the least significant limb is the last column
    range_limb_ext(p[0] & mask, lw);
    ps_put_words(out + j * col_words, lw);
#pragma unroll
    for (int i = 0; i < 7; ++i) p[i] = (p[i] >> b) | (p[i + 1] << (32 - b));      // 1 <= b <= 16
    p[7] >>= b;
  }
  uint32_t rest = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) rest |= p[i];
  return rest != 0;
}
