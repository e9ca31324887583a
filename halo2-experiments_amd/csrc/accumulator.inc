// accumulator.inc -- the witness of the SafeAccumulator circuit (circuits.safe_accumulator, synthesis.SafeAccumulatorLayout; DESIGN.md
// section 26).  Included after poseidon.inc (ps_get_words / ps_put_words) and range.inc (range_plain, range_limb_ext) by
// accumulator.hip, which holds the kernels and their driver, and by host_check.cpp, which runs the same functions under -DHM_BOUNDS.
//
// The running total of a circuit is `acc_cols` limbs of `max_bits` bits, W = max_bits * acc_cols <= 64 bits in all, so the state
// after row r is one wrapping 64-bit integer: S_r = (S_0 + v_1 + ... + v_r) mod 2^W, a prefix sum.  Row 0 of the table holds the limbs
// of the initial state as given; the lane of row r, 1 <= r <= rows, owns (S_{r-1}, v_r) and writes its whole row from them:
//   column 0            the value as given
//   column 1            the inverse of the top limb of S_r (0 when that limb is 0), from a table of the 2^max_bits - 1 inverses
//   columns 2 .. 1+A    the carries: c[A-1] = (prev[A-1] + v_r >= 2^b), c[i] = (prev[i] + c[i+1] >= 2^b), c[0] = 0
//   columns 2+A .. 1+2A the limbs of S_r, most significant first
// The limbs of both states are peeled off the low end of two integers that are shifted down by max_bits a column (never by W, which
// may be 64), so no register is indexed by a runtime number.  Nothing is judged: a value at or above 2^b, or a total that reaches
// the top limb, gives a row that fails its gate, and the lane reports it.

constexpr uint32_t ACC_MAX_BITS = 4, ACC_MAX_WIDTH = 64;

struct AccArgs {
  const uint32_t* values;     // m x rows x 8 words, canonical Montgomery
  const uint64_t* initial;    // m x acc_cols plain limb integers, most significant first
  const uint32_t* inverses;   // (2^max_bits - 1) x 8 words: entry j the Montgomery words of (j + 1)^-1
  uint32_t* advice;           // m x (2 + 2 acc_cols) x 2^log_n x 8 words, every word written
  uint64_t* finals;           // m x acc_cols: the plain limbs of S_rows
  uint32_t max_bits, acc_cols, log_n, rows;
};

HM_HD uint64_t acc_width_mask(uint32_t width) { return width >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << width) - 1); }

// the low 64 bits of a value's plain integer, and whether the integer is at or above 2^max_bits
HM_HD uint64_t acc_value_low(const uint32_t (&w)[8], uint32_t max_bits, bool& big) {
  uint32_t p[8];
  range_plain(w, p);
  uint32_t high = p[0] >> max_bits;
#pragma unroll
  for (int i = 1; i < 8; ++i) high |= p[i];
  big = high != 0;
  return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
}

// x < 2^64 -> the canonical Montgomery words of x, by doubling and adding 2^256 mod r over plain 32-bit words: the limbs of the
// initial state are whatever the caller passes, not only what range_limb_ext takes.  A circuit runs this acc_cols times.
HM_HD void acc_mont_u64(uint64_t x, uint32_t (&w)[8]) {
  uint32_t mod[8], one[8];
  fe_pack(mod, fe_const<FrParams>(FrParams::MOD));
  fe_pack(one, fe_const<FrParams>(FrParams::INT2EXT));
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0;
  for (int bit = 63; bit >= 0; --bit) {
    for (int step = 0; step < 2; ++step) {                  // w <- 2 w, then w <- w + one where the bit is set; both below 2 r < 2^255
      if (step == 1 && !((x >> bit) & 1)) break;
      uint32_t s[8], d[8];
      uint64_t carry = 0;
      int64_t borrow = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        carry += (uint64_t)w[i] + (step ? one[i] : w[i]);
        s[i] = (uint32_t)carry;
        carry >>= 32;
        borrow += (int64_t)s[i] - (int64_t)mod[i];
        d[i] = (uint32_t)borrow;
        borrow >>= 32;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = borrow ? s[i] : d[i];
    }
  }
}

// the initial state of circuit c as one integer below 2^W; -> a limb is at or above 2^max_bits, or the top limb is not zero
HM_HD bool acc_initial_state(const AccArgs& a, uint64_t c, uint64_t& s0) {
  const uint64_t* lim = a.initial + c * a.acc_cols;
  bool bad = lim[0] != 0;
  uint64_t s = 0;
  for (uint32_t i = 0; i < a.acc_cols; ++i) {               // Horner from the top: the shifts are by max_bits, never by W
    s = (s << a.max_bits) + lim[i];
    bad = bad || (lim[i] >> a.max_bits) != 0;
  }
  s0 = s & acc_width_mask(a.max_bits * a.acc_cols);
  return bad;
}

// row 0 of accumulate column i of circuit c: the initial limb as given
HM_HD void acc_initial_cell(const AccArgs& a, uint64_t c, uint32_t i) {
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t w[8];
  acc_mont_u64(a.initial[c * a.acc_cols + i], w);
  ps_put_words(a.advice + (c * (2 + 2 * (uint64_t)a.acc_cols) + 2 + a.acc_cols + i) * col_words, w);
}

// Row `row` >= 1 of a circuit from (S_{row-1}, the value's words): `out` is word 0 of column 0 on that row.  Leaves S_row in s_new.
// -> the value is at or above 2^max_bits, or the top limb of S_row is not zero
HM_HD bool accumulator_row(const AccArgs& a, uint32_t* out, uint64_t s_prev, const uint32_t (&w)[8], uint64_t& s_new) {
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  const uint32_t b = a.max_bits, A = a.acc_cols;
  const uint64_t mask = ((uint64_t)1 << b) - 1, wmask = acc_width_mask(b * A);
  bool big;
  const uint64_t v = acc_value_low(w, b, big) & wmask;
  ps_put_words(out, w);
  s_new = (s_prev + v) & wmask;
  uint64_t sp = s_prev, sn = s_new;
  uint32_t carry = ((v >> b) != 0 || (((v & mask) + (sp & mask)) >> b) != 0) ? 1u : 0u, top = 0;
  uint32_t lw[8];
  for (uint32_t j = A - 1;; --j) {                          // the least significant limb is the last column
    if (j == 0) carry = 0;                                  // the reference's `idx > 0`
    else if (j != A - 1) carry = (uint32_t)(((sp & mask) + carry) >> b);
    range_limb_ext(carry, lw);
    ps_put_words(out + (2 + j) * col_words, lw);
    top = (uint32_t)(sn & mask);
    range_limb_ext(top, lw);
    ps_put_words(out + (2 + A + j) * col_words, lw);
    if (j == 0) break;
    sp >>= b;
    sn >>= b;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) lw[i] = 0;
  if (top) ps_get_words(a.inverses + (uint64_t)(top - 1) * 8, lw);      // 0 < top < 2^max_bits
  ps_put_words(out + col_words, lw);
  return big || top != 0;
}

// the limbs of the final state
HM_HD void acc_write_finals(const AccArgs& a, uint64_t c, uint64_t s) {
  const uint64_t mask = ((uint64_t)1 << a.max_bits) - 1;
  for (uint32_t i = a.acc_cols; i-- > 0;) {
    a.finals[c * a.acc_cols + i] = s & mask;
    s >>= a.max_bits;
  }
}

// `count` zero cells from column `first` on, on the row `out` is word 0 of column 0 of
HM_HD void acc_zero_cells(uint32_t* out, uint64_t col_words, uint32_t first, uint32_t count) {
  const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t j = first; j < first + count; ++j) ps_put_words(out + j * col_words, z);
}
