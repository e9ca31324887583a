// sorted.inc -- the witness of the sorted-column circuit (circuits.sorted_column, synthesis.SortedColumnLayout; DESIGN.md section 32)
// and the record order of the id argsort.  Included after poseidon.inc (Fr, ps_get_words / ps_put_words) and range.inc by sorted.hip,
// which holds the kernels and their drivers, and by host_check.cpp, which runs the same lane function under -DHM_BOUNDS: the gap comes
// out of Montgomery form with range.inc's range_plain and its limbs go back with its range_limb_ext.
//
// Column 0 of a circuit is the id as given, columns 1 .. acc_cols the limbs of the gap to the NEXT row's id, gap = id[i+1] - id[i] - 1
// mod r, most significant first; one lane per (circuit, row) writes its row of every column, as range_witness_lane does.  The gap is
// formed on the canonical Montgomery words (the form is linear: two subtractions with borrow, r added back after each that wraps),
// so ONE product brings it out of Montgomery form; the limbs are cut as in range.inc, by shifts of constant distance inside unrolled
// loops -- no register is indexed by a runtime number, nothing goes to scratch, and there is no LDS.  The last live row has no next id:
// its limbs are zero, as are all rows behind it.

struct SortedArgs {
  const uint32_t* ids;      // m x rows x 8 words, canonical Montgomery
  uint32_t* advice;         // m x (1 + acc_cols) x 2^log_n x 8 words, every word written
  uint32_t* over;           // m counters, zeroed by the caller; or null
  uint64_t lanes;           // m << log_n
  uint32_t max_bits, acc_cols, log_n, rows;
};

// the 8 x 32-bit words of a constant below 2^256 given as 9 x 29-bit limbs (r itself, 2^256 mod r): folded by the compiler
HM_HD void sorted_const_words(const uint32_t (&c)[9], uint32_t (&w)[8]) {
  fe_pack(w, fe_const<FrParams>(c));
}

// a = a - b mod r on canonical words: the difference with borrow, then r added back (under a mask, not a branch) when it wrapped
HM_HD void sorted_sub_mod(uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t mod[8];
  sorted_const_words(FrParams::MOD, mod);
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a[i] - b[i] - borrow;
    a[i] = (uint32_t)t;
    borrow = (uint32_t)(t >> 63);
  }
  const uint32_t mask = 0u - borrow;
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a[i] + (mod[i] & mask) + carry;
    a[i] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}

// row (idx mod 2^log_n) of circuit (idx >> log_n); -> the gap to the next id has bits at or above max_bits * acc_cols (the ids are
// not ascending, equal, or too far apart: one verdict for all three)
HM_HD bool sorted_witness_lane(const SortedArgs& a, uint64_t idx) {
  const uint64_t c = idx >> a.log_n, row = idx & (((uint64_t)1 << a.log_n) - 1);
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* out = a.advice + c * (1 + a.acc_cols) * col_words + row * 8;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row >= a.rows) {
    for (uint32_t j = 0; j <= a.acc_cols; ++j) ps_put_words(out + j * col_words, w);
    return false;
  }
  const uint32_t* id = a.ids + (c * a.rows + row) * 8;
  ps_get_words(id, w);
  ps_put_words(out, w);
  uint32_t lw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row + 1 >= a.rows) {                                 // the last live row: no selector, zero limbs
    for (uint32_t j = 1; j <= a.acc_cols; ++j) ps_put_words(out + j * col_words, lw);
    return false;
  }
  uint32_t g[8], one[8], p[8];
  ps_get_words(id + 8, g);                                 // the next row's id, the same circuit
  sorted_const_words(FrParams::INT2EXT, one);              // 1 in Montgomery form
  sorted_sub_mod(g, w);
  sorted_sub_mod(g, one);
  range_plain(g, p);
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

// ---- the argsort's records: a 256-bit canonical integer and the 32-bit row it came from, 9 words ---------------------------------------
// a before b: by key, the top word first, then by row -- no two records of one sort are equal, so the network's result does not depend
// on its shape, and equal keys keep the order of their rows
HM_HD bool sorted_record_less(const uint32_t (&a)[9], const uint32_t (&b)[9]) {
  bool less = a[8] < b[8];                                 // word 8 is the row: it decides only when every key word agrees
#pragma unroll
  for (int k = 0; k < 8; ++k) less = a[k] != b[k] ? a[k] < b[k] : less;
  return less;
}
