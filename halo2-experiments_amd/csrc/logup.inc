// logup.inc -- the per-lane functions of the logUp lookup argument (DESIGN.md section 33): the multiplicity column m and the running
// sum phi.  Included after poseidon.inc (Fr, ps_get_words / ps_put_words), range.inc (range_plain) and sorted.inc (sorted_sub_mod,
// sorted_const_words) by logup.hip, which holds the kernels and their drivers, and by host_check.cpp, which runs the same functions
// under -DHM_BOUNDS (hc_logup_multiplicities, hc_grand_sum).
//
// Everything here works on the columns' own memory format, canonical Montgomery words: the form is linear, so a sum of Montgomery
// words mod r is the Montgomery form of the sum, and an addition is eight adds with carry and a subtraction of r under a mask.  Every
// sum is reduced as it is formed: no lazy limb ever exists, which is the whole bound argument of the scan.  A value leaves Montgomery
// form (range_plain, one product) only where it is a KEY: a table value or an input value that is counted or searched.

// every live table key below 2^LU_COUNT_BITS: the multiplicities are counted in value bins (lookup.hip's LK_COUNT_BITS, the same choice)
constexpr uint32_t LU_COUNT_BITS = 20;
constexpr uint32_t LU_NO_ROW = 0xFFFFFFFFu;                 // a bin that no table row holds

struct LuFr {
  uint32_t l[9];
};

// a = a + b mod r on canonical words: a + b < 2 r < 2^255, so the sum has no carry out; r comes off when the sum reaches it
HM_HD void lu_add_mod(uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t mod[8], s[8], d[8];
  sorted_const_words(FrParams::MOD, mod);
  uint64_t carry = 0;
  int64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    carry += (uint64_t)a[i] + b[i];
    s[i] = (uint32_t)carry;
    carry >>= 32;
    borrow += (int64_t)s[i] - (int64_t)mod[i];
    d[i] = (uint32_t)borrow;
    borrow >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = borrow ? s[i] : d[i];
}

// the key of a value: its plain integer; -> it lies below nbins (a power of two at most 2^LU_COUNT_BITS), and then key[0] is its bin
HM_HD bool lu_key(const uint32_t* value, uint32_t nbins, uint32_t (&key)[8]) {
  uint32_t w[8];
  ps_get_words(value, w);
  range_plain(w, key);
  uint32_t high = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i) high |= key[i];
  return high == 0 && key[0] < nbins;
}

// a count below 2^32 -> its canonical Montgomery words: the integer times `to_mont`, the constant lookup.hip's lk_fill_kernel
// brings its keys back with (the element 2^256 in internal form)
HM_HD void lu_count_ext(uint32_t count, const LuFr& to_mont, uint32_t (&w)[8]) {
  const uint32_t raw[8] = {count, 0, 0, 0, 0, 0, 0, 0};
  Fr cc;
#pragma unroll
  for (int j = 0; j < 9; ++j) cc.l[j] = to_mont.l[j];
  HM_DECLARE(cc, 1.0);
  fe_pack(w, fe_canonical(fe_mul(fe_unpack<FrParams>(raw), cc)));
}

// the first record of `keys` (n ascending 8-word keys, equal keys by ascending row) that holds `key`, or n
HM_HD uint64_t lu_find(const uint32_t* keys, uint64_t n, const uint32_t (&key)[8]) {
  const uint64_t at = mock_key_lower_bound(keys, n, key);
  return at < n && mock_key_cmp(keys + at * 8, key) == 0 ? at : n;
}

// rows a workgroup of the scan covers, one per lane
constexpr uint32_t LU_SCAN_ROWS = 256;
