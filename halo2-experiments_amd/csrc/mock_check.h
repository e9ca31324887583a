// mock_check.h -- the rules of the witness checker (mock.hip) that the host states too (host_check.cpp: hc_mock_key_search, hc_mock_value_key,
// hc_mock_record; tests/test_mock_prover.py): how a value becomes a key, how a key is searched in the sorted table keys, and how
// a failure is packed into a record.
#pragma once
#include <stdint.h>

#include "ff29.h"
#include "g1.h"

namespace hm {

// -1 / 0 / +1 as a < / == / > b for 256-bit keys of eight little-endian words (the top word decides first): the order lookup.hip's
// key_cmp sorts by
HM_HD int mock_key_cmp(const uint32_t* a, const uint32_t* b) {
  for (int k = 7; k >= 0; --k) {
    if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
  }
  return 0;
}

// the first position of `sorted` (n keys, ascending) whose key is not below `key`: n when every key is below it
HM_HD uint64_t mock_key_lower_bound(const uint32_t* sorted, uint64_t n, const uint32_t* key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (mock_key_cmp(sorted + mid * 8, key) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
HM_HD bool mock_key_found(const uint32_t* sorted, uint64_t n, const uint32_t* key) {
  const uint64_t at = mock_key_lower_bound(sorted, n, key);
  return at < n && mock_key_cmp(sorted + at * 8, key) == 0;
}

// the canonical integer of a value held in the evaluator's internal form (normalised, < 3r), as the eight words the table keys are:
// the internal form is 32 * 2^256 * value and a product divides by 2^261, so the product with the INTEGER 1 is the value itself
// (lk_convert_kernel multiplies raw Montgomery words, 2^256 * value, by the integer 32 to the same end)
HM_HD void mock_value_key(uint32_t (&key)[8], const Fr& reduced) {
  Fr one = fe_zero<FrParams>();
  one.l[0] = 1u;
  HM_DECLARE(one, 1.0);
  fe_pack(key, fe_canonical(fe_mul(reduced, one)));
}

// a failure: (user, row) of a gate or lookup, (user, copy index) of a copy -- records sort by user first
HM_HD uint64_t mock_record(uint32_t user, uint32_t index) { return ((uint64_t)user << 32) | index; }
HM_HD uint32_t mock_record_user(uint64_t rec) { return (uint32_t)(rec >> 32); }
HM_HD uint32_t mock_record_index(uint64_t rec) { return (uint32_t)rec; }

}  // namespace hm
