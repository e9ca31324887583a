// g1_mul.h -- the double-and-add product of a G1 point by a 256-bit integer, shared by the units that multiply single points:
// g1_mul_words (g1_fft.hip: the butterflies' twiddles, the store kernel's scale, the FK20 table products) and its field-by-field
// twin g1_mul_words_by_field (verify.hip: the per-proof sums).  Host-callable, so that host_check.cpp can run them with the bound
// tracking on.
#pragma once
#include "g1.h"

namespace hm {

// [e] b for a 256-bit integer e (8 words, little-endian), left to right; leading zero bits cost a flag test each
HM_HD G1Jac g1_mul_words(const G1Jac& b, const uint32_t (&e_in)[8]) {
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = e_in[k];
  G1Jac acc = g1_identity();
  for (int bit = 0; bit < 256; ++bit) {
    acc = g1_double(acc);
    if (e[7] >> 31) acc = g1_add(acc, b);
#pragma unroll
    for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
    e[0] <<= 1;
  }
  return acc;
}

// d <- s field by field
HM_HD void g1_assign(G1Jac& d, const G1Jac& s) {
  d.x = s.x;
  d.y = s.y;
  d.z = s.z;
  d.inf = s.inf;
}

// The same product, limb for limb, for a kernel that has to stay free of scratch.  g1_mul_words assigns whole G1Jac values
// (acc = g1_double(acc)), the three padding bytes behind the flag with them; around its loop those copies form a cycle between two
// stack slots that the compiler drops in g1_fft.hip's kernels and keeps in verify_sums_kernel (12 bytes of scratch per lane, read
// from -Rpass-analysis and the IR).  Here the accumulator is assigned field by field, so no padding byte is ever copied into it.
HM_HD G1Jac g1_mul_words_by_field(const G1Jac& b, const uint32_t (&e_in)[8]) {
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = e_in[k];
  G1Jac acc = g1_identity();
  for (int bit = 0; bit < 256; ++bit) {
    if (!acc.inf) g1_assign(acc, g1_double_nz(acc));
    if (e[7] >> 31) g1_assign(acc, g1_add(acc, b));
#pragma unroll
    for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
    e[0] <<= 1;
  }
  return acc;
}

}  // namespace hm
