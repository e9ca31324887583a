// fq_inverse.h -- the Fermat inversion in Fq that ends every Jacobian -> affine normalisation on the device (msm.hip: the fixed-base
// tables and products; g1_fft.hip: the store kernel; verify.hip: the per-proof sums).  Host-callable for host_check.cpp.
#pragma once
#include "g1.h"

namespace hm {

HM_HD Fq fq_inverse(const Fq& a) {  // a^(p-2), a a product output
  // exponent p - 2 in 29-bit limbs
  uint32_t e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) e[i] = FqParams::MOD[i];
  e[0] -= 2;  // MOD[0] is odd and > 2: no borrow
  Fq acc = fe_one<FqParams>();
  for (int i = 8; i >= 0; --i) {
    const int top = i == 8 ? 24 : 28;
    for (int bit = top; bit >= 0; --bit) {
      acc = fe_sqr(acc);
      if ((e[i] >> bit) & 1) acc = fe_mul(acc, a);
    }
  }
  return acc;
}

}  // namespace hm
