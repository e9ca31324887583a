// Stand-alone check (tests/test_mont_forms_host.py builds it with -fsanitize=address,undefined, with and without
// -DHM_BOUNDS): the lockstep (product-scanning) forms of csrc/ff29.h -- fe_mul_x2, fe_mul_x3, fe_sqr_x2, fe_mul_mul2 -- and
// its single fe_mul / fe_mul2 / fe_sqr against a verbatim copy of the three operand-scanning routines, limb for limb,
// for Fq and Fr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ff29.h"

using namespace hm;

struct Limbs {
  uint32_t l[9];
};

// ---- the reference: ff29.h's three operand-scanning routines, copied (bound tracking left out) -----------------
template <class F>
static Limbs ref_mul(const uint32_t* a, const uint32_t* b) {
  uint64_t t[10];
  for (int j = 0; j < 10; ++j) t[j] = 0;
  for (int i = 0; i < 9; ++i) {
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)a[j] * b[i];
    const uint32_t m = ((uint32_t)t[0] * F::INV29) & MASK29;
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)m * F::MOD[j];
    t[1] += t[0] >> 29;
    for (int j = 0; j < 9; ++j) t[j] = t[j + 1];
    t[9] = 0;
  }
  Limbs r;
  for (int j = 0; j < 8; ++j) {
    r.l[j] = (uint32_t)t[j] & MASK29;
    t[j + 1] += t[j] >> 29;
  }
  r.l[8] = (uint32_t)t[8];
  return r;
}

template <class F>
static Limbs ref_mul2(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d) {
  uint64_t t[10];
  for (int j = 0; j < 10; ++j) t[j] = 0;
  for (int i = 0; i < 9; ++i) {
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)a[j] * b[i];
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)c[j] * d[i];
    const uint32_t m = ((uint32_t)t[0] * F::INV29) & MASK29;
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)m * F::MOD[j];
    t[1] += t[0] >> 29;
    for (int j = 0; j < 9; ++j) t[j] = t[j + 1];
    t[9] = 0;
  }
  Limbs r;
  for (int j = 0; j < 8; ++j) {
    r.l[j] = (uint32_t)t[j] & MASK29;
    t[j + 1] += t[j] >> 29;
  }
  r.l[8] = (uint32_t)t[8];
  return r;
}

template <class F>
static Limbs ref_sqr(const uint32_t* a) {
  uint32_t d[9];
  for (int j = 0; j < 9; ++j) d[j] = a[j] << 1;
  uint64_t t[10];
  for (int j = 0; j < 10; ++j) t[j] = 0;
  for (int i = 0; i < 9; ++i) {
    if (2 * i - i <= 8) t[i] += (uint64_t)a[i] * a[i];
    for (int j = i + 1; j < 9; ++j)
      if (j <= 8) t[j] += (uint64_t)a[i] * d[j];
    const uint32_t m = ((uint32_t)t[0] * F::INV29) & MASK29;
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)m * F::MOD[j];
    t[1] += t[0] >> 29;
    for (int j = 0; j < 9; ++j) t[j] = t[j + 1];
    t[9] = 0;
  }
  Limbs r;
  for (int j = 0; j < 8; ++j) {
    r.l[j] = (uint32_t)t[j] & MASK29;
    t[j + 1] += t[j] >> 29;
  }
  r.l[8] = (uint32_t)t[8];
  return r;
}

// ---- operands ---------------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// An operand with limbs 0..7 <= lb and top limb <= tb.  Its value is < (tb + ceil(lb / MASK29)) * 2^232; with bound
// tracking on, that is what it is declared at, and an operand no class could hold (that bound >= 2^261) is refused.
template <class F>
static bool make(Fe<F>& out, const uint32_t (&l)[9], uint64_t lb, uint64_t tb) {
  for (int i = 0; i < 9; ++i) out.l[i] = l[i];
#ifdef HM_BOUNDS
  const double units = (double)tb + (double)((lb + MASK29 - 1) / MASK29);
  const double vb = units * std::ldexp(1.0, 232) / mod_as_double<F>() * (1.0 + 1e-12);
  if (!(vb * mod_as_double<F>() < std::ldexp(1.0, 261))) return false;
  set_bounds(out, vb, lb, tb);
#else
  (void)lb;
  (void)tb;
#endif
  return true;
}

template <class F>
static uint32_t top_at(int k) {  // a top limb no larger than that of any value < k * MOD
  return (uint32_t)((uint64_t)k * F::MOD[8] + (((uint64_t)k * F::MOD[7]) >> 29));
}

template <class F>
static std::vector<Fe<F>> edge_operands(bool lazy) {
  std::vector<Fe<F>> v;
  Fe<F> x;
  auto push = [&](const uint32_t (&l)[9], uint64_t lb, uint64_t tb) {
    if (make<F>(x, l, lb, tb)) v.push_back(x);
  };
  uint32_t l[9] = {};
  push(l, 0, 0);                                                  // 0
  l[0] = 1;
  push(l, MASK29, 0);                                             // the integer 1
  for (int i = 0; i < 9; ++i) l[i] = F::ONE[i];
  push(l, MASK29, F::MOD[8]);                                     // the field's 1
  for (int i = 0; i < 9; ++i) l[i] = F::MOD[i];
  l[0] -= 1;
  push(l, MASK29, F::MOD[8]);                                     // p - 1
  for (int i = 0; i < 9; ++i) l[i] = MASK29;
  push(l, MASK29, MASK29);                                        // all limbs at MASK29 (2^261 - 1: beyond every class)
  l[8] = MASK29 - 1;
  push(l, MASK29, MASK29 - 1);                                    // the largest declarable normalised value
  for (int k : {1, 2, 3, 4, 5, 8, 9, 12}) {                       // top limb at the bound of the class "< k * MOD"
    l[8] = top_at<F>(k);
    push(l, MASK29, l[8]);
  }
  if (lazy) {                                                     // unnormalised limbs: lazy sums and differences
    for (uint32_t lb : {(1u << 30) - 1u, (3u << 29) - 1u, (1u << 31) - 1u}) {
      for (int i = 0; i < 8; ++i) l[i] = lb;
      l[8] = top_at<F>(12);
      push(l, lb, l[8]);
      l[8] = MASK29 - 8;
      push(l, lb, l[8]);
    }
  }
  return v;
}

template <class F>
static Fe<F> random_operand() {
  uint32_t l[9];
  for (int i = 0; i < 8; ++i) l[i] = (uint32_t)rng() & MASK29;
  const uint32_t top = top_at<F>(3);
  l[8] = (uint32_t)(rng() % (top + 1));
  Fe<F> x;
  make<F>(x, l, MASK29, top);
  return x;
}

// ---- the comparisons -----------------------------------------------------------------------------------------------
static long failures = 0, checks = 0;
template <class F>
static void expect(const Fe<F>& got, const Limbs& exp, const char* what) {
  ++checks;
  for (int i = 0; i < 9; ++i)
    if (got.l[i] != exp.l[i]) {
      if (++failures <= 10) std::fprintf(stderr, "MISMATCH %s limb %d: got %08x expected %08x\n", what, i, got.l[i], exp.l[i]);
      return;
    }
}

// largest limb of an operand: the column precondition 9*A*B (+ 9*C*D) + 9*2^58 + 2^40 < 2^64 decides what may be multiplied
template <class F>
static long double amax(const Fe<F>& a) {
#ifdef HM_BOUNDS
  return (long double)(a.lb > a.tb ? a.lb : a.tb);  // what the operand is declared at, as the library's check reads it
#endif
  uint32_t m = 0;
  for (int i = 0; i < 9; ++i) m = a.l[i] > m ? a.l[i] : m;
  return (long double)m;
}
static bool fits(long double sum_ab) {
  return 9.0L * sum_ab + 9.0L * 288230376151711744.0L + 1099511627776.0L < 18446744073709551616.0L;
}

// with bound tracking on, the result must be declarable too: (value bound of the products) / 2^261 + 1 modulus below 2^261
template <class F>
static bool result_fits(const Fe<F>& a, const Fe<F>& b, const Fe<F>* c = nullptr, const Fe<F>* d = nullptr) {
#ifdef HM_BOUNDS
  const double prod = a.vb * b.vb + (c ? c->vb * d->vb : 0.0);
  return (prod * mod_as_double<F>() / std::ldexp(1.0, 261) + 1.0) * mod_as_double<F>() < std::ldexp(1.0, 261);
#else
  (void)a; (void)b; (void)c; (void)d;
  return true;
#endif
}

template <class F>
static void check_pair(const Fe<F>& a, const Fe<F>& b, const Fe<F>& c, const Fe<F>& d) {
  Fe<F> r0, r1, r2;
  if (fits(amax(a) * amax(b)) && result_fits(a, b)) {
    const Limbs e = ref_mul<F>(a.l, b.l);
    expect(fe_mul(a, b), e, "fe_mul");
    if (fits(amax(c) * amax(d)) && result_fits(c, d)) {
      const Limbs e1 = ref_mul<F>(c.l, d.l);
      fe_mul_x2(r0, r1, a, b, c, d);
      expect(r0, e, "fe_mul_x2[0]");
      expect(r1, e1, "fe_mul_x2[1]");
      if (fits(amax(b) * amax(c)) && result_fits(b, c)) {
        fe_mul_x3(r0, r1, r2, a, b, c, d, b, c);
        expect(r0, e, "fe_mul_x3[0]");
        expect(r1, e1, "fe_mul_x3[1]");
        expect(r2, ref_mul<F>(b.l, c.l), "fe_mul_x3[2]");
      }
    }
    if (fits(amax(a) * amax(b) + amax(c) * amax(d)) && result_fits(a, b, &c, &d)) {
      const Limbs e2 = ref_mul2<F>(a.l, b.l, c.l, d.l);
      expect(fe_mul2(a, b, c, d), e2, "fe_mul2");
      fe_mul_mul2(r0, r1, a, b, a, b, c, d);
      expect(r0, e, "fe_mul_mul2[0]");
      expect(r1, e2, "fe_mul_mul2[1]");
    }
  }
  if (2.0L * amax(a) < 4294967296.0L && fits(amax(a) * amax(a)) && result_fits(a, a)) {
    const Limbs e = ref_sqr<F>(a.l);
    expect(fe_sqr(a), e, "fe_sqr");
    expect(fe_sqr(a), ref_mul<F>(a.l, a.l), "fe_sqr against the plain product");
    if (2.0L * amax(c) < 4294967296.0L && fits(amax(c) * amax(c)) && result_fits(c, c)) {
      fe_sqr_x2(r0, r1, a, c);
      expect(r0, e, "fe_sqr_x2[0]");
      expect(r1, ref_sqr<F>(c.l), "fe_sqr_x2[1]");
    }
  }
}

template <class F>
static void run_field(const char* name, int randoms) {
  const long before = checks;
  const std::vector<Fe<F>> edges = edge_operands<F>(true);
  for (const Fe<F>& a : edges)
    for (const Fe<F>& b : edges) check_pair<F>(a, b, b, a);
  for (const Fe<F>& a : edges) {
    const Fe<F> x = random_operand<F>(), y = random_operand<F>();
    check_pair<F>(a, x, y, a);
    check_pair<F>(x, a, a, y);
  }
  for (int i = 0; i < randoms; ++i) {
    const Fe<F> a = random_operand<F>(), b = random_operand<F>(), c = random_operand<F>(), d = random_operand<F>();
    check_pair<F>(a, b, c, d);
  }
  std::printf("%s: %zu edge operands, %d random quadruples, %ld comparisons\n", name, edges.size(), randoms, checks - before);
}

int main(int argc, char** argv) {
  const int randoms = argc > 1 ? std::atoi(argv[1]) : 100000;
  run_field<FqParams>("Fq", randoms);
  run_field<FrParams>("Fr", randoms);
  if (failures) {
    std::fprintf(stderr, "%ld of %ld comparisons FAILED\n", failures, checks);
    return 1;
  }
  std::printf("ok: %ld comparisons, all bit-identical\n", checks);
  return 0;
}
