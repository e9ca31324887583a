// poseidon.inc -- Poseidon over BN256 Fr (halo2_gadgets::poseidon::primitives, P128Pow5T3-style specs: x^5 S-box, R_F full and
// R_P partial rounds) for ConstantLength<L> messages with L = RATE, and the Merkle (sum) trees the reference builds from it
// (/root/reference/src/circuits/merkle_sum_tree.rs:118-150, src/chips/merkle_v3.rs).  Included by polyops.hip from inside
// namespace hm, so that the kernels fall under polyops.o's ISA checks; host_check.cpp includes it too (without the kernels)
// for the bound proof of the 64-round chain.  DESIGN.md section 12.
//
// One hash per lane, the WIDTH state words in registers.  The constants of a spec (hm_poseidon_create) live in device memory
// in the internal form of ff29.h, canonical:
//     rc[(r_f + r_p)][WIDTH][9]   mds[WIDTH][WIDTH][9] (row-major)   cap[9] (the capacity word L * 2^64)
// and are read at addresses that depend only on the round number: every lane of a wave reads the same words.
//
// A round is   x_j = s_j + rc[r][j];   x_j <- x_j^5 (every j in a full round, j = 0 in a partial one);   s_i = sum_j mds[i][j] x_j.
// The MDS row is ONE Montgomery reduction over the WIDTH products (poseidon_dot): 81 WIDTH + 81 wide multiplies per output word
// instead of 162 WIDTH, the dense form (no sparse rewriting of the partial rounds).

HM_HD Fr ps_load9(const uint32_t* p) {              // a constant of the spec: canonical internal form
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = p[i];
  HM_DECLARE(r, 1.0);
  return r;
}

// sum_j row[j] * x[j] * 2^-261: the products of all WIDTH terms share the column accumulators and the reduction.
// Needs normalised limbs on both sides (9 WIDTH + 9 products of 58 bits per column: WIDTH <= 5 fits 64 bits).
template <int W>
HM_HD Fr poseidon_dot(const uint32_t* row, const Fr (&x)[W]) {
  static_assert(W <= 5, "poseidon_dot: the column sum of more than 5 terms does not fit 64 bits");
#ifdef HM_BOUNDS
  {
    long double sum = 0;
    for (int k = 0; k < W; ++k) {
      const long double B = (long double)(x[k].lb > x[k].tb ? x[k].lb : x[k].tb);
      sum += (long double)MASK29 * B;
    }
    HM_CHECK(9.0L * sum + 9.0L * 288230376151711744.0L + 1099511627776.0L < 18446744073709551616.0L,
             "poseidon_dot column sum may overflow 64 bits");
  }
#endif
  uint64_t t[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const uint32_t c = row[k * 9 + i];
#pragma unroll
      for (int j = 0; j < 9; ++j) t[j] += (uint64_t)x[k].l[j] * c;
    }
    const uint32_t m = ((uint32_t)t[0] * FrParams::INV29) & MASK29;
#pragma unroll
    for (int j = 0; j < 9; ++j) t[j] += (uint64_t)m * FrParams::MOD[j];
    t[1] += t[0] >> 29;
#pragma unroll
    for (int j = 0; j < 9; ++j) t[j] = t[j + 1];
    t[9] = 0;
  }
  Fr r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    r.l[j] = (uint32_t)t[j] & MASK29;
    t[j + 1] += t[j] >> 29;
  }
  r.l[8] = (uint32_t)t[8];
#ifdef HM_BOUNDS
  {
    double vsum = 0;
    for (int k = 0; k < W; ++k) {
      HM_CHECK(row[k * 9 + 8] <= FrParams::MOD[8], "poseidon_dot: a constant is not canonical");
      vsum += x[k].vb;
    }
    const double vb = vsum * mod_as_double<FrParams>() / std::ldexp(1.0, 261) + 1.0;
    set_bounds(r, vb, MASK29, top_bound_from_value<FrParams>(vb));
    HM_CHECK(r.l[8] <= r.tb, "poseidon_dot result exceeds its bound");
  }
#endif
  return r;
}

// x^5 of a lazy sum (limbs < 2^30): two squarings and one product
HM_HD Fr poseidon_sbox(const Fr& x) {
  const Fr x2 = fe_sqr(x);
  return fe_mul(fe_sqr(x2), x);
}

// The steps of a round over the words J... as pack expansions: a `#pragma unroll` loop of this size is refused by the unroller
// ("unrolled size is too large"), and a loop left rolled indexes the state at run time, which puts it in scratch.
template <int W, int... J>
HM_HD void poseidon_sbox_rest(Fr (&x)[W], std::integer_sequence<int, J...>) {
  ((x[J + 1] = poseidon_sbox(x[J + 1])), ...);
}
template <int W, int... J>
HM_HD void poseidon_norm_rest(Fr (&x)[W], std::integer_sequence<int, J...>) {
  ((x[J + 1] = fe_norm(x[J + 1])), ...);
}
template <int W, int... I>
HM_HD void poseidon_mix(Fr (&s)[W], const uint32_t* mds, const Fr (&x)[W], std::integer_sequence<int, I...>) {
  ((s[I] = poseidon_dot<W>(mds + I * W * 9, x)), ...);
}

// What a caller may watch of a permutation -- the rows of the Pow5 chip's "permute state" region (witness.inc section below):
// row(i, s) gets the state BEFORE every full round and before every first round of a pair of partial rounds, and the final state;
// sbox0(i, x) the first S-box output of the pair that row i starts.  The hashing kernels pass PoseidonNoTrace: nothing is
// computed for it and their code is what it was.
struct PoseidonNoTrace {
  template <int W>
  HM_HD void row(uint32_t, const Fr (&)[W]) const {}
  template <int W>
  HM_HD void sbox0(uint32_t, const Fr&) const {}
};

// the permutation on WIDTH words in internal form (normalised, product outputs or constants); c = the spec's constant block
template <int W, class Sink>
HM_HD void poseidon_permute(Fr (&s)[W], const uint32_t* c, uint32_t r_f, uint32_t r_p, const Sink& sink) {
  const uint32_t rounds = r_f + r_p, half = r_f >> 1;
  const uint32_t* mds = c + (size_t)rounds * W * 9;
  uint32_t row = 0;
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; ++r) {
    const bool full = r < half || r >= half + r_p;     // the same in every lane
    const bool first = full || !((r - half) & 1u);     // a row of the chip starts with this round
    const uint32_t* rc = c + (size_t)r * W * 9;
    if (first) sink.row(row, s);
    Fr x[W];
#pragma unroll
    for (int j = 0; j < W; ++j) x[j] = fe_add(s[j], ps_load9(rc + j * 9));
    x[0] = poseidon_sbox(x[0]);
    if (first && !full) sink.template sbox0<W>(row, x[0]);
    row += first ? 1u : 0u;
    if (full)
      poseidon_sbox_rest<W>(x, std::make_integer_sequence<int, W - 1>{});
    else
      poseidon_norm_rest<W>(x, std::make_integer_sequence<int, W - 1>{});
    poseidon_mix<W>(s, mds, x, std::make_integer_sequence<int, W>{});
  }
  sink.row(row, s);
}
template <int W>
HM_HD void poseidon_permute(Fr (&s)[W], const uint32_t* c, uint32_t r_f, uint32_t r_p) {
  poseidon_permute<W>(s, c, r_f, r_p, PoseidonNoTrace{});
}

// Hash<_, Spec, ConstantLength<W - 1>, W, W - 1>::init().hash(msg): state = [msg, L * 2^64], one permutation, word 0.
// msg and out are external Montgomery words (msg canonical).
template <int W>
HM_HD void poseidon_hash_one(const uint32_t (&msg)[W - 1][8], const uint32_t* c, uint32_t r_f, uint32_t r_p, uint32_t (&out)[8]) {
  Fr s[W];
#pragma unroll
  for (int j = 0; j < W - 1; ++j) s[j] = fe_from_ext<FrParams>(msg[j]);
  s[W - 1] = ps_load9(c + ((size_t)(r_f + r_p) * W + (size_t)W * W) * 9);
  poseidon_permute<W>(s, c, r_f, r_p);
  fe_to_ext(out, s[0]);
}

// (a + b) mod r on external Montgomery words (the sum of two balances): any 256-bit inputs, canonical output
HM_HD void fr_add_ext(const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t (&out)[8]) {
  const Fr v = fe_canonical(fe_reduce_small(fe_norm(fe_add(fe_unpack<FrParams>(a), fe_unpack<FrParams>(b)))));
  fe_pack(out, v);
}

// one node of a Merkle sum tree: children (hash, balance) x 2 as 32 external words -> (hash, balance) as 16
HM_HD void merkle_sum_node_one(const uint32_t (&kids)[4][8], const uint32_t* c, uint32_t r_f, uint32_t r_p, uint32_t (&hash)[8],
                               uint32_t (&balance)[8]) {
  fr_add_ext(kids[1], kids[3], balance);
  poseidon_hash_one<5>(kids, c, r_f, r_p, hash);
}

// ---- the MerkleSumTree circuit's witness (DESIGN.md section 13) -----------------------------------------------------------------
// The advice columns of circuits.merkle_sum_tree() for one inclusion path, filled as the reference's chip assigns them
// (/root/reference/src/chips/merkle_sum_tree.rs:140-352; the Pow5 and Lt chips as recalled in synthesis.py).  One lane per
// (user, level): it writes the level's "merkle prove layer" rows, the hash's initial-state and pad-and-add rows and, through the
// sink of poseidon_permute, the trace of the permutation; the lane of level 0 adds the leaf rows, the lane of the last level the
// less-than region and the root.  Cells the chip leaves unassigned are zero: the caller clears the columns first.
//
// Row placement (synthesis.MerkleSumTreeLayout restates it; tests compare the two for every depth):
//     row 0 leaf hash, row 1 leaf balance; level l at 2 + l * level_rows: prove layer (2 rows), initial state (1), pad-and-add (3),
//     permute state (perm_rows = r_f + r_p / 2 + 1); then the less-than row; then 5 constants per level in rc_b[0] (fixed only).
constexpr uint32_t WITNESS_ADVICE = 20;      // a b c d e | state[5] | partial_sbox | lt | diff[8]
constexpr uint32_t WITNESS_U8_ROWS = 256;    // the LtChip's range table occupies rows 0..255 of its own fixed column
struct WitnessLayout {
  uint32_t perm_rows, level_rows, lt_row, const_row, rows_used;
};
HM_HD WitnessLayout merkle_sum_witness_layout(uint32_t depth, uint32_t r_f, uint32_t r_p) {
  WitnessLayout w;
  w.perm_rows = r_f + r_p / 2 + 1;
  w.level_rows = 2 + 1 + 3 + w.perm_rows;
  w.lt_row = 2 + depth * w.level_rows;
  w.const_row = w.lt_row + 1;
  w.rows_used = w.const_row + 5 * depth;
  if (w.rows_used < WITNESS_U8_ROWS) w.rows_used = WITNESS_U8_ROWS;
  return w;
}

struct PsConst {
  static constexpr uint32_t TO_CANON[9] = {32u, 0, 0, 0, 0, 0, 0, 0, 0};     // x * 32 * 2^-261 = x * 2^-256: Montgomery words -> the integer
  // 2^517 mod r: v * 2^517 * 2^-261 = v * 2^256, a small integer -> its Montgomery words
  static constexpr uint32_t SMALL2EXT[9] = {0x142db4dfu, 0x19d6990eu, 0x1472f48cu, 0x06dbe7e3u, 0x0b84d579u, 0x10f9faf7u, 0x121f4380u,
                                            0x17a112deu, 0x001275c7u};
};

struct alignas(16) PsQuad {
  uint32_t v[4];
};
HM_HD void ps_get_words(const uint32_t* p, uint32_t (&w)[8]) {
  const PsQuad* q = reinterpret_cast<const PsQuad*>(p);
  const PsQuad lo = q[0], hi = q[1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i] = lo.v[i];
    w[4 + i] = hi.v[i];
  }
}
HM_HD void ps_put_words(uint32_t* p, const uint32_t (&w)[8]) {
  PsQuad* q = reinterpret_cast<PsQuad*>(p);
  q[0] = PsQuad{{w[0], w[1], w[2], w[3]}};
  q[1] = PsQuad{{w[4], w[5], w[6], w[7]}};
}

// internal form -> Montgomery words as a division by 32 (v * 2^261 -> v * 2^256): one reduction step on the low 5 bits and a shift,
// 9 narrow multiplies instead of fe_to_ext's full product by a constant.  a: normalised limbs, value < 2^261.  Canonical output.
HM_HD void fe_to_ext_shift(uint32_t (&w)[8], const Fr& a) {
#ifdef HM_BOUNDS
  HM_CHECK(a.lb <= MASK29 && a.tb < (1ull << 29), "fe_to_ext_shift needs normalised limbs");
#endif
  const uint32_t m = (a.l[0] * FrParams::INV29) & 31u;        // a + m * MOD = 0 mod 32
  uint32_t t[9];
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t v = (uint64_t)a.l[i] + (uint64_t)m * FrParams::MOD[i] + carry;
    t[i] = (uint32_t)v & MASK29;
    carry = v >> 29;
  }
  t[8] = (uint32_t)((uint64_t)a.l[8] + (uint64_t)m * FrParams::MOD[8] + carry);     // < 2^29 + 2^30
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = (t[i] >> 5) | ((t[i + 1] & 31u) << 24);
  r.l[8] = t[8] >> 5;
#ifdef HM_BOUNDS
  HM_CHECK((t[0] & 31u) == 0, "fe_to_ext_shift: the sum is not divisible by 32");
  {
    const double vb = (a.vb + 31.0) / 32.0;
    set_bounds(r, vb, MASK29, top_bound_from_value<FrParams>(vb));
    HM_CHECK(r.l[8] <= r.tb, "fe_to_ext_shift result exceeds its bound");
  }
#endif
  fe_pack(w, fe_canonical(r));
}

// Montgomery words (any 256-bit value) -> the canonical integer as 8 little-endian words
HM_HD void fr_ext_to_int(const uint32_t (&w)[8], uint32_t (&out)[8]) {
  fe_pack(out, fe_canonical(fe_mul(fe_unpack<FrParams>(w), fe_const<FrParams>(PsConst::TO_CANON))));
}
// an integer below 2^29 -> its Montgomery words
HM_HD void fr_small_to_ext(uint32_t v, uint32_t (&out)[8]) {
  Fr x = fe_zero<FrParams>();
  x.l[0] = v & MASK29;
  HM_DECLARE(x, 1.0);
  fe_pack(out, fe_canonical(fe_mul(x, fe_const<FrParams>(PsConst::SMALL2EXT))));
}

// LtChip::assign on the integers lhs, rhs (canonical, 8 words each): lt = lhs < rhs and the low 8 bytes of
// (lhs - rhs + lt * 2^64) mod r.  r mod 2^64 = 0x43e1f593f0000001.
HM_HD void lt_chip_values(const uint32_t (&lhs)[8], const uint32_t (&rhs)[8], uint32_t& lt, uint64_t& diff) {
  bool less = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    less = (!decided && lhs[i] != rhs[i]) ? lhs[i] < rhs[i] : less;
    decided = decided || lhs[i] != rhs[i];
  }
  uint32_t e[8];                       // |lhs - rhs|
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t hi = less ? rhs[i] : lhs[i], lo = less ? lhs[i] : rhs[i];
    const uint64_t t = (uint64_t)hi - lo - borrow;
    e[i] = (uint32_t)t;
    borrow = (uint32_t)(t >> 63);
  }
  const uint64_t e_lo = (uint64_t)e[0] | ((uint64_t)e[1] << 32);
  const bool above = (e[3] | e[4] | e[5] | e[6] | e[7]) != 0 || e[2] > 1 || (e[2] == 1 && e_lo != 0);   // e > 2^64
  lt = less ? 1u : 0u;
  diff = !less ? e_lo : (above ? 0x43e1f593f0000001ull - e_lo : 0ull - e_lo);
}

struct WitnessArgs {
  const uint32_t* leaves;        // m x 16 words: hash, balance
  const uint32_t* siblings;      // m x depth x 16
  const uint64_t* indices;       // m: bit l = the path's node is the right child at level l
  const uint32_t* nodes;         // the built tree (2^(depth+1) - 1 nodes of 16 words), or null
  const uint32_t* run;           // without a tree: m x (depth - 1) x 16, the path's node after levels 1 .. depth - 1 (merkle_sum_chain_lane)
  uint32_t* advice;              // m x WITNESS_ADVICE x 2^log_n x 8, cleared
  uint32_t* instance;            // m x 4 x 8: leaf hash, leaf balance, root, assets
  const uint32_t* consts;
  uint64_t m;
  uint32_t depth, log_n, r_f, r_p;
  uint32_t assets[8];
};

// the rows of "permute state" into the columns state[0..W-1] and partial_sbox (the column after them) of one hash
struct WitnessSink {
  uint32_t* state0;              // word 0 of column state[0] at the region's first row
  uint64_t col_words;            // words from one column to the next
  template <int W>
  HM_HD void row(uint32_t i, const Fr (&s)[W]) const {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      uint32_t w[8];
      fe_to_ext_shift(w, s[j]);
      ps_put_words(state0 + j * col_words + (uint64_t)i * 8, w);
    }
  }
  template <int W>
  HM_HD void sbox0(uint32_t i, const Fr& x) const {
    uint32_t w[8];
    fe_to_ext_shift(w, x);
    ps_put_words(state0 + W * col_words + (uint64_t)i * 8, w);
  }
};

// the path's node after level l + 1, for l = 0 .. depth - 2, of user u: the chain that a built tree makes unnecessary
HM_HD void merkle_sum_chain_lane(const WitnessArgs& a, uint64_t u, uint32_t* run) {
  uint32_t node[2][8];
  ps_get_words(a.leaves + u * 16, node[0]);
  ps_get_words(a.leaves + u * 16 + 8, node[1]);
  const uint64_t idx = a.indices[u];
#pragma unroll 1
  for (uint32_t l = 0; l + 1 < a.depth; ++l) {
    uint32_t sib[2][8], kids[4][8];
    ps_get_words(a.siblings + (u * a.depth + l) * 16, sib[0]);
    ps_get_words(a.siblings + (u * a.depth + l) * 16 + 8, sib[1]);
    const bool right = (idx >> l) & 1ull;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kids[0][i] = right ? sib[0][i] : node[0][i];
      kids[1][i] = right ? sib[1][i] : node[1][i];
      kids[2][i] = right ? node[0][i] : sib[0][i];
      kids[3][i] = right ? node[1][i] : sib[1][i];
    }
    merkle_sum_node_one(kids, a.consts, a.r_f, a.r_p, node[0], node[1]);
    ps_put_words(run + (u * (a.depth - 1) + l) * 16, node[0]);
    ps_put_words(run + (u * (a.depth - 1) + l) * 16 + 8, node[1]);
  }
}

// everything level l of user u contributes to the witness (see the head of this section)
HM_HD void merkle_sum_witness_lane(const WitnessArgs& a, uint64_t u, uint32_t l) {
  const WitnessLayout lay = merkle_sum_witness_layout(a.depth, a.r_f, a.r_p);
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* adv = a.advice + u * WITNESS_ADVICE * col_words;
  const uint64_t base = 2 + (uint64_t)l * lay.level_rows;
  const uint64_t idx = a.indices[u] & ((a.depth >= 64 ? 0 : (1ull << a.depth)) - 1);
  const bool right = (idx >> l) & 1ull;

  uint32_t kids[4][8], sum[8], w[8];
  {
    uint32_t prev[2][8], sib[2][8];
    const uint32_t* p = l == 0 ? a.leaves + u * 16
                        : a.nodes ? a.nodes + (((2ull << a.depth) - (2ull << (a.depth - l))) + (idx >> l)) * 16
                                  : a.run + (u * (a.depth - 1) + (l - 1)) * 16;
    ps_get_words(p, prev[0]);
    ps_get_words(p + 8, prev[1]);
    ps_get_words(a.siblings + (u * a.depth + l) * 16, sib[0]);
    ps_get_words(a.siblings + (u * a.depth + l) * 16 + 8, sib[1]);
    if (l == 0) {                                          // "assign leaf hash", "assign leaf balance"; instance rows 0, 1
      ps_put_words(adv + 0 * col_words + 0 * 8, prev[0]);
      ps_put_words(adv + 1 * col_words + 1 * 8, prev[1]);
      ps_put_words(a.instance + u * 32, prev[0]);
      ps_put_words(a.instance + u * 32 + 8, prev[1]);
    }
    // "merkle prove layer" row 0: previous node, sibling, index
    ps_put_words(adv + 0 * col_words + base * 8, prev[0]);
    ps_put_words(adv + 1 * col_words + base * 8, prev[1]);
    ps_put_words(adv + 2 * col_words + base * 8, sib[0]);
    ps_put_words(adv + 3 * col_words + base * 8, sib[1]);
    fr_small_to_ext(right ? 1u : 0u, w);
    ps_put_words(adv + 4 * col_words + base * 8, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kids[0][i] = right ? sib[0][i] : prev[0][i];
      kids[1][i] = right ? sib[1][i] : prev[1][i];
      kids[2][i] = right ? prev[0][i] : sib[0][i];
      kids[3][i] = right ? prev[1][i] : sib[1][i];
    }
  }
  fr_add_ext(kids[1], kids[3], sum);
  // row 1: left, right, their sum; the hash's input row and the pad-and-add output row repeat the four words
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ps_put_words(adv + j * col_words + (base + 1) * 8, kids[j]);
    ps_put_words(adv + (5 + j) * col_words + (base + 4) * 8, kids[j]);
    ps_put_words(adv + (5 + j) * col_words + (base + 5) * 8, kids[j]);
  }
  ps_put_words(adv + 4 * col_words + (base + 1) * 8, sum);
  // the capacity word: "initial state", pad-and-add rows 0 and 2 (the four rate words of the initial state are zero)
  fe_to_ext_shift(w, ps_load9(a.consts + ((size_t)(a.r_f + a.r_p) * 5 + 25) * 9));
  ps_put_words(adv + 9 * col_words + (base + 2) * 8, w);
  ps_put_words(adv + 9 * col_words + (base + 3) * 8, w);
  ps_put_words(adv + 9 * col_words + (base + 5) * 8, w);

  if (l + 1 == a.depth) {          // "enforce sum to be less than total assets": a = the sum, b = the assets, c = check = 1, LtChip
    const uint64_t row = lay.lt_row;
    uint32_t si[8], ai[8], lt;
    uint64_t diff;
    ps_put_words(adv + 0 * col_words + row * 8, sum);
    ps_put_words(adv + 1 * col_words + row * 8, a.assets);
    ps_put_words(a.instance + u * 32 + 24, a.assets);
    fr_ext_to_int(sum, si);
    fr_ext_to_int(a.assets, ai);
    lt_chip_values(si, ai, lt, diff);
    fr_small_to_ext(1u, w);
    ps_put_words(adv + 2 * col_words + row * 8, w);
    fr_small_to_ext(lt, w);
    ps_put_words(adv + 11 * col_words + row * 8, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      fr_small_to_ext((uint32_t)(diff >> (8 * i)) & 0xffu, w);
      ps_put_words(adv + (12 + i) * col_words + row * 8, w);
    }
  }

  Fr s[5];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = fe_from_ext<FrParams>(kids[j]);
  s[4] = ps_load9(a.consts + ((size_t)(a.r_f + a.r_p) * 5 + 25) * 9);
  const WitnessSink sink{adv + 5 * col_words + (base + 6) * 8, col_words};
  poseidon_permute<5>(s, a.consts, a.r_f, a.r_p, sink);
  if (l + 1 == a.depth) {                                  // the root: instance row 2
    fe_to_ext_shift(w, s[0]);
    ps_put_words(a.instance + u * 32 + 16, w);
  }
}

// ---- the MerkleTreeV3 and Poseidon circuits' witnesses (DESIGN.md section 14) -------------------------------------------------------
// The advice columns of circuits.merkle_v3() for one inclusion path (/root/reference/src/chips/merkle_v3.rs:84-172) and of
// circuits.poseidon() for one hash (src/chips/poseidon/hash_with_instance.rs:78-148), with the Pow5 regions of the section above.
// Row placement (synthesis.MerkleTreeV3Layout / PoseidonCircuitLayout restate it; tests compare the two):
//     merkle_v3: row 0 the leaf; level l at 1 + l * level_rows: prove layer (2 rows), initial state (1), pad-and-add (3), permute
//                state (perm_rows); then 3 constants per level in rc_b[0] (fixed only).
//     poseidon:  row 0 the private inputs, row 1 their copies, initial state (1), pad-and-add (3), permute state; then 5 constants.
constexpr uint32_t MERKLE_WITNESS_ADVICE = 7;        // a b c | state[3] | partial_sbox
constexpr uint32_t POSEIDON_WITNESS_ADVICE = 6;      // state[5] | partial_sbox
struct Pow5Layout {
  uint32_t perm_rows, level_rows, const_row, rows_used;
};
HM_HD Pow5Layout merkle_witness_layout(uint32_t depth, uint32_t r_f, uint32_t r_p) {
  Pow5Layout w;
  w.perm_rows = r_f + r_p / 2 + 1;
  w.level_rows = 2 + 1 + 3 + w.perm_rows;
  w.const_row = 1 + depth * w.level_rows;
  w.rows_used = w.const_row + 3 * depth;
  return w;
}
HM_HD Pow5Layout poseidon_witness_layout(uint32_t r_f, uint32_t r_p) {      // level_rows: everything before the constants
  Pow5Layout w;
  w.perm_rows = r_f + r_p / 2 + 1;
  w.level_rows = 1 + 1 + 1 + 3 + w.perm_rows;
  w.const_row = w.level_rows;
  w.rows_used = w.const_row + 5;
  return w;
}

struct MerkleWitnessArgs {
  const uint32_t* leaves;        // m x 8 words
  const uint32_t* siblings;      // m x depth x 8
  const uint64_t* indices;       // m: bit l = the path's node is the right child at level l
  const uint32_t* nodes;         // the built tree (2^(depth+1) - 1 nodes of 8 words), or null
  const uint32_t* run;           // without a tree: m x (depth - 1) x 8, the path's node after levels 1 .. depth - 1 (merkle_chain_lane)
  uint32_t* advice;              // m x MERKLE_WITNESS_ADVICE x 2^log_n x 8, cleared
  uint32_t* instance;            // m x 2 x 8: leaf, root
  const uint32_t* consts;
  uint64_t m;
  uint32_t depth, log_n, r_f, r_p;
};

// the path's node after level l + 1, for l = 0 .. depth - 2, of user u
HM_HD void merkle_chain_lane(const MerkleWitnessArgs& a, uint64_t u, uint32_t* run) {
  uint32_t node[8];
  ps_get_words(a.leaves + u * 8, node);
  const uint64_t idx = a.indices[u];
#pragma unroll 1
  for (uint32_t l = 0; l + 1 < a.depth; ++l) {
    uint32_t sib[8], kids[2][8];
    ps_get_words(a.siblings + (u * a.depth + l) * 8, sib);
    const bool right = (idx >> l) & 1ull;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kids[0][i] = right ? sib[i] : node[i];
      kids[1][i] = right ? node[i] : sib[i];
    }
    poseidon_hash_one<3>(kids, a.consts, a.r_f, a.r_p, node);
    ps_put_words(run + (u * (a.depth - 1) + l) * 8, node);
  }
}

// everything level l of user u contributes to the MerkleTreeV3 witness
HM_HD void merkle_witness_lane(const MerkleWitnessArgs& a, uint64_t u, uint32_t l) {
  const Pow5Layout lay = merkle_witness_layout(a.depth, a.r_f, a.r_p);
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* adv = a.advice + u * MERKLE_WITNESS_ADVICE * col_words;
  const uint64_t base = 1 + (uint64_t)l * lay.level_rows;
  const uint64_t idx = a.indices[u] & ((1ull << a.depth) - 1);          // depth <= 32
  const bool right = (idx >> l) & 1ull;

  uint32_t kids[2][8], w[8];
  {
    uint32_t prev[8], sib[8];
    const uint32_t* p = l == 0 ? a.leaves + u * 8
                        : a.nodes ? a.nodes + (((2ull << a.depth) - (2ull << (a.depth - l))) + (idx >> l)) * 8
                                  : a.run + (u * (a.depth - 1) + (l - 1)) * 8;
    ps_get_words(p, prev);
    ps_get_words(a.siblings + (u * a.depth + l) * 8, sib);
    if (l == 0) {                                          // "assign leaf"; instance row 0
      ps_put_words(adv + 0 * col_words + 0 * 8, prev);
      ps_put_words(a.instance + u * 16, prev);
    }
    // "merkle prove layer" row 0: previous node, path element, index
    ps_put_words(adv + 0 * col_words + base * 8, prev);
    ps_put_words(adv + 1 * col_words + base * 8, sib);
    fr_small_to_ext(right ? 1u : 0u, w);
    ps_put_words(adv + 2 * col_words + base * 8, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kids[0][i] = right ? sib[i] : prev[i];
      kids[1][i] = right ? prev[i] : sib[i];
    }
  }
  // row 1: left, right; the hash's input row and the pad-and-add output row repeat the two words
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ps_put_words(adv + j * col_words + (base + 1) * 8, kids[j]);
    ps_put_words(adv + (3 + j) * col_words + (base + 4) * 8, kids[j]);
    ps_put_words(adv + (3 + j) * col_words + (base + 5) * 8, kids[j]);
  }
  // the capacity word: "initial state", pad-and-add rows 0 and 2 (the two rate words of the initial state are zero)
  const uint32_t* cap = a.consts + ((size_t)(a.r_f + a.r_p) * 3 + 9) * 9;
  fe_to_ext_shift(w, ps_load9(cap));
  ps_put_words(adv + 5 * col_words + (base + 2) * 8, w);
  ps_put_words(adv + 5 * col_words + (base + 3) * 8, w);
  ps_put_words(adv + 5 * col_words + (base + 5) * 8, w);

  Fr s[3];
  s[0] = fe_from_ext<FrParams>(kids[0]);
  s[1] = fe_from_ext<FrParams>(kids[1]);
  s[2] = ps_load9(cap);
  const WitnessSink sink{adv + 3 * col_words + (base + 6) * 8, col_words};
  poseidon_permute<3>(s, a.consts, a.r_f, a.r_p, sink);
  if (l + 1 == a.depth) {                                  // the root: instance row 1
    fe_to_ext_shift(w, s[0]);
    ps_put_words(a.instance + u * 16 + 8, w);
  }
}

struct PoseidonWitnessArgs {
  const uint32_t* msgs;          // m x 4 x 8 words
  uint32_t* advice;              // m x POSEIDON_WITNESS_ADVICE x 2^log_n x 8, cleared
  uint32_t* instance;            // m x 8: the digest
  const uint32_t* consts;
  uint64_t m;
  uint32_t log_n, r_f, r_p;
};

// the whole Poseidon circuit of message u
HM_HD void poseidon_witness_lane(const PoseidonWitnessArgs& a, uint64_t u) {
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* adv = a.advice + u * POSEIDON_WITNESS_ADVICE * col_words;
  uint32_t msg[4][8], w[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ps_get_words(a.msgs + (u * 4 + j) * 8, msg[j]);
    ps_put_words(adv + j * col_words + 0 * 8, msg[j]);     // "load private inputs"
    ps_put_words(adv + j * col_words + 1 * 8, msg[j]);     // "copy input cells to hash input cells"
    ps_put_words(adv + j * col_words + 4 * 8, msg[j]);     // pad-and-add: the message row and the output row
    ps_put_words(adv + j * col_words + 5 * 8, msg[j]);
  }
  const uint32_t* cap = a.consts + ((size_t)(a.r_f + a.r_p) * 5 + 25) * 9;
  fe_to_ext_shift(w, ps_load9(cap));
  ps_put_words(adv + 4 * col_words + 2 * 8, w);            // "initial state", pad-and-add rows 0 and 2
  ps_put_words(adv + 4 * col_words + 3 * 8, w);
  ps_put_words(adv + 4 * col_words + 5 * 8, w);
  Fr s[5];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = fe_from_ext<FrParams>(msg[j]);
  s[4] = ps_load9(cap);
  const WitnessSink sink{adv + 6 * 8, col_words};
  poseidon_permute<5>(s, a.consts, a.r_f, a.r_p, sink);
  fe_to_ext_shift(w, s[0]);
  ps_put_words(a.instance + u * 8, w);
}

#if defined(__HIPCC__)
constexpr int PS_THREADS = 256;

__device__ __forceinline__ void ps_load_words(const uint32_t* __restrict__ p, uint32_t (&w)[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
  w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void ps_store_words(uint32_t* __restrict__ p, const uint32_t (&w)[8]) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// message i = the W - 1 consecutive elements at in + i * in_stride (u32 words), digest i at out + i * out_stride: a flat
// message array (strides 8 (W - 1), 8) and a level of the plain width-3 tree (strides 16, 8) are the same launch
template <int W>
__global__ __launch_bounds__(PS_THREADS) void poseidon_hash_kernel(const uint32_t* __restrict__ in, uint64_t in_stride,
                                                                   uint32_t* __restrict__ out, uint64_t out_stride, uint64_t n,
                                                                   const uint32_t* __restrict__ consts, uint32_t r_f, uint32_t r_p) {
  const uint64_t i = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[W - 1][8], d[8];
#pragma unroll
  for (int j = 0; j < W - 1; ++j) ps_load_words(in + i * in_stride + j * 8, msg[j]);
  poseidon_hash_one<W>(msg, consts, r_f, r_p, d);
  ps_store_words(out + i * out_stride, d);
}

// node i of a level of the sum tree from nodes 2i, 2i + 1 of the level below (16 words per node: hash, balance)
__global__ __launch_bounds__(PS_THREADS) void merkle_sum_level_kernel(const uint32_t* __restrict__ below, uint32_t* __restrict__ level,
                                                                      uint64_t n, const uint32_t* __restrict__ consts, uint32_t r_f,
                                                                      uint32_t r_p) {
  const uint64_t i = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t kids[4][8], hash[8], balance[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) ps_load_words(below + i * 32 + j * 8, kids[j]);
  fr_add_ext(kids[1], kids[3], balance);                 // merkle_sum_node_one, the balance stored before the hash runs: it does
  ps_store_words(level + i * 16 + 8, balance);           // not stay in registers across the permutation
  poseidon_hash_one<5>(kids, consts, r_f, r_p, hash);
  ps_store_words(level + i * 16, hash);
}

// sibling nodes of `m` leaves, bottom up: out[(p * depth + l) * words ..] = node ((index_p >> l) ^ 1) of level l, where level l
// starts at node 2^(depth+1) - 2^(depth-l+1) of `nodes`.  One lane per (leaf, level, element).  An index >= 2^depth gives zeros.
__global__ __launch_bounds__(PS_THREADS) void merkle_path_kernel(const uint32_t* __restrict__ nodes, uint32_t depth, uint32_t words_per_node,
                                                                 const uint64_t* __restrict__ indices, uint64_t m,
                                                                 uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  const uint64_t per_path = (uint64_t)depth * words_per_node;
  if (t >= m * per_path) return;
  const uint64_t p = t / per_path, rest = t % per_path;
  const uint32_t l = (uint32_t)(rest / words_per_node), e = (uint32_t)(rest % words_per_node);
  const uint64_t idx = indices[p];
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (idx < (1ull << depth)) {
    const uint64_t level_start = (2ull << depth) - (2ull << (depth - l));
    const uint64_t node = level_start + ((idx >> l) ^ 1ull);
    ps_load_words(nodes + (node * words_per_node + e) * 8, w);
  }
  ps_store_words(out + t * 8, w);
}
// one lane per (user, level); the columns were cleared by the caller
__global__ __launch_bounds__(PS_THREADS) void merkle_sum_witness_kernel(const WitnessArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= a.m * a.depth) return;
  merkle_sum_witness_lane(a, t / a.depth, (uint32_t)(t % a.depth));
}

// one lane per user: depth - 1 hashes in sequence (paths that come without a tree)
__global__ __launch_bounds__(PS_THREADS) void merkle_sum_chain_kernel(const WitnessArgs a, uint32_t* __restrict__ run) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= a.m) return;
  merkle_sum_chain_lane(a, u, run);
}

// MerkleTreeV3: one lane per (user, level); the columns were cleared by the caller
__global__ __launch_bounds__(PS_THREADS) void merkle_witness_kernel(const MerkleWitnessArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= a.m * a.depth) return;
  merkle_witness_lane(a, t / a.depth, (uint32_t)(t % a.depth));
}
__global__ __launch_bounds__(PS_THREADS) void merkle_chain_kernel(const MerkleWitnessArgs a, uint32_t* __restrict__ run) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= a.m) return;
  merkle_chain_lane(a, u, run);
}
// the Poseidon circuit: one lane per hash
__global__ __launch_bounds__(PS_THREADS) void poseidon_witness_kernel(const PoseidonWitnessArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= a.m) return;
  poseidon_witness_lane(a, u);
}
#endif
