// poseidon.inc -- Poseidon over BN256 Fr (halo2_gadgets::poseidon::primitives, P128Pow5T3-style specs: x^5 S-box, R_F full and
// R_P partial rounds) for ConstantLength<L> messages with L = RATE, and the Merkle (sum) trees the reference builds from it
// (/root/reference/src/circuits/merkle_sum_tree.rs:118-150, src/chips/merkle_v3.rs).  Included inside namespace hm by
// poseidon.hip, which holds the kernels and the drivers, by range.hip for the word helpers, and by host_check.cpp for the bound
// proof of the 64-round chain.  DESIGN.md section 12.
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

// ---- the witnesses of the three circuits (DESIGN.md section 13) -----------------------------------------------------------------
// The advice columns of circuits.merkle_sum_tree(), circuits.merkle_v3() and circuits.poseidon(), filled as the reference's chips
// assign them (/root/reference/src/chips/merkle_sum_tree.rs:140-352, src/chips/merkle_v3.rs:84-172,
// src/chips/poseidon/hash_with_instance.rs:78-148; the Pow5 and Lt chips as recalled in synthesis.py).  The rows of one hash are
// written in ONE place, pow5_hash_rows; the two path circuits are one lane function over E, the elements per node (2: the sum tree's
// (hash, balance), W = 5; 1: MerkleTreeV3, W = 3), one lane per (user, level); the Poseidon circuit is one lane per hash.
// Cells the chips leave unassigned are zero: the caller clears the columns first.
//
// Row placement (synthesis.py's layouts restate it; tests compare the two for every depth), with hash = initial state (1 row),
// pad-and-add (3), permute state (perm_rows = r_f + r_p / 2 + 1):
//     path circuits: leaf element e in column e, row e; level l at E + l * level_rows: prove layer (2 rows), hash; E = 2 only: the
//                    less-than row; then W constants per level in rc_b[0] (fixed only).
//     poseidon:      row 0 the private inputs, row 1 their copies, hash; then 5 constants.
// Columns: a b c d e | state[5] | partial_sbox | lt | diff[8] (E = 2), a b c | state[3] | partial_sbox (E = 1), state[5] | partial_sbox
constexpr uint32_t WITNESS_U8_ROWS = 256;    // the LtChip's range table occupies rows 0..255 of its own fixed column
HM_HD constexpr uint32_t witness_advice(uint32_t E) { return E == 2 ? 20u : E == 1 ? 7u : 6u; }
struct WitnessLayout {
  uint32_t perm_rows, level_rows, lt_row, const_row, rows_used;      // lt_row: E = 2 only
};
// E = 0: the Poseidon circuit (depth is ignored; level_rows counts every row before the constants)
HM_HD WitnessLayout witness_layout(uint32_t E, uint32_t depth, uint32_t r_f, uint32_t r_p) {
  const uint32_t levels = E ? depth : 1u, W = E ? 2 * E + 1 : 5u;
  WitnessLayout w;
  w.perm_rows = r_f + r_p / 2 + 1;
  w.level_rows = 2 + 1 + 3 + w.perm_rows;
  w.lt_row = E + levels * w.level_rows;
  w.const_row = w.lt_row + (E == 2 ? 1u : 0u);
  w.rows_used = w.const_row + W * levels;
  if (E == 2 && w.rows_used < WITNESS_U8_ROWS) w.rows_used = WITNESS_U8_ROWS;
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
  const uint32_t* leaves;        // m x E x 8 words (E = 2: hash, balance); the Poseidon circuit: the messages, m x 4 x 8
  const uint32_t* siblings;      // m x depth x E x 8
  const uint64_t* indices;       // m: bit l = the path's node is the right child at level l
  const uint32_t* nodes;         // the built tree (2^(depth+1) - 1 nodes of E x 8 words), or null
  const uint32_t* run;           // without a tree: m x (depth - 1) x E x 8, the path's node after levels 1 .. depth - 1 (merkle_chain_lane)
  uint32_t* advice;              // m x witness_advice(E) x 2^log_n x 8, cleared
  uint32_t* instance;            // m x rows x 8: E = 2 leaf hash, leaf balance, root, assets; E = 1 leaf, root; poseidon the digest
  const uint32_t* consts;
  uint64_t m;
  uint32_t depth, log_n, r_f, r_p;
  uint32_t assets[8];            // E = 2 only
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

// The Pow5 chip's rows of one hash of `msg`; state0: word 0 of column state[0] at the "initial state" row.  The capacity word on
// rows 0 ("initial state"), 1 and 3 (pad-and-add rows 0 and 2; the rate words of the initial state are zero), the message on rows
// 2 and 3 (the message row and the output row), the trace of the permutation from row 4.  Leaves the final state in s.
template <int W>
HM_HD void pow5_hash_rows(uint32_t* state0, uint64_t col_words, const uint32_t (&msg)[W - 1][8], const uint32_t* consts, uint32_t r_f,
                          uint32_t r_p, Fr (&s)[W]) {
#pragma unroll
  for (int j = 0; j < W - 1; ++j) {
    ps_put_words(state0 + j * col_words + 2 * 8, msg[j]);
    ps_put_words(state0 + j * col_words + 3 * 8, msg[j]);
  }
  const uint32_t* cap = consts + ((size_t)(r_f + r_p) * W + (size_t)W * W) * 9;
  uint32_t w[8];
  fe_to_ext_shift(w, ps_load9(cap));
  ps_put_words(state0 + (W - 1) * col_words + 0 * 8, w);
  ps_put_words(state0 + (W - 1) * col_words + 1 * 8, w);
  ps_put_words(state0 + (W - 1) * col_words + 3 * 8, w);
#pragma unroll
  for (int j = 0; j < W - 1; ++j) s[j] = fe_from_ext<FrParams>(msg[j]);
  s[W - 1] = ps_load9(cap);
  poseidon_permute<W>(s, consts, r_f, r_p, WitnessSink{state0 + 4 * 8, col_words});
}

// one level of a path folded upwards: node <- the parent of (node, sibling), `right` = node is the right child
template <int E>
HM_HD void merkle_fold_level(uint32_t (&node)[E][8], const uint32_t* sibling, bool right, const uint32_t* consts, uint32_t r_f,
                             uint32_t r_p) {
  uint32_t sib[E][8], kids[2 * E][8];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    ps_get_words(sibling + e * 8, sib[e]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kids[e][i] = right ? sib[e][i] : node[e][i];
      kids[E + e][i] = right ? node[e][i] : sib[e][i];
    }
  }
  if constexpr (E == 2)
    merkle_sum_node_one(kids, consts, r_f, r_p, node[0], node[1]);
  else
    poseidon_hash_one<3>(kids, consts, r_f, r_p, node[0]);
}

// the path's node after level l + 1, for l = 0 .. depth - 2, of user u: the chain that a built tree makes unnecessary
template <int E>
HM_HD void merkle_chain_lane(const WitnessArgs& a, uint64_t u, uint32_t* run) {
  uint32_t node[E][8];
#pragma unroll
  for (int e = 0; e < E; ++e) ps_get_words(a.leaves + (u * E + e) * 8, node[e]);
  const uint64_t idx = a.indices[u];
#pragma unroll 1
  for (uint32_t l = 0; l + 1 < a.depth; ++l) {
    merkle_fold_level<E>(node, a.siblings + (u * a.depth + l) * E * 8, (idx >> l) & 1ull, a.consts, a.r_f, a.r_p);
#pragma unroll
    for (int e = 0; e < E; ++e) ps_put_words(run + ((u * (a.depth - 1) + l) * E + e) * 8, node[e]);
  }
}

// the same fold finished to the root (compute_merkle_sum_root for E = 2): path u of `depth` siblings in the layout the path kernel
// writes -> E elements at roots + u * E * 8.  Bit l of the index = the node is the right child at level l; higher bits are ignored.
template <int E>
HM_HD void merkle_root_lane(const uint32_t* leaves, const uint32_t* siblings, const uint64_t* indices, uint32_t depth, const uint32_t* consts,
                            uint32_t r_f, uint32_t r_p, uint64_t u, uint32_t* roots) {
  uint32_t node[E][8];
#pragma unroll
  for (int e = 0; e < E; ++e) ps_get_words(leaves + (u * E + e) * 8, node[e]);
  const uint64_t idx = indices[u];
#pragma unroll 1
  for (uint32_t l = 0; l < depth; ++l)
    merkle_fold_level<E>(node, siblings + (u * depth + l) * E * 8, (idx >> l) & 1ull, consts, r_f, r_p);
#pragma unroll
  for (int e = 0; e < E; ++e) ps_put_words(roots + (u * E + e) * 8, node[e]);
}

// ---- updating a built tree in place (DESIGN.md section 15) ------------------------------------------------------------------------
// m entries (leaf index, new leaf) applied in array order.  The plan, all of it a function of the indices alone:
//   key      entry p -> (index << 32) | ~p, an index >= 2^depth -> MU_DROPPED; sorted ascending, the LAST entry of an index comes
//            first in its run, and the dropped entries (and the padding of the sort, all ones) come last
//   owned    the first entry of a run is live.  It owns its path's node at every level l < owned, where owned - 1 is the highest bit in
//            which its index differs from the live entry before it (depth + 1 for the first): below that bit the two paths are
//            apart, from it upwards they are one, and the earlier entry has the node.  0 = not live.
//   counts   the entries ordered by `owned`, largest first (bins by a histogram; the order inside a bin is irrelevant): the owners
//            of level l are the prefix of length counts[l] = sum of hist[d] over d > l -- one hash per distinct touched node.
constexpr uint32_t MU_DROPPED = 0xffffffffu;
constexpr uint32_t MU_BINS = 32;                 // owned <= depth + 1 <= 31
HM_HD uint64_t merkle_update_key(uint64_t index, uint32_t pos, uint32_t depth) {
  const uint32_t hi = index < (1ull << depth) ? (uint32_t)index : MU_DROPPED;
  return ((uint64_t)hi << 32) | (uint32_t)~pos;
}
HM_HD uint32_t merkle_update_owned(uint64_t prev_key, uint64_t key, bool first, uint32_t depth) {
  const uint32_t idx = (uint32_t)(key >> 32), prev = (uint32_t)(prev_key >> 32);
  if (idx == MU_DROPPED) return 0;
  if (first) return depth + 1;
  const uint32_t x = idx ^ prev;
  return x ? 32u - (uint32_t)__builtin_clz(x) : 0u;
}
// counts[l], l = 0 .. depth: the live entries (l = 0), the nodes hashed at level l; also where bin l of the ordered entries starts
HM_HD uint32_t merkle_update_count(const uint32_t* hist, uint32_t l) {
  uint32_t above = 0;
  for (uint32_t d = l + 1; d < MU_BINS; ++d) above += hist[d];
  return above;
}

// "enforce sum to be less than total assets" at row0 = word 0 of column a at the less-than row: a = the sum, b = the assets,
// c = check = 1, LtChip (lt in column 11, the bytes of diff in 12 .. 19)
HM_HD void merkle_sum_lt_row(uint32_t* row0, uint64_t col_words, const uint32_t (&sum)[8], const uint32_t (&assets)[8]) {
  uint32_t si[8], ai[8], w[8], lt;
  uint64_t diff;
  ps_put_words(row0 + 0 * col_words, sum);
  ps_put_words(row0 + 1 * col_words, assets);
  fr_ext_to_int(sum, si);
  fr_ext_to_int(assets, ai);
  lt_chip_values(si, ai, lt, diff);
  fr_small_to_ext(1u, w);
  ps_put_words(row0 + 2 * col_words, w);
  fr_small_to_ext(lt, w);
  ps_put_words(row0 + 11 * col_words, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fr_small_to_ext((uint32_t)(diff >> (8 * i)) & 0xffu, w);
    ps_put_words(row0 + (12 + i) * col_words, w);
  }
}

// everything level l of user u contributes to the witness of a path circuit: the level's "merkle prove layer" rows and its hash;
// the lane of level 0 adds the leaf rows, the lane of the last level the root (and, E = 2, the less-than region and the assets)
template <int E>
HM_HD void merkle_witness_lane(const WitnessArgs& a, uint64_t u, uint32_t l) {
  constexpr int W = 2 * E + 1;
  const WitnessLayout lay = witness_layout(E, a.depth, a.r_f, a.r_p);
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* adv = a.advice + u * witness_advice(E) * col_words;
  uint32_t* inst = a.instance + u * (E == 2 ? 4 : 2) * 8;
  const uint64_t base = E + (uint64_t)l * lay.level_rows;
  const uint64_t idx = a.indices[u] & ((1ull << a.depth) - 1);          // depth <= 32
  const bool right = (idx >> l) & 1ull;

  uint32_t kids[2 * E][8], w[8];
  {
    uint32_t prev[E][8], sib[E][8];
    const uint32_t* p = l == 0 ? a.leaves + u * E * 8
                        : a.nodes ? a.nodes + (((2ull << a.depth) - (2ull << (a.depth - l))) + (idx >> l)) * E * 8
                                  : a.run + (u * (a.depth - 1) + (l - 1)) * E * 8;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      ps_get_words(p + e * 8, prev[e]);
      ps_get_words(a.siblings + ((u * a.depth + l) * E + e) * 8, sib[e]);
      if (l == 0) {                                          // "assign leaf (hash, balance)"; instance rows 0 .. E - 1
        ps_put_words(adv + e * col_words + e * 8, prev[e]);
        ps_put_words(inst + e * 8, prev[e]);
      }
      // "merkle prove layer" row 0: previous node, sibling, index
      ps_put_words(adv + e * col_words + base * 8, prev[e]);
      ps_put_words(adv + (E + e) * col_words + base * 8, sib[e]);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        kids[e][i] = right ? sib[e][i] : prev[e][i];
        kids[E + e][i] = right ? prev[e][i] : sib[e][i];
      }
    }
    fr_small_to_ext(right ? 1u : 0u, w);
    ps_put_words(adv + 2 * E * col_words + base * 8, w);
  }
  // row 1: left, right (the hash's message)
#pragma unroll
  for (int j = 0; j < 2 * E; ++j) ps_put_words(adv + j * col_words + (base + 1) * 8, kids[j]);
  if constexpr (E == 2) {                                    // and the sum of their balances
    uint32_t sum[8];
    fr_add_ext(kids[1], kids[3], sum);
    ps_put_words(adv + 4 * col_words + (base + 1) * 8, sum);
    if (l + 1 == a.depth) {
      merkle_sum_lt_row(adv + (uint64_t)lay.lt_row * 8, col_words, sum, a.assets);
      ps_put_words(inst + 24, a.assets);
    }
  }
  Fr s[W];
  pow5_hash_rows<W>(adv + W * col_words + (base + 2) * 8, col_words, kids, a.consts, a.r_f, a.r_p, s);
  if (l + 1 == a.depth) {                                    // the root: instance row E
    fe_to_ext_shift(w, s[0]);
    ps_put_words(inst + E * 8, w);
  }
}

// the whole Poseidon circuit of message u
HM_HD void poseidon_witness_lane(const WitnessArgs& a, uint64_t u) {
  const uint64_t col_words = (uint64_t)8 << a.log_n;
  uint32_t* adv = a.advice + u * witness_advice(0) * col_words;
  uint32_t msg[4][8], w[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ps_get_words(a.leaves + (u * 4 + j) * 8, msg[j]);
    ps_put_words(adv + j * col_words + 0 * 8, msg[j]);     // "load private inputs"
    ps_put_words(adv + j * col_words + 1 * 8, msg[j]);     // "copy input cells to hash input cells"
  }
  Fr s[5];
  pow5_hash_rows<5>(adv + 2 * 8, col_words, msg, a.consts, a.r_f, a.r_p, s);
  fe_to_ext_shift(w, s[0]);
  ps_put_words(a.instance + u * 8, w);
}
