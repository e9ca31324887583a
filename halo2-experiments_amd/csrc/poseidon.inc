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

// the permutation on WIDTH words in internal form (normalised, product outputs or constants); c = the spec's constant block
template <int W>
HM_HD void poseidon_permute(Fr (&s)[W], const uint32_t* c, uint32_t r_f, uint32_t r_p) {
  const uint32_t rounds = r_f + r_p, half = r_f >> 1;
  const uint32_t* mds = c + (size_t)rounds * W * 9;
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; ++r) {
    const bool full = r < half || r >= half + r_p;     // the same in every lane
    const uint32_t* rc = c + (size_t)r * W * 9;
    Fr x[W];
#pragma unroll
    for (int j = 0; j < W; ++j) x[j] = fe_add(s[j], ps_load9(rc + j * 9));
    x[0] = poseidon_sbox(x[0]);
    if (full)
      poseidon_sbox_rest<W>(x, std::make_integer_sequence<int, W - 1>{});
    else
      poseidon_norm_rest<W>(x, std::make_integer_sequence<int, W - 1>{});
    poseidon_mix<W>(s, mds, x, std::make_integer_sequence<int, W>{});
  }
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
#endif
