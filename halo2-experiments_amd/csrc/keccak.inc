// keccak.inc -- Keccak-256 on the device, one lane per message, and on it the EVM-style transcript of a batch of proofs, one lane per
// proof, with the uncompressed read of such proofs (batch_verifier.py with encoding="evm" is the caller; transcript.py states the rules):
//
//   permute    keccak_f1600: theta, rho, pi and chi of ONE round written out with literal offsets, so that the 25 lanes of the state are
//              only ever indexed by constants and stay in registers; the 24 rounds are a rolled loop whose only run-time index is into
//              the round constants.
//   absorber   KcState holds the 25 lanes and the write position; the 136-byte block of a lane lies OUTSIDE the registers, 34 words
//              behind a KcBuf (word i at w[i * T]: a column of an LDS array on the device, plain words on the host), because the
//              position is a run-time value and an XOR into A[pos] would send the state to scratch.  A block is XOR-ed into the state
//              at constant indices, whole, when it is full (kc_push_word / kc_push) or at the padding (kc_pad_permute).  Unlike
//              Blake2b a full block is absorbed at once: a message that ends on a block boundary pads a block of its own.
//   words      everything the transcript absorbs is whole 32-byte words, so its lane knows kc_push_word only; kc_push, with the
//              one-word shifter for single bytes, serves kc_hash_lane alone (messages of any length and alignment).
//   squeeze    kc_squeeze_restart: buf = everything absorbed since the last squeeze (the previous digest first); data = buf, and one
//              byte 0x01 behind it if and only if len(buf) == 32 -- the state remembers whether a block was absorbed since, so the
//              rule hangs on the LENGTH, not on what the previous operation was --; the padding 0x01 .. 0x80 follows at once, the state
//              is permuted, the digest is its first 32 bytes, and the sponge restarts with the digest as the first 32 bytes of buf.
//   challenge  kc_challenge: the digest read as a BIG-endian integer, any 256-bit word, times R2INT: its residue mod r as the 4
//              Montgomery words the terms kernel reads.
//   read       evm_point_one / evm_scalar_one: 32 big-endian bytes per coordinate or scalar, byte-reversed, checked < p and on the curve
//              (g1_codec.inc), or < r, into the words hm_verify_read_proofs_dev leaves for the same point or scalar.  No square root.
//   lane       evm_proof_one: the preamble words of proof b, then the schedule's (absorb a slots, squeeze s challenges) pairs over the
//              proof's slots, absorbed verbatim.  One kc_push_word site and one kc_squeeze_restart site: the permutation is inlined
//              twice per kernel.
// Included inside namespace hm by verify.hip, which holds the three kernels and their drivers, behind g1_codec.inc, verify_read.inc and
// transcript.inc (the schedule's check); the lane functions are host-callable: host_check.cpp includes this file and runs them with
// the bound tracking on.

constexpr uint32_t KC_THREADS = 64;                              // one wave per block: 8.5 KiB of LDS, no barrier anywhere
constexpr uint32_t KC_RATE = 136, KC_BLOCK_WORDS = 34;           // the rate of Keccak-256 in bytes and in 32-bit words (17 lanes)
constexpr uint32_t KC_DOMAIN = 0x01;                             // Keccak's padding byte (SHA-3's is 0x06)
// the slot table of an "evm" layout: bit 31 a point (its x slot; y is the next slot), bit 30 the tail, bits 0 .. 29 the index; the
// second slot of a point carries EVM_SKIP and is read by the lane of the first
constexpr uint32_t EVM_POINT = 1u << 31, EVM_TAIL = 1u << 30, EVM_SKIP = 1u << 29, EVM_INDEX = EVM_SKIP - 1u;

struct KcRc {
  static constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
};

HM_HD uint64_t kc_rotl(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

#define HM_KC_THETA(x) \
  A[x] ^= D##x, A[x + 5] ^= D##x, A[x + 10] ^= D##x, A[x + 15] ^= D##x, A[x + 20] ^= D##x;
#define HM_KC_CHI(y)                                  \
  A[y + 0] = B[y + 0] ^ (~B[y + 1] & B[y + 2]);      \
  A[y + 1] = B[y + 1] ^ (~B[y + 2] & B[y + 3]);      \
  A[y + 2] = B[y + 2] ^ (~B[y + 3] & B[y + 4]);      \
  A[y + 3] = B[y + 3] ^ (~B[y + 4] & B[y + 0]);      \
  A[y + 4] = B[y + 4] ^ (~B[y + 0] & B[y + 1]);

// Keccak-f[1600] on lane x + 5 y at A[x + 5 y]
HM_HD void keccak_f1600(uint64_t (&A)[25]) {
  for (int round = 0; round < 24; ++round) {
    const uint64_t C0 = A[0] ^ A[5] ^ A[10] ^ A[15] ^ A[20], C1 = A[1] ^ A[6] ^ A[11] ^ A[16] ^ A[21];
    const uint64_t C2 = A[2] ^ A[7] ^ A[12] ^ A[17] ^ A[22], C3 = A[3] ^ A[8] ^ A[13] ^ A[18] ^ A[23];
    const uint64_t C4 = A[4] ^ A[9] ^ A[14] ^ A[19] ^ A[24];
    const uint64_t D0 = C4 ^ kc_rotl(C1, 1), D1 = C0 ^ kc_rotl(C2, 1), D2 = C1 ^ kc_rotl(C3, 1), D3 = C2 ^ kc_rotl(C4, 1);
    const uint64_t D4 = C3 ^ kc_rotl(C0, 1);
    HM_KC_THETA(0) HM_KC_THETA(1) HM_KC_THETA(2) HM_KC_THETA(3) HM_KC_THETA(4)
    uint64_t B[25];                                              // rho and pi: B[y + 5 ((2 x + 3 y) % 5)] = rotl(A[x + 5 y], r[x][y])
    B[0] = A[0], B[10] = kc_rotl(A[1], 1), B[20] = kc_rotl(A[2], 62), B[5] = kc_rotl(A[3], 28), B[15] = kc_rotl(A[4], 27);
    B[16] = kc_rotl(A[5], 36), B[1] = kc_rotl(A[6], 44), B[11] = kc_rotl(A[7], 6), B[21] = kc_rotl(A[8], 55), B[6] = kc_rotl(A[9], 20);
    B[7] = kc_rotl(A[10], 3), B[17] = kc_rotl(A[11], 10), B[2] = kc_rotl(A[12], 43), B[12] = kc_rotl(A[13], 25), B[22] = kc_rotl(A[14], 39);
    B[23] = kc_rotl(A[15], 41), B[8] = kc_rotl(A[16], 45), B[18] = kc_rotl(A[17], 15), B[3] = kc_rotl(A[18], 21), B[13] = kc_rotl(A[19], 8);
    B[14] = kc_rotl(A[20], 18), B[24] = kc_rotl(A[21], 2), B[9] = kc_rotl(A[22], 61), B[19] = kc_rotl(A[23], 56), B[4] = kc_rotl(A[24], 14);
    HM_KC_CHI(0) HM_KC_CHI(5) HM_KC_CHI(10) HM_KC_CHI(15) HM_KC_CHI(20)
    A[0] ^= KcRc::RC[round];
  }
}
#undef HM_KC_THETA
#undef HM_KC_CHI

// the 136-byte block of one lane: word i at w[i * T]
struct KcBuf {
  uint32_t* w;
  uint32_t T;
};
// pos: the bytes in the block, 0 .. 135 (a full block is absorbed at once);  spilled: a block was absorbed since the last restart, so
// what was absorbed since is longer than 32 bytes whatever pos says
struct KcState {
  uint64_t A[25];
  uint32_t pos;
  bool spilled;
};

HM_HD void kc_init(KcState& s) {
#pragma unroll
  for (int i = 0; i < 25; ++i) s.A[i] = 0;
  s.pos = 0;
  s.spilled = false;
}

// the full block behind buf into the state, and the permutation
HM_HD void kc_absorb_block(KcState& s, const KcBuf& buf) {
#pragma unroll
  for (int i = 0; i < 17; ++i) s.A[i] ^= (uint64_t)buf.w[(size_t)(2 * i) * buf.T] | ((uint64_t)buf.w[(size_t)(2 * i + 1) * buf.T] << 32);
  keccak_f1600(s.A);
  s.pos = 0;
  s.spilled = true;
}

// append the 4 bytes of w (little-endian) at a position that is a multiple of 4
HM_HD void kc_push_word(KcState& s, const KcBuf& buf, uint32_t w) {
  buf.w[(size_t)(s.pos >> 2) * buf.T] = w;
  s.pos += 4;
  if (s.pos == KC_RATE) kc_absorb_block(s, buf);
}

// append the low nb bytes of w, nb = 1 or 4 (w < 2^(8 nb)), at any position.  part: the pos % 4 bytes of word pos / 4 that are not yet
// stored (zero when pos % 4 == 0).  The rate is a multiple of 4, so a word that straddles two blocks completes the last word of the
// first (its low bytes) and leaves its high bytes as the part of the next.
HM_HD void kc_push(KcState& s, const KcBuf& buf, uint32_t& part, uint32_t w, uint32_t nb) {
  const uint32_t sh = (s.pos & 3u) * 8u;
  const bool completes = (s.pos & 3u) + nb >= 4u;
  const uint32_t lo = part | (w << sh), hi = sh ? w >> (32u - sh) : 0u;
  if (completes) buf.w[(size_t)(s.pos >> 2) * buf.T] = lo;
  const uint32_t np = s.pos + nb;
  if (np >= KC_RATE) {
    kc_absorb_block(s, buf);
    s.pos = np - KC_RATE;
  } else {
    s.pos = np;
  }
  part = completes ? hi : lo;
}

// pad and permute: the stored words of the block, then `tail` as word pos / 4 -- the bytes not yet stored with the domain byte behind
// them --, zeros, and 0x80 on the block's last byte
HM_HD void kc_pad_permute(KcState& s, const KcBuf& buf, uint32_t tail) {
  const uint32_t whole = s.pos >> 2;                             // <= 33
#pragma unroll
  for (int i = 0; i < 17; ++i) {
    const uint32_t a = 2 * i, b = 2 * i + 1;
    const uint32_t wa = a < whole ? buf.w[(size_t)a * buf.T] : a == whole ? tail : 0u;
    uint32_t wb = b < whole ? buf.w[(size_t)b * buf.T] : b == whole ? tail : 0u;
    if (i == 16) wb ^= 0x80000000u;
    s.A[i] ^= (uint64_t)wa | ((uint64_t)wb << 32);
  }
  keccak_f1600(s.A);
}

// Keccak-256 (domain byte `domain`) of len bytes at msg (any alignment: whole words are read where the address allows it) -> 8 words
HM_HD void kc_hash_lane(const KcBuf& buf, const uint8_t* msg, uint32_t len, uint32_t domain, uint32_t* out8) {
  KcState s;
  kc_init(s);
  uint32_t part = 0, at = 0;
  const bool aligned = ((uintptr_t)msg & 3u) == 0;
  while (at < len) {
    uint32_t w, nb;
    if (aligned && at + 4u <= len) {
      w = *reinterpret_cast<const uint32_t*>(msg + at);
      nb = 4;
    } else {
      w = msg[at];
      nb = 1;
    }
    kc_push(s, buf, part, w, nb);
    at += nb;
  }
  kc_pad_permute(s, buf, part | (domain << ((s.pos & 3u) * 8u)));
#pragma unroll
  for (int i = 0; i < 4; ++i) out8[2 * i] = (uint32_t)s.A[i], out8[2 * i + 1] = (uint32_t)(s.A[i] >> 32);
}

// The transcript's squeeze, on whole words: -> the digest as 8 little-endian words, and the sponge restarted on it
HM_HD void kc_squeeze_restart(KcState& s, const KcBuf& buf, uint32_t (&digest)[8]) {
  const bool lone = !s.spilled && s.pos == 32u;                   // len(buf) == 32: one byte 0x01 of DATA, then the padding's 0x01
  kc_pad_permute(s, buf, lone ? 0x0101u : KC_DOMAIN);
#pragma unroll
  for (int i = 0; i < 4; ++i) digest[2 * i] = (uint32_t)s.A[i], digest[2 * i + 1] = (uint32_t)(s.A[i] >> 32);
  kc_init(s);
#pragma unroll
  for (int i = 0; i < 8; ++i) buf.w[(size_t)i * buf.T] = digest[i];
  s.pos = 32;
}

HM_HD uint32_t kc_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// 32 big-endian bytes, as 8 words in memory order -> the 8 little-endian words of the integer
HM_HD void kc_be_words(const uint32_t (&in)[8], uint32_t (&out)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = kc_bswap(in[7 - k]);
}

// a digest read big-endian, ANY 256-bit integer -> its residue mod r as Montgomery words: v R2INT 2^-261 = v 2^261, the internal form
HM_HD void kc_challenge(const uint32_t (&digest)[8], uint32_t (&out)[8]) {
  uint32_t v[8];
  kc_be_words(digest, v);
  fe_to_ext(out, fe_mul(fe_unpack<FrParams>(v), fe_const<FrParams>(FrParams::R2INT)));
}

// 32 big-endian bytes -> Montgomery words; false (and zeros) for a value not below r
HM_HD bool evm_scalar_one(const uint32_t (&in)[8], uint32_t (&out)[8]) {
  uint32_t v[8];
  kc_be_words(in, v);
  return proof_scalar_one(v, out);
}

// 64 bytes, x then y big-endian -> affine Montgomery words; false (and zeros) for a coordinate >= p or a point off y^2 = x^3 + 3,
// which the 64 zero bytes are
HM_HD bool evm_point_one(const uint32_t (&inx)[8], const uint32_t (&iny)[8], uint32_t (&ox)[8], uint32_t (&oy)[8]) {
  uint32_t vx[8], vy[8];
  kc_be_words(inx, vx);
  kc_be_words(iny, vy);
#pragma unroll
  for (int k = 0; k < 8; ++k) ox[k] = oy[k] = 0;
  if (!fq_words_canonical(vx) || !fq_words_canonical(vy)) return false;
  const Fq x = fe_mul(fe_unpack<FqParams>(vx), fe_const<FqParams>(FqParams::R2INT));   // as g1_decompress_one: v 2^261
  const Fq y = fe_mul(fe_unpack<FqParams>(vy), fe_const<FqParams>(FqParams::R2INT));
  if (!fq_equal(fe_canonical(fe_sqr(y)), fe_canonical(g1_curve_rhs(x)))) return false;   // (0, 0): 0 != 3
  fe_to_ext(ox, x);
  fe_to_ext(oy, y);
  return true;
}

// The transcript of one proof: n_pre preamble words of 32 bytes, then the schedule's pairs over the proof's slots, 8 words each,
// verbatim; challenge j -> rec[8 j ..].  The schedule was checked by the caller: its absorbed slots sum to the proof's slots.
HM_HD void evm_challenges_lane(const KcBuf& buf, const uint32_t* proof, const uint32_t* preamble, uint32_t n_pre, const uint32_t* sched,
                               uint32_t n_pairs, uint32_t* rec) {
  KcState s;
  kc_init(s);
  uint32_t pre = 0, pair = 0, left_absorb = 0, left_squeeze = 0, slot = 0, chal = 0;
  for (;;) {
    const uint32_t* from;
    if (pre < n_pre) {
      from = preamble + (size_t)pre * 8;
      ++pre;
    } else if (left_absorb) {
      from = proof + (size_t)slot * 8;
      ++slot, --left_absorb;
    } else if (left_squeeze) {
      from = nullptr;
      --left_squeeze;
    } else {
      if (pair == n_pairs) break;
      left_absorb = sched[2 * pair], left_squeeze = sched[2 * pair + 1];
      ++pair;
      continue;
    }
    if (from) {
#pragma unroll 1
      for (uint32_t k = 0; k < 8; ++k) kc_push_word(s, buf, from[k]);   // rolled: one site of the permutation, not eight
    } else {
      uint32_t digest[8], out[8];
      kc_squeeze_restart(s, buf, digest);
      kc_challenge(digest, out);
#pragma unroll
      for (int k = 0; k < 8; ++k) rec[(size_t)chal * 8 + k] = out[k];
      ++chal;
    }
  }
}

// Proof b of a batch: a proof flagged on entry is not hashed; a preamble count above the stride flags the proof and reads nothing.
// A flagged proof gets zero challenges; the row's elements behind the schedule's challenges are left alone.
HM_HD void evm_proof_one(const KcBuf& buf, size_t b, const uint32_t* proofs, uint32_t slots, const uint32_t* preamble, const uint32_t* counts,
                         uint32_t stride, const uint32_t* sched, uint32_t n_pairs, uint32_t* bad, uint32_t* records, uint32_t record_elems) {
  uint32_t* rec = records + b * record_elems * 8;
  const uint32_t n_pre = counts[b];
  const bool ok = bad[b] == 0 && n_pre <= stride;
  if (ok) {
    evm_challenges_lane(buf, proofs + b * slots * 8, preamble + b * stride * 8, n_pre, sched, n_pairs, rec);
  } else {
    uint32_t challenges = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) challenges += sched[2 * p + 1];
    for (uint32_t i = 0; i < challenges * 8; ++i) rec[i] = 0;
    bad[b] = 1;
  }
}

// Slot `slot` of a proof of `slots` 32-byte slots (8 words each at `proof`), by its table entry: a point's x slot reads the y slot
// behind it and writes 16 words to its row of points (or to tail); a scalar slot writes 8 words; a y slot (EVM_SKIP) does nothing.
// -> false for a slot that cannot be read (zeros are left) or an entry outside its array (nothing is read or written).
HM_HD bool evm_read_slot(const uint32_t* proof, uint32_t slot, uint32_t slots, uint32_t entry, uint32_t own_points, uint32_t n_scalars,
                         uint32_t* points_row0, uint32_t* tail_row, uint32_t* scalars_row0) {
  const uint32_t index = entry & EVM_INDEX;
  uint32_t a[8], o1[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = proof[(size_t)slot * 8 + k];
  if (entry & EVM_POINT) {
    const bool in_tail = (entry & EVM_TAIL) != 0;
    if (slot + 1 >= slots || (!in_tail && index >= own_points)) return false;
    uint32_t c[8], o2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = proof[(size_t)(slot + 1) * 8 + k];
    const bool ok = evm_point_one(a, c, o1, o2);
    uint32_t* dst = in_tail ? tail_row : points_row0 + (size_t)index * 16;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = o1[k], dst[8 + k] = o2[k];
    return ok;
  }
  if (entry & EVM_SKIP) return true;
  if (index >= n_scalars) return false;
  const bool ok = evm_scalar_one(a, o1);
#pragma unroll
  for (int k = 0; k < 8; ++k) scalars_row0[(size_t)index * 8 + k] = o1[k];
  return ok;
}
