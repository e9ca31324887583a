// transcript.inc -- Blake2b-512 on the device, one lane per message, and on it the verifier's transcript of a batch of proofs, one lane
// per proof (batch_verifier.py with transcript="device" is the caller; transcript.py states the transcript's rules):
//
//   compress   blake2b_compress: the 12 rounds written out with the message schedule as literals, so that m[] and v[] are only ever
//              indexed by constants and stay in registers (a schedule table indexed at run time would put m[] in scratch).
//   absorber   B2State holds h, the byte counter and the write position; the 128-byte block of a lane lies OUTSIDE the registers, 32
//              words behind a B2Buf (word i at w[i * T]): on the device a column of an LDS array block[32][lanes] -- lanes that write
//              the same word index hit distinct banks --, on the host 32 plain words.  b2_push appends 1 or 4 bytes at any byte
//              offset through a one-word shifter (`part`: the bytes of the word being filled); records are 33 and 65 bytes, so the
//              offset takes every residue mod 4.  The transcript lane stages the 16 words of the record it absorbs in 16 more words
//              of the same column, because it walks them with a run-time index.  A full block is compressed only when another byte
//              arrives (Blake2b's rule: the last block, full or not, is compressed with the final flag).
//   squeeze    b2_final compresses a COPY of h over the block as it stands -- the words behind the position taken as zero, the counter
//              plus the buffered bytes, the final flag -- and leaves state and block untouched: the running state keeps the prefix
//              byte of the squeeze, and two squeezes in a row differ.
//   wide       fr_from_wide: the 64 digest bytes as a little-endian integer lo + hi 2^256, reduced mod r into the 4 Montgomery
//              words the terms kernel reads (Challenge255 / from_bytes_wide).
//   lane       tr_proof_one: the preamble scalars of proof b (prefix 2), then the schedule's (absorb a slots, squeeze s challenges)
//              pairs over the proof's slots; a point slot absorbs prefix 1, x (the proof's bytes without the sign bit) and the y bytes
//              the read kernel left, a scalar slot prefix 2 and its bytes.  Every record goes through ONE b2_push site and every
//              squeeze through ONE b2_final site: the compression is inlined twice per kernel, not once per kind of record.
// Included inside namespace hm by verify.hip, which holds the two kernels and their drivers, and by capi_verify.hip for the schedule's
// check; the lane functions are host-callable: host_check.cpp includes this file and runs them with the bound tracking on.

constexpr uint32_t TR_THREADS = 64;                              // one wave per block: 8 or 12 KiB of LDS, no barrier anywhere
constexpr uint32_t TR_SCALAR = 2, TR_POINT = 1, TR_CHALLENGE = 0;   // the prefix bytes (transcript.py)
constexpr uint64_t TR_PERSONAL_LO = 0x72542d326f6c6148ull, TR_PERSONAL_HI = 0x7470697263736e61ull;   // b"Halo2-Transcript"
constexpr uint32_t TR_VR_POINT = 1u << 31, TR_VR_INDEX = (1u << 30) - 1u;   // verify_read.inc's slot table bits

struct B2Iv {
  static constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
};

HM_HD uint64_t b2_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

#define HM_B2_G(a, b, c, d, x, y)  \
  v[a] = v[a] + v[b] + (x);        \
  v[d] = b2_rotr(v[d] ^ v[a], 32); \
  v[c] = v[c] + v[d];              \
  v[b] = b2_rotr(v[b] ^ v[c], 24); \
  v[a] = v[a] + v[b] + (y);        \
  v[d] = b2_rotr(v[d] ^ v[a], 16); \
  v[c] = v[c] + v[d];              \
  v[b] = b2_rotr(v[b] ^ v[c], 63);
#define HM_B2_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  HM_B2_G(0, 4, 8, 12, m[s0], m[s1])                                                       \
  HM_B2_G(1, 5, 9, 13, m[s2], m[s3])                                                       \
  HM_B2_G(2, 6, 10, 14, m[s4], m[s5])                                                      \
  HM_B2_G(3, 7, 11, 15, m[s6], m[s7])                                                      \
  HM_B2_G(0, 5, 10, 15, m[s8], m[s9])                                                      \
  HM_B2_G(1, 6, 11, 12, m[s10], m[s11])                                                    \
  HM_B2_G(2, 7, 8, 13, m[s12], m[s13])                                                     \
  HM_B2_G(3, 4, 9, 14, m[s14], m[s15])

// h <- F(h, m, t, last): one 128-byte block m (16 little-endian words), t the bytes absorbed up to and including it (below 2^64)
HM_HD void blake2b_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = h[i], v[8 + i] = B2Iv::IV[i];
  v[12] ^= t;
  if (last) v[14] = ~v[14];
  HM_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  HM_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  HM_B2_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  HM_B2_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  HM_B2_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  HM_B2_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  HM_B2_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  HM_B2_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  HM_B2_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  HM_B2_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
  HM_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  HM_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}
#undef HM_B2_ROUND
#undef HM_B2_G

// the 128-byte block of one lane: word i at w[i * T]; the transcript lane keeps TR_STAGE_WORDS more behind it (the record being absorbed)
constexpr uint32_t B2_BLOCK_WORDS = 32, TR_STAGE_WORDS = 16;
struct B2Buf {
  uint32_t* w;
  uint32_t T;
};
// pos: the bytes in the block, 0 .. 128;  part: the pos % 4 bytes of word pos / 4, not yet stored (zero when pos % 4 == 0);  t: the
// bytes compressed so far
struct B2State {
  uint64_t h[8];
  uint64_t t;
  uint32_t pos, part;
};

// digest length 64, no key, fanout and depth 1, the 16 personalisation bytes as two little-endian words (zero: none)
HM_HD void b2_init(B2State& s, uint64_t personal_lo, uint64_t personal_hi) {
#pragma unroll
  for (int i = 0; i < 8; ++i) s.h[i] = B2Iv::IV[i];
  s.h[0] ^= 0x01010040ull;
  s.h[6] ^= personal_lo;
  s.h[7] ^= personal_hi;
  s.t = 0;
  s.pos = s.part = 0;
}

// append the low nb bytes of w, nb = 1 or 4 (w < 2^(8 nb)).  The push completes word pos / 4 when pos % 4 + nb >= 4; with the block
// full (pos = 128), or filled by the first bytes of w, the block is compressed first and what is left of w opens the next one.
HM_HD void b2_push(B2State& s, const B2Buf& buf, uint32_t w, uint32_t nb) {
  const uint32_t pos = s.pos, sh = (pos & 3u) * 8u;
  const bool full = pos == 128u, completes = (pos & 3u) + nb >= 4u;
  const uint32_t lo = s.part | (w << sh), hi = sh ? w >> (32u - sh) : 0u;
  uint32_t np = pos + nb;
  if (!full && completes) buf.w[(size_t)(pos >> 2) * buf.T] = lo;
  if (np > 128u) {
    uint64_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = (uint64_t)buf.w[(size_t)(2 * i) * buf.T] | ((uint64_t)buf.w[(size_t)(2 * i + 1) * buf.T] << 32);
    s.t += 128u;
    blake2b_compress(s.h, m, s.t, false);
    np -= 128u;
  }
  if (full && completes) buf.w[0] = lo;
  s.part = completes ? hi : lo;
  s.pos = np;
}

// the digest of everything pushed so far, as 8 little-endian words; neither the state nor the block changes
HM_HD void b2_final(const B2State& s, const B2Buf& buf, uint64_t (&out)[8]) {
  const uint32_t whole = s.pos >> 2;                             // the words of the block that are stored; word `whole` is `part`
  uint64_t m[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t a = 2 * i, b = 2 * i + 1;
    const uint32_t wa = a < whole ? buf.w[(size_t)a * buf.T] : a == whole ? s.part : 0u;
    const uint32_t wb = b < whole ? buf.w[(size_t)b * buf.T] : b == whole ? s.part : 0u;
    m[i] = (uint64_t)wa | ((uint64_t)wb << 32);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = s.h[i];
  blake2b_compress(out, m, s.t + s.pos, true);
}

// Blake2b-512 of len bytes at msg (any alignment: whole words are read where the address allows it) -> 16 words
HM_HD void b2_hash_lane(const B2Buf& buf, const uint8_t* msg, uint32_t len, uint64_t personal_lo, uint64_t personal_hi, uint32_t* out16) {
  B2State s;
  b2_init(s, personal_lo, personal_hi);
  const bool aligned = ((uintptr_t)msg & 3u) == 0;
  uint32_t at = 0;
  while (at < len) {
    uint32_t w, nb;
    if (aligned && at + 4u <= len) {
      w = *reinterpret_cast<const uint32_t*>(msg + at);
      nb = 4;
    } else {
      w = msg[at];
      nb = 1;
    }
    b2_push(s, buf, w, nb);
    at += nb;
  }
  uint64_t d[8];
  b2_final(s, buf, d);
#pragma unroll
  for (int i = 0; i < 8; ++i) out16[2 * i] = (uint32_t)d[i], out16[2 * i + 1] = (uint32_t)(d[i] >> 32);
}

// 64 digest bytes, a little-endian integer lo + hi 2^256 with lo, hi ANY 256-bit words -> its residue mod r as Montgomery words:
// lo R2INT 2^-261 = lo 2^261 and hi WIDE2INT 2^-261 = hi 2^256 2^261 are the internal forms of the two halves
HM_HD void fr_from_wide(const uint64_t (&d)[8], uint32_t (&out)[8]) {
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo[2 * i] = (uint32_t)d[i], lo[2 * i + 1] = (uint32_t)(d[i] >> 32);
    hi[2 * i] = (uint32_t)d[4 + i], hi[2 * i + 1] = (uint32_t)(d[4 + i] >> 32);
  }
  const Fr a = fe_mul(fe_unpack<FrParams>(lo), fe_const<FrParams>(FrParams::R2INT));
  const Fr b = fe_mul(fe_unpack<FrParams>(hi), fe_const<FrParams>(FrParams::WIDE2INT));
  fe_to_ext(out, fe_reduce_small(fe_norm(fe_add(a, b))));
}

// The transcript of one proof: n_pre preamble scalars, then the schedule's pairs over the proof's slots; challenge j -> rec[8 j ..].
// The schedule was checked by the caller: its absorbed slots sum to the proof's slots.  -> false for a point slot whose table index
// lies outside the proof's points (what it then writes is defined, and discarded by the caller).
HM_HD bool tr_challenges_lane(const B2Buf& buf, const uint32_t* proof, const uint32_t* slot_table, uint32_t n_points, const uint32_t* ybytes,
                              const uint32_t* preamble, uint32_t n_pre, const uint32_t* sched, uint32_t n_pairs, uint32_t* rec) {
  B2State s;
  b2_init(s, TR_PERSONAL_LO, TR_PERSONAL_HI);
  bool ok = true;
  uint32_t pre = 0, pair = 0, left_absorb = 0, left_squeeze = 0, slot = 0, chal = 0;
  for (;;) {
    uint32_t prefix, words = 8;
    const uint32_t *first = proof, *second = proof;
    bool point = false;
    if (pre < n_pre) {
      prefix = TR_SCALAR;
      first = second = preamble + (size_t)pre * 8;
      ++pre;
    } else if (left_absorb) {
      const uint32_t entry = slot_table[slot];
      first = second = proof + (size_t)slot * 8;
      prefix = TR_SCALAR;
      if (entry & TR_VR_POINT) {
        uint32_t index = entry & TR_VR_INDEX;
        if (index >= n_points) ok = false, index = 0;
        point = true, prefix = TR_POINT, words = 16;
        second = ybytes + (size_t)index * 8;
      }
      ++slot, --left_absorb;
    } else if (left_squeeze) {
      prefix = TR_CHALLENGE, words = 0;
      --left_squeeze;
    } else {
      if (pair == n_pairs) break;
      left_absorb = sched[2 * pair], left_squeeze = sched[2 * pair + 1];
      ++pair;
      continue;
    }
    // the record's words wait in the lane's staging words behind the block: the loop below reads them by a run-time index, which
    // registers cannot serve (a private array indexed at run time -- and a chain of selects over one, which the compiler turns back
    // into the array -- goes to scratch)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      buf.w[(size_t)(B2_BLOCK_WORDS + k) * buf.T] = k == 7 && point ? first[k] & 0x7fffffffu : first[k];   // the sign of y is no part of x
      buf.w[(size_t)(B2_BLOCK_WORDS + 8 + k) * buf.T] = second[k];
    }
    for (uint32_t step = 0; step <= words; ++step) {
      const bool head = step == 0;
      b2_push(s, buf, head ? prefix : buf.w[(size_t)(B2_BLOCK_WORDS - 1 + step) * buf.T], head ? 1u : 4u);
    }
    if (words == 0) {
      uint64_t d[8];
      uint32_t out[8];
      b2_final(s, buf, d);
      fr_from_wide(d, out);
#pragma unroll
      for (int k = 0; k < 8; ++k) rec[(size_t)chal * 8 + k] = out[k];
      ++chal;
    }
  }
  return ok;
}

// Proof b of a batch: a proof flagged on entry is not hashed; a preamble count above the stride flags the proof and reads nothing.
// A flagged proof gets zero challenges; the row's elements behind the schedule's challenges are left alone.
HM_HD void tr_proof_one(const B2Buf& buf, size_t b, const uint32_t* proofs, const uint32_t* slot_table, uint32_t slots, uint32_t n_points,
                        const uint32_t* ybytes, const uint32_t* preamble, const uint32_t* counts, uint32_t stride, const uint32_t* sched,
                        uint32_t n_pairs, uint32_t* bad, uint32_t* records, uint32_t record_elems) {
  uint32_t* rec = records + b * record_elems * 8;
  const uint32_t n_pre = counts[b];
  bool ok = bad[b] == 0 && n_pre <= stride;
  if (ok)
    ok = tr_challenges_lane(buf, proofs + b * slots * 8, slot_table, n_points, ybytes + b * n_points * 8, preamble + b * stride * 8, n_pre, sched,
                            n_pairs, rec);
  if (!ok) {
    uint32_t challenges = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) challenges += sched[2 * p + 1];
    for (uint32_t i = 0; i < challenges * 8; ++i) rec[i] = 0;
    bad[b] = 1;
  }
}

// what hm_verify_transcript_dev refuses in a schedule (host memory): null when it is sound
inline const char* tr_schedule_problem(const uint32_t* sched, size_t n_pairs, uint32_t slots, uint32_t record_elems) {
  uint64_t absorbed = 0, squeezed = 0;
  for (size_t p = 0; p < n_pairs; ++p) absorbed += sched[2 * p], squeezed += sched[2 * p + 1];
  if (absorbed != slots) return "transcript: the schedule's absorbed slots do not sum to the proof's slots";
  if (squeezed > record_elems) return "transcript: the schedule squeezes more challenges than a record holds";
  return nullptr;
}
