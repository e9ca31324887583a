// digest.hip -- the keyed digest of a host array that keys the drop-in MSM's converted-base cache (capi_msm.hip: msm_host_one).
#include <chrono>
#include <random>

#include "hm_internal.h"

namespace hm {

// Keyed digest of a host array over EVERY word.  It keys the converted-base cache of the drop-in call: unlike round 1's
// 64-point probe it reads the whole array, so a buffer that was mutated at any index -- or re-allocated at the same
// address with other contents -- hashes differently.  The patched best_multiexp also serves the verifier, whose base
// array holds prover-chosen commitments, so an unkeyed mixing function would let a third party construct two arrays
// with one digest.  This one is a universal hash under a per-process random key the caller of the library never sees:
//   inner  NH (UMAC): per 512-byte block  sum_j (m[2j] + k[2j]) * (m[2j+1] + k[2j+1])  mod 2^128 -- two equal-length
//          blocks that differ collide with probability 2^-64 over the key
//   outer  the 128-bit block values as three coefficients each of two polynomials over GF(2^61 - 1), evaluated at two
//          secret points (Horner): a difference anywhere survives with probability 1 - (3 blocks / 2^61)^2
// ~1 multiplication per 16 bytes: as fast as the multiply-rotate lanes it replaces (the digest must stay cheaper than
// the upload it saves).
namespace {
constexpr uint64_t kP61 = (1ull << 61) - 1;
inline uint64_t mulmod61(uint64_t a, uint64_t b) {
  const unsigned __int128 t = (unsigned __int128)a * b;
  uint64_t r = (uint64_t)(t & kP61) + (uint64_t)(t >> 61);
  r = (r & kP61) + (r >> 61);
  return r >= kP61 ? r - kP61 : r;
}
inline uint64_t addmod61(uint64_t a, uint64_t b) {
  uint64_t r = a + b;             // both < 2^61
  return r >= kP61 ? r - kP61 : r;
}
struct DigestKey {
  uint64_t nh[64];
  uint64_t r1, r2, s1, s2;
};
const DigestKey& digest_key() {
  static const DigestKey key = [] {
    DigestKey k;
    uint64_t seed[8];
    try {
      std::random_device rd;
      for (auto& w : seed) w = ((uint64_t)rd() << 32) ^ rd();
    } catch (...) {             // no entropy source: address-space layout and the clock still differ per process
      const uint64_t t = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
      for (int i = 0; i < 8; ++i) seed[i] = t * (2 * i + 1) ^ (uint64_t)(uintptr_t)&k ^ (0x9E3779B97F4A7C15ULL * (i + 1));
    }
    uint64_t x = seed[0] ^ seed[1] ^ seed[2] ^ seed[3] ^ seed[4] ^ seed[5] ^ seed[6] ^ seed[7], y = seed[3] * 3 + seed[5];
    auto next = [&]() {        // splitmix64 over the seeded state: expands the entropy, adds none
      x += 0x9E3779B97F4A7C15ULL + y;
      uint64_t z = x;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
      return z ^ (z >> 31);
    };
    for (auto& w : k.nh) w = next();
    k.r1 = next() % (kP61 - 2) + 1; k.r2 = next() % (kP61 - 2) + 1;
    k.s1 = next() % (kP61 - 2) + 1; k.s2 = next() % (kP61 - 2) + 1;
    return k;
  }();
  return key;
}
}  // namespace

// digest of words [0, count): out = { poly1, poly2 } (both < 2^61)
static void digest_words(const uint64_t* w, size_t count, uint64_t out[2]) {
  const DigestKey& K = digest_key();
  uint64_t a1 = 0, a2 = 0;
  auto absorb = [&](unsigned __int128 nh) {
    const uint64_t lo = (uint64_t)nh, hi = (uint64_t)(nh >> 64);
    const uint64_t c0 = lo & kP61, c1 = ((lo >> 61) | (hi << 3)) & kP61, c2 = hi >> 58;
    a1 = addmod61(mulmod61(addmod61(mulmod61(addmod61(mulmod61(a1, K.r1), c0), K.r1), c1), K.r1), c2);
    a2 = addmod61(mulmod61(addmod61(mulmod61(addmod61(mulmod61(a2, K.r2), c0), K.r2), c1), K.r2), c2);
  };
  size_t i = 0;
  for (; i + 64 <= count; i += 64) {
    unsigned __int128 nh = 0;
    for (int j = 0; j < 64; j += 2) nh += (unsigned __int128)(w[i + j] + K.nh[j]) * (w[i + j + 1] + K.nh[j + 1]);
    absorb(nh);
  }
  if (i < count) {                               // last, partial block: zero-padded (the length is part of the key)
    uint64_t pad[64] = {};
    std::memcpy(pad, w + i, (count - i) * 8);
    unsigned __int128 nh = 0;
    for (int j = 0; j < 64; j += 2) nh += (unsigned __int128)(pad[j] + K.nh[j]) * (pad[j + 1] + K.nh[j + 1]);
    absorb(nh);
  }
  out[0] = a1;
  out[1] = a2;
}

void digest_bases(const uint64_t* bases, size_t n, uint64_t out[4]) {
  hm_fault_point("digest");
  const size_t words = n * 8;
  const unsigned parts = words >= (1u << 20) ? 4u : 1u;      // >= 8 MiB: four host threads (the digest must stay cheaper than the upload)
  uint64_t part[4][2] = {};
  auto lo_of = [&](unsigned p) { return (words * p / parts) & ~(size_t)63; };    // block-aligned cuts
  auto run = [&](unsigned p) {
    const size_t lo = lo_of(p), hi = p + 1 == parts ? words : lo_of(p + 1);
    digest_words(bases + lo, hi - lo, part[p]);
  };
  {
    JoinOnExit pool;                              // joined before `part` is read, and on every other way out
    bool done[4] = {true, false, false, false};
    for (unsigned p = 1; p < parts; ++p) done[p] = spawn_or_false(pool, "digest_spawn", [&run, p] { run(p); });
    run(0);
    for (unsigned p = 1; p < parts; ++p)
      if (!done[p]) run(p);                       // no thread to be had: this one does the part too
  }
  const DigestKey& K = digest_key();
  uint64_t h1 = 0, h2 = 0;
  for (unsigned p = 0; p < parts; ++p) {
    h1 = addmod61(mulmod61(h1, K.s1), part[p][0]);
    h2 = addmod61(mulmod61(h2, K.s2), part[p][1]);
  }
  out[0] = h1;
  out[1] = h2;
  out[2] = (uint64_t)words;
  out[3] = parts;
}


}  // namespace hm
