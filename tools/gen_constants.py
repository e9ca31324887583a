#!/usr/bin/env python3
"""Generate halo2-experiments_amd/csrc/bn256_constants.inc: 29-bit-limb constants for Fq / Fr.

The device field layer keeps elements as 9 unsaturated limbs of 29 bits (261-bit container) in
Montgomery form with radix 2^261 ("internal" form).  The reference's memory format (SURVEY.md
§8a) is 4 x u64 Montgomery with radix 2^256 ("external" form).  This script derives every
constant from the two moduli; nothing here is copied from any implementation.
"""
import os

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
W, NL = 29, 9
MASK = (1 << W) - 1
RADIX = 1 << (W * NL)  # 2^261


def limbs(v):
    out = [(v >> (W * i)) & MASK for i in range(NL - 1)]
    out.append(v >> (W * (NL - 1)))
    assert out[-1] < (1 << 32)
    return out


def spread(k, mod, bits):
    """k*mod written with limb i raised by 2^bits borrowed from limb i+1 (value unchanged)."""
    c = limbs(k * mod)
    b = 1 << (bits - W)
    s = [c[0] + (1 << bits)] + [c[i] + (1 << bits) - b for i in range(1, NL - 1)] + [c[NL - 1] - b]
    assert sum(x << (W * i) for i, x in enumerate(s)) == k * mod
    assert all(0 <= x < (1 << 32) for x in s), (k, bits, s)
    return s


def arr(name, vals):
    return "  static constexpr uint32_t %s[9] = {%s};\n" % (name, ", ".join("0x%08xu" % v for v in vals))


def field(name, mod):
    out = "struct %s {\n" % name
    out += arr("MOD", limbs(mod))
    out += "  static constexpr uint32_t INV29 = 0x%08xu;  // -MOD^-1 mod 2^29\n" % ((-pow(mod, -1, 1 << W)) % (1 << W))
    out += arr("ONE", limbs(RADIX % mod))                      # internal Montgomery one
    out += arr("EXT2INT", limbs((1 << 266) % mod))             # mont_mul(x_ext, .) = x * 2^261
    out += arr("INT2EXT", limbs((1 << 256) % mod))             # mont_mul(x_int, .) = x * 2^256
    out += arr("R2INT", limbs((1 << 522) % mod))               # mont_mul(x_plain, .) = x * 2^261
    # the high half of a 512-bit integer lo + hi * 2^256 (a Blake2b digest reduced into a challenge, csrc/transcript.inc):
    # mont_mul(hi_plain, .) = hi * 2^778 * 2^-261 = (hi * 2^256) * 2^261, the internal form of hi's contribution
    out += "  // WIDE2INT = 2^778 mod MOD: mont_mul(hi, .) = hi * 2^778 * 2^-261 = (hi * 2^256) * 2^261, the high half of lo + hi * 2^256\n"
    out += arr("WIDE2INT", limbs((1 << 778) % mod))
    for k, bits in [(3, 29), (4, 29), (6, 30), (8, 30), (10, 30), (12, 30), (16, 30), (20, 31), (24, 31), (32, 31)]:
        out += arr("SUB%d_%d" % (k, bits), spread(k, mod, bits))
    # 32-bit packed limbs (8 x u32) of mod, for the final canonical conditional subtraction
    out += "  static constexpr uint32_t MOD32[8] = {%s};\n" % ", ".join("0x%08xu" % ((mod >> (32 * i)) & 0xFFFFFFFF) for i in range(8))
    out += "  static constexpr uint32_t TOPMOD = %du;      // MOD >> 232\n" % (mod >> 232)
    out += "  static constexpr uint32_t QK = %du;  // floor(2^53 / (TOPMOD + 1))\n" % ((1 << 53) // ((mod >> 232) + 1))
    # a small plain integer l < 2^16 into external form without a Montgomery product (csrc/range.inc): l * INT2EXT - q * MOD with
    # q = (l * EXTQ32) >> 32, which is floor(l * INT2EXT / MOD) or one less
    out += "  static constexpr uint32_t EXTQ32 = %du;  // floor((2^256 mod MOD) * 2^32 / MOD)\n" % ((((1 << 256) % mod) << 32) // mod)
    out += "};\n"
    return out


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = f2_mul(acc, acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


def pairing_constants():
    """The constants of csrc/pairing.inc over Fq2 = Fq[u] / (u^2 + 1), xi = 9 + u, in the internal form of Fq: what the coefficient
    of w^k picks up under the Frobenius maps p, p^2, p^3 (w^p = w xi^((p - 1) / 6), so gamma_k = xi^(k (p - 1) / 6); twice:
    gamma_k conj(gamma_k); three times: that times gamma_k), the twist's b' = 3 / xi, and 9 and -1 for the product by xi."""
    xi = (9, 1)
    conj = lambda a: (a[0], -a[1] % P)
    rows = []
    gamma = [f2_pow(xi, k * (P - 1) // 6) for k in range(6)]
    for n in (1, 2, 3):
        for k in range(6):
            g = gamma[k]
            c = g if n == 1 else f2_mul(g, conj(g)) if n == 2 else f2_mul(f2_mul(g, conj(g)), g)
            rows += [c[0], c[1]]
    xi_inv = f2_pow(xi, P * P - 2)
    assert f2_mul(xi, xi_inv) == (1, 0)
    b = f2_mul((3, 0), xi_inv)
    internal = lambda v: limbs(v * RADIX % P)
    out = "struct PairingParams {\n"
    out += arr("NINE", internal(9)) + arr("MINUS1", internal(P - 1))
    out += arr("TWIST_B0", internal(b[0])) + arr("TWIST_B1", internal(b[1]))
    out += "  // FROB[((n - 1) * 6 + k) * 2 + c]: component c of the factor of w^k under the Frobenius map p^n\n"
    out += "  static constexpr uint32_t FROB[36][9] = {\n"
    for v in rows:
        out += "    {%s},\n" % ", ".join("0x%08xu" % x for x in internal(v))
    out += "  };\n};\n"
    return out


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "..", "halo2-experiments_amd", "csrc", "bn256_constants.inc")
    txt = "// GENERATED by tools/gen_constants.py -- do not edit.\n"
    txt += "// 29-bit-limb constants of the BN256 base field Fq and scalar field Fr.\n"
    txt += field("FqParams", P) + field("FrParams", R) + pairing_constants()
    with open(dst, "w") as f:
        f.write(txt)
    print("wrote", os.path.normpath(dst))


if __name__ == "__main__":
    main()
