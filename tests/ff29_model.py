"""The reference of the unit-op tests (test_unit_ops_host.py, test_unit_ops_gpu.py): csrc/ff29.h and csrc/g1.h in Python integers.

A field element is 9 limbs of any size below 2^32 ("lazy" or normalised); value(limbs) = sum l[i] << 29*i, and it stands for
value * 2^-261 mod p.  Everything here is derived from the oracle's two moduli alone -- the limbs of p, -p^-1, ONE = 2^261 mod p,
EXT2INT = 2^266 mod p, INT2EXT = 2^256 mod p, the subtraction constants -- so comparing the C code with it checks
csrc/bn256_constants.inc as well.

Products are exact to the limb: T = (S + M * p) >> 261 with S = A*B [+ C*D] and M = -S * p^-1 mod 2^261; limbs 0..7 are the 29-bit
digits of T and limb 8 is T >> 232.  Operand scanning, product scanning and the lockstep forms all compute this integer as long as
no 64-bit column overflows, which `mont_admissible` states from the operands' actual limb maxima:
9 * (Amax*Bmax [+ Cmax*Dmax]) + 9 * 2^58 + 2^40 < 2^64.  Linear operations are exact limb by limb and the model asserts that
none wraps before it expects anything."""
import re
from fractions import Fraction

from oracle import bn256_ref as o

MASK29 = (1 << 29) - 1
RADIX = 1 << 261
U32 = 1 << 32


def value(limbs) -> int:
    v = 0
    for i, l in enumerate(limbs):
        v += int(l) << (29 * i)
    return v


def digits(v: int):
    """normalised limbs of v < 2^261 + ...: limbs 0..7 the 29-bit digits, limb 8 the rest"""
    assert 0 <= v and (v >> 232) < U32
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def is_normalised(limbs) -> bool:
    return all(int(l) <= MASK29 for l in limbs[:8])


class Field:
    def __init__(self, name: str, index: int, p: int):
        self.name, self.index, self.p = name, index, p
        self.mod = digits(p)
        self.pinv = pow(p, -1, RADIX)
        self.inv29 = (-pow(p, -1, 1 << 29)) % (1 << 29)
        self.one = digits(RADIX % p)
        self.ext2int = digits((1 << 266) % p)
        self.int2ext = digits((1 << 256) % p)
        self.topmod = p >> 232
        self.qk = (1 << 53) // (self.topmod + 1)
        self.rinv = pow(RADIX, -1, p)              # internal value -> the element it stands for

    # ---- the tracker's rules, exactly ----
    def top_bound(self, vb: float) -> int:
        """floor(vb * p / 2^232) + 1 for the double vb, in exact arithmetic"""
        return int(Fraction(vb) * self.p // (1 << 232)) + 1

    # ---- Montgomery products ----
    @staticmethod
    def mont_admissible(*pairs) -> bool:
        s = sum(max(int(x) for x in a) * max(int(x) for x in b) for a, b in pairs)
        return 9 * s + 9 * (1 << 58) + (1 << 40) < (1 << 64)

    def mont(self, *pairs):
        """(sum of a*b over the pairs) * 2^-261, as fe_mul / fe_mul2 / fe_sqr and the lockstep forms give it"""
        assert self.mont_admissible(*pairs), "a 64-bit column of the product may overflow: inadmissible operands"
        s = sum(value(a) * value(b) for a, b in pairs)
        m = (-s * self.pinv) % RADIX
        t = (s + m * self.p) >> 261
        return digits(t)

    def sqr(self, a):
        assert 2 * max(int(x) for x in a) < U32, "fe_sqr: a doubled limb overflows"
        return self.mont((a, a))

    # ---- linear operations ----
    def sub_const(self, k: int, bits: int):
        """k * p with limb i raised by 2^bits borrowed from limb i + 1 (make_sub_const restated)"""
        c = digits(k * self.p)
        b = 1 << (bits - 29)
        s = [c[0] + (1 << bits)] + [c[i] + (1 << bits) - b for i in range(1, 8)] + [c[8] - b]
        assert value(s) == k * self.p and all(0 <= x < U32 for x in s)
        return s

    def sub(self, k: int, bits: int, a, b):
        s = self.sub_const(k, bits)
        r = [int(a[i]) + s[i] - int(b[i]) for i in range(9)]
        assert all(0 <= x < U32 for x in r), "fe_sub: a limb wraps: inadmissible operands"
        return r

    @staticmethod
    def add(a, b):
        r = [int(x) + int(y) for x, y in zip(a, b)]
        assert all(x < U32 for x in r), "fe_add: a limb wraps: inadmissible operands"
        return r

    @staticmethod
    def shl(a, n: int):
        r = [int(x) << n for x in a]
        assert all(x < U32 for x in r), "fe_dbl / fe_mul4: a limb wraps: inadmissible operands"
        return r

    @staticmethod
    def norm(a):
        r, c = [], 0
        for i in range(8):
            t = int(a[i]) + c
            assert t < U32, "fe_norm: a carry add wraps: inadmissible operand"
            r.append(t & MASK29)
            c = t >> 29
        assert int(a[8]) + c < U32
        return r + [int(a[8]) + c]

    # ---- canonical forms ----
    def small(self, a) -> bool:
        """the precondition of fe_is_zero_mod / fe_canonical"""
        return is_normalised(a) and value(a) < 3 * self.p

    def is_zero_mod(self, a) -> bool:
        assert self.small(a)
        return value(a) % self.p == 0

    def canonical(self, a):
        assert self.small(a)
        return digits(value(a) % self.p)

    def reduce_small_ok(self, a, r) -> str:
        """fe_reduce_small by its contract (whatever the quotient estimate): '' or what is wrong with the result r"""
        assert is_normalised(a) and int(a[8]) <= MASK29
        if not is_normalised(r):
            return "limbs not normalised"
        if value(r) >= 3 * self.p:
            return "value >= 3p"
        if (value(r) - value(a)) % self.p:
            return "residue changed"
        return ""

    def reduce_small(self, a):
        """fe_reduce_small to the limb: the quotient estimate q = (top * QK) >> 53, then a - q p by signed carries"""
        q = (int(a[8]) * self.qk) >> 53
        r, carry = [], 0
        for i in range(8):
            t = int(a[i]) - q * self.mod[i] + carry
            r.append(t & MASK29)
            carry = t >> 29
        return r + [(int(a[8]) - q * self.mod[8] + carry) % U32]

    # ---- packing ----
    @staticmethod
    def unpack(words):
        return digits(sum(int(w) << (32 * i) for i, w in enumerate(words)))

    @staticmethod
    def pack(a):
        v = value(a)
        assert is_normalised(a) and v < (1 << 256), "fe_pack needs a normalised value < 2^256"
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]

    def from_ext(self, words):
        return self.mont((self.unpack(words), self.ext2int))

    def to_ext(self, a):
        return self.pack(self.canonical(self.mont((a, self.int2ext))))

    def elem(self, limbs) -> int:
        """the field element the limbs stand for"""
        return value(limbs) * self.rinv % self.p

    def internal(self, x: int) -> int:
        """the canonical internal value of the field element x"""
        return x * RADIX % self.p


FQ = Field("fq", 0, o.P)
FR = Field("fr", 1, o.R)
FIELDS = (FQ, FR)

# class bounds of g1.h, in multiples of p
JAC_CLASS = (12, 5, 2)
XYZZ_CLASS = (8, 3, 2, 2)
AFF_CLASS = (2, 2)


def in_class(coords, cls) -> str:
    """'' or what puts the coordinates outside their class (normalised limbs, value < bound * p)"""
    for i, (c, b) in enumerate(zip(coords, cls)):
        if not is_normalised(c):
            return f"coordinate {i} is not normalised"
        if value(c) >= b * FQ.p:
            return f"coordinate {i} is >= {b} p"
    return ""


def jac_to_affine(x, y, z):
    """the affine point of Jacobian limbs (X / Z^2, Y / Z^3); Z = 0 mod p is an error, the identity is a flag"""
    zz = FQ.elem(z)
    assert zz != 0, "Z = 0 in a point that is not flagged as the identity"
    zi = pow(zz, -1, FQ.p)
    return (FQ.elem(x) * zi * zi % FQ.p, FQ.elem(y) * zi * zi * zi % FQ.p)


def xyzz_to_affine(x, y, zz, zzz):
    a, b = FQ.elem(zz), FQ.elem(zzz)
    assert a != 0 and b != 0, "ZZ or ZZZ = 0 in a point that is not flagged as the identity"
    assert (a * a * a - b * b) % FQ.p == 0, "ZZ^3 != ZZZ^2"
    return (FQ.elem(x) * pow(a, -1, FQ.p) % FQ.p, FQ.elem(y) * pow(b, -1, FQ.p) % FQ.p)


# ---- the exceptional branches: which multiple of p the squares come out as ------------------------------------------------
def signed_s2(s2p, neg):
    return FQ.sub(3, 29, [0] * 9, s2p) if neg else s2p


def madd_nz_squares(px, py, pz, qx, qy, neg):
    """g1_madd_nz's hh = h^2 and rr0 = r0^2 as multiples of p (None: not a multiple)"""
    z1z1 = FQ.sqr(pz)
    u2 = FQ.mont((qx, z1z1))
    s2 = signed_s2(FQ.mont((qy, FQ.mont((pz, z1z1)))), neg)
    hh = value(FQ.sqr(FQ.norm(FQ.sub(13, 29, u2, px))))
    rr0 = value(FQ.sqr(FQ.norm(FQ.sub(6, 29, s2, py))))
    return tuple(v // FQ.p if v % FQ.p == 0 else None for v in (hh, rr0))


def add_nz_squares(px, py, pz, qx, qy, qz):
    z1z1, z2z2 = FQ.sqr(pz), FQ.sqr(qz)
    u1, u2 = FQ.mont((px, z2z2)), FQ.mont((qx, z1z1))
    s1, s2 = FQ.mont((py, FQ.mont((qz, z2z2)))), FQ.mont((qy, FQ.mont((pz, z1z1))))
    hh = value(FQ.sqr(FQ.norm(FQ.sub(3, 29, u2, u1))))
    rr0 = value(FQ.sqr(FQ.norm(FQ.sub(3, 29, s2, s1))))
    return tuple(v // FQ.p if v % FQ.p == 0 else None for v in (hh, rr0))


def xmadd_fast_square(ax, azz, qx):
    """g1x_madd_fast's PP = (U2 - X1)^2 as a multiple of p (None: not a multiple)"""
    v = value(FQ.sqr(FQ.norm(FQ.sub(9, 29, FQ.mont((qx, azz)), ax))))
    return v // FQ.p if v % FQ.p == 0 else None


# ---- what the C sources state ------------------------------------------------------------------------------------------------
def parse_ops(header_text: str):
    """{'UF_MUL': 0, ..., 'UC_ADD': 10} from csrc/unit_ops.h"""
    return {name: int(num) for name, num in re.findall(r"^\s*(U[FC]_[A-Z0-9_]+) = (\d+),", header_text, re.M)}


def parse_constants(inc_text: str):
    """{'FqParams': {'MOD': [...], 'INV29': n, ...}, 'FrParams': ...} from csrc/bn256_constants.inc"""
    out = {}
    for name, body in re.findall(r"struct (\w+) \{(.*?)\n\};", inc_text, re.S):
        d = {}
        for key, arr in re.findall(r"uint32_t (\w+)\[\d+\] = \{([^}]*)\}", body):
            d[key] = [int(x.strip().rstrip("u"), 16) for x in arr.split(",")]
        for key, num in re.findall(r"uint32_t (\w+) = (\w+)u;", body):
            d[key] = int(num, 0)
        out[name] = d
    return out
