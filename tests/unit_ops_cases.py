"""The case tables of the unit-op tests and their comparison with the model (ff29_model.py), shared by test_unit_ops_host.py (the CPU
runner, plain and -DHM_BOUNDS) and test_unit_ops_gpu.py (libhm_devcheck.so).  Records are the u32 words csrc/unit_ops.h describes.

Every operand is generated inside a class (vb, lb, tb) -- value < vb * p, limbs 0..7 <= lb, top limb <= tb -- that is written into
the record beside it, and every case satisfies its op's precondition for the DECLARED class, so the -DHM_BOUNDS build must accept
it; nothing is filtered after generation, and check_* counts what it compared so that the tests can assert that it was everything."""
import functools
import os
import random
import struct
from fractions import Fraction

import numpy as np

import ff29_model as m
from ff29_model import FQ, MASK29, RADIX, digits, value
from oracle import bn256_ref as o

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "halo2-experiments_amd", "csrc")
with open(os.path.join(CSRC, "unit_ops.h")) as _f:
    OPS = m.parse_ops(_f.read())
FIELD_IN, FIELD_OUT, CURVE_IN, CURVE_OUT = 80, 48, 80, 40
SUBS = sorted((int(n.split("_")[2]), int(n.split("_")[3])) for n in OPS if n.startswith("UF_SUB_"))
RANDOMS = 2048            # random cases per OP (and field), dealt round-robin over the op's admissible class tuples: a product has
#                           dozens to hundreds of those, so one class tuple sees 2048 / (number of tuples) randoms; every class's
#                           edge operands are all there whatever this number is
COLUMN_LIMIT = ((1 << 64) - 1 - 9 * (1 << 58) - (1 << 40)) // 9      # the largest admissible Amax*Bmax (+ Cmax*Dmax)
SQR_LB = int(COLUMN_LIMIT ** 0.5) - 1                                 # the largest limb a square admits (floor(sqrt) to double precision)
assert SQR_LB * SQR_LB <= COLUMN_LIMIT < (SQR_LB + 3) ** 2


# ---- operands in classes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_limit(field, vb):
    """the least integer >= vb * p for the double vb: a value is inside the class when it is below this"""
    return -((-Fraction(vb) * field.p) // 1)


@functools.lru_cache(maxsize=None)
def top_bound(field, vb):
    return field.top_bound(vb)


class El:
    """limbs with the class they are declared at; exact: tb is what the value bound implies (the C side then checks its own rule)"""
    __slots__ = ("l", "vb", "lb", "tb", "exact")

    def __init__(self, field, limbs, vb, lb, tb=None, check_value=True):
        self.l, self.vb, self.lb = [int(x) for x in limbs], float(vb), int(lb)
        self.exact = tb is None and lb == MASK29
        self.tb = top_bound(field, self.vb) if tb is None else int(tb)
        assert all(0 <= x <= self.lb for x in self.l[:8]) and 0 <= self.l[8] <= self.tb, "operand outside its declared limb bounds"
        assert value_limit(field, self.vb) < RADIX and self.lb < (1 << 32) and self.tb < (1 << 32)
        if check_value:
            assert value(self.l) < value_limit(field, self.vb) or value(self.l) == 0, "operand outside its declared value bound"


def lazy(limbs, lb, rng=None):
    """the same integer with limbs 0..7 raised towards lb by 2^29 units borrowed from the limb above (rng: by a random amount)"""
    l = [int(x) for x in limbs]
    for i in range(8):
        k = min(l[i + 1], (lb - l[i]) >> 29)
        if rng is not None:
            k = rng.randint(0, k)
        l[i] += k << 29
        l[i + 1] -= k
    return l


def elem(field, v, vb, lb=MASK29, rng=None):
    assert 0 <= v
    return El(field, lazy(digits(v), lb, rng) if lb > MASK29 else digits(v), vb, lb)


def all_at(field, lb, vb):
    """every limb 0..7 exactly lb, the top limb the largest the value bound admits"""
    low = sum(lb << (29 * i) for i in range(8))
    top = int((Fraction(vb) * field.p - 1 - low) // (1 << 232))
    assert 0 <= top
    return El(field, [lb] * 8 + [top], vb, lb)


def vb_max(field):
    """the largest value bound the tracker accepts, a hair under 2^261 / p"""
    return float(Fraction(RADIX, field.p)) * (1 - 1e-9)


def edge_values(field, vb):
    p = field.p
    top = int(Fraction(vb) * p)
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1, top - 1, top - p, top - p - 1, top // 2]
    out = []
    for v in vals:
        if 0 <= v < Fraction(vb) * p and v not in out:
            out.append(v)
    return out


def edges(field, vb, lb=MASK29):
    """the class's edge operands: the listed values (lazy classes: re-expressed with limbs up to lb), every limb at its maximum"""
    out = [elem(field, v, vb, lb) for v in edge_values(field, vb)]
    if lb == MASK29:
        tb = field.top_bound(vb)
        if tb >= 2:
            out.append(El(field, [MASK29] * 8 + [tb - 2], vb, lb))       # all ones under the largest top limb of the class
        # every limb at MASK29 with the top limb AT tb: that value belongs to the next class up, which is what it is declared at
        vb2 = float(Fraction((tb + 1) << 232, field.p)) * (1 + 1e-12)
        if Fraction(vb2) * field.p < RADIX * (1 - 1e-9):
            out.append(El(field, [MASK29] * 8 + [tb], vb2, lb))
    else:
        out.append(all_at(field, lb, vb))
    return out


def rand_elem(field, rng, vb, lb=MASK29):
    return elem(field, rng.randrange(value_limit(field, vb)), vb, lb, rng if lb > MASK29 else None)


NORMAL_VB = (1.0, 2.0, 3.0, 5.0, 12.0, 16.0, 60.0, 160.0)
LAZY = (((1 << 30) - 1, 6.0), ((3 << 29) - 1, 9.0), ((1 << 31) - 1, 12.0), ((1 << 31) - 1, 160.0))
CLASSES = tuple((vb, MASK29) for vb in NORMAL_VB) + tuple((vb, lb) for lb, vb in LAZY)


def product_fits(field, *pairs):
    """the precondition of a product for the DECLARED classes of its operand pairs, and a result the tracker can hold"""
    col = sum(max(a[1], field.top_bound(a[0])) * max(b[1], field.top_bound(b[0])) for a, b in pairs)
    vbs = sum(Fraction(a[0]) * Fraction(b[0]) for a, b in pairs)
    return col <= COLUMN_LIMIT and (vbs * field.p / RADIX + 1) * field.p < RADIX * (1 - 1e-6)


# ---- records -----------------------------------------------------------------------------------------------------------------
def field_record(ops, words=None):
    r = [0] * FIELD_IN
    exact = 0
    for i, e in enumerate(ops):
        r[9 * i:9 * i + 9] = e.l
        lo, hi = struct.unpack("<II", struct.pack("<d", e.vb))
        r[54 + 4 * i:58 + 4 * i] = [e.lb, e.tb, lo, hi]
        exact |= int(e.exact) << i
    r[78] = exact
    if words is not None:
        r[0:8] = [int(w) for w in words]
    return r


# ---- the field tables --------------------------------------------------------------------------------------------------------
def _mul_cases(field, rng, n_random):
    cases = []
    pairs = [(a, b) for a in CLASSES for b in CLASSES if product_fits(field, (a, b))]
    assert ((160.0, (1 << 31) - 1), (2.0, MASK29)) in pairs
    # the edge operands of one class against those of another, for the class pairs the callers use and the widest ones
    for a, b in (((3.0, MASK29), (3.0, MASK29)), ((12.0, MASK29), (2.0, MASK29)), ((12.0, (1 << 31) - 1), (3.0, MASK29)),
                 ((6.0, (1 << 30) - 1), (6.0, (1 << 30) - 1)), ((160.0, (1 << 31) - 1), (160.0, MASK29)), ((160.0, MASK29), (1.0, MASK29))):
        assert (a, b) in pairs
        cases += [(x, y) for x in edges(field, *a) for y in edges(field, *b)]
    # the maximum admissible column sum: every limb of A at 2^31 - 1 and of B at the largest limb that still fits, and the square root of it
    for la in ((1 << 31) - 1, (1 << 30) + 12345, SQR_LB):
        lb = COLUMN_LIMIT // la
        cases.append((all_at(field, la, 168.0), all_at(field, lb, 168.0)))
        cases.append((all_at(field, lb, 168.0), all_at(field, la, 12.0)))
    # M = 0 (A * B = 2^261 and = 0) and M = 2^261 - 1 (A = 1, B = p)
    cases.append((elem(field, 1 << 131, 2.0), elem(field, 1 << 130, 2.0)))
    cases.append((elem(field, 0, 2.0), elem(field, field.p - 1, 2.0)))
    cases.append((elem(field, 1, 2.0), elem(field, field.p, 2.0)))
    cases.append((elem(field, field.p, 2.0), elem(field, 1, 2.0)))
    for i in range(n_random):
        a, b = pairs[i % len(pairs)]
        cases.append((rand_elem(field, rng, *a), rand_elem(field, rng, *b)))
    return cases


def _sqr_cases(field, rng, n_random):
    classes = [c for c in CLASSES if product_fits(field, (c, c)) and 2 * c[1] < (1 << 32)]
    assert (6.0, (1 << 30) - 1) in classes
    cases = [x for c in classes for x in edges(field, *c)]
    cases += [all_at(field, SQR_LB, 160.0), all_at(field, SQR_LB, 12.0), elem(field, 1 << 131, 2.0)]
    cases += [rand_elem(field, rng, *classes[i % len(classes)]) for i in range(n_random)]
    return [(x,) for x in cases]


def _mul2_cases(field, rng, n_random):
    quads = [(a, b, c, d) for a in CLASSES for b in CLASSES[:5] for c in CLASSES for d in CLASSES[:5] if product_fits(field, (a, b), (c, d))]
    # g1_madd_nz's Y3 = r (V - X3) - 2 Y1 J: limbs < 2^30 by normalised plus limbs < 2^31 by normalised
    madd = ((6.0, (1 << 30) - 1), (12.0, MASK29), (12.0, (1 << 31) - 1), (2.0, MASK29))
    assert madd in quads
    cases = []
    for q in (madd, ((3.0, MASK29),) * 4, ((12.0, MASK29), (12.0, MASK29), (12.0, (1 << 31) - 1), (1.0, MASK29))):
        assert q in quads
        es = [edges(field, *c) for c in q]
        n = max(len(e) for e in es)
        for s in range(n):                                  # every edge of every operand, against rotating edges of the others
            for t in range(3):
                cases.append(tuple(es[j][(s + t * j) % len(es[j])] for j in range(4)))
    # the maximum admissible column sum, split between the two products
    la = (1 << 31) - 1
    for lb in (MASK29, COLUMN_LIMIT // (2 * la)):
        rest = COLUMN_LIMIT - la * lb
        lc = MASK29
        ld = rest // lc
        cases.append((all_at(field, la, 100.0), all_at(field, lb, 100.0), all_at(field, lc, 100.0), all_at(field, min(ld, (1 << 32) - 1), 100.0)))
    cases.append((elem(field, 1 << 131, 2.0), elem(field, 1 << 129, 2.0), elem(field, 1 << 130, 2.0), elem(field, 1 << 130, 2.0)))   # M = 0
    cases.append((elem(field, 1, 2.0), elem(field, field.p - 1, 2.0), elem(field, 1, 2.0), elem(field, 1, 2.0)))                       # M = 2^261 - 1
    for i in range(n_random):
        q = quads[(i * 7919) % len(quads)]
        cases.append(tuple(rand_elem(field, rng, *c) for c in q))
    return cases


def _linear_cases(field, rng, n_random):
    """{op: cases} for add, dbl, mul4, norm"""
    out = {}
    lim = vb_max(field)
    add_pairs = [(a, b) for a in CLASSES for b in CLASSES if a[1] + b[1] < (1 << 32) and a[0] + b[0] < lim]
    cases = []
    for a, b in (((3.0, MASK29), (3.0, MASK29)), ((2.0, MASK29), (6.0, (1 << 30) - 1)), ((12.0, (1 << 31) - 1), (12.0, (1 << 31) - 1)),
                 ((160.0, (1 << 31) - 1), (6.0, (1 << 30) - 1))):
        assert (a, b) in add_pairs
        cases += [(x, y) for x in edges(field, *a) for y in edges(field, *b)]
    cases += [(rand_elem(field, rng, *add_pairs[i % len(add_pairs)][0]), rand_elem(field, rng, *add_pairs[i % len(add_pairs)][1]))
              for i in range(n_random)]
    out["UF_ADD"] = cases
    for name, shift in (("UF_DBL", 1), ("UF_MUL4", 2)):
        classes = [c for c in CLASSES if (c[1] << shift) < (1 << 32) and c[0] * (1 << shift) < lim]
        classes.append((lim / (1 << shift) * (1 - 1e-9), (1 << (32 - shift)) - 1))        # the widest class the op admits
        cases = [(x,) for c in classes for x in edges(field, *c)]
        cases += [(rand_elem(field, rng, *classes[i % len(classes)]),) for i in range(n_random)]
        out[name] = cases
    classes = list(CLASSES) + [(lim, (1 << 32) - 17), (12.0, (1 << 32) - 17)]              # fe_norm: lb + 16 < 2^32
    cases = [(x,) for c in classes for x in edges(field, *c)]
    cases += [(rand_elem(field, rng, *classes[i % len(classes)]),) for i in range(n_random)]
    out["UF_NORM"] = cases
    return out


def _sub_cases(field, rng, k, bits, n_random):
    s = field.sub_const(k, bits)
    smax, lim = max(s[:8]), vb_max(field)
    lbmax = (1 << bits) - (1 << (bits - 29))
    # subtrahends: the normalised class below (k - 1) p that the header names, and the widest the constant admits: limbs up to
    # 2^bits - 2^(bits - 29) under a top limb up to the constant's
    assert field.top_bound(float(k - 1)) <= s[8]
    bs = edges(field, float(k - 1))
    wide = (float(k), lbmax, s[8])
    bs.append(El(field, [lbmax] * 8 + [s[8]], *wide))
    for v in edge_values(field, float(k - 1)):
        bs.append(El(field, lazy(digits(v), lbmax), *wide))
    # minuends: zero as fe_zero declares it, normalised classes, the laziest limbs the result admits
    a_lb = min((1 << 31) - 1, (1 << 32) - 1 - smax)
    a_classes = [(c, MASK29) for c in (2.0, 3.0, 12.0, lim - k - 1e-6)] + [(12.0, a_lb)]
    as_ = [El(field, [0] * 9, 0.0, 0, 0)] + [x for c in a_classes for x in edges(field, *c)]
    cases = [(x, y) for x in as_ for y in bs]
    for i in range(n_random):
        a = rand_elem(field, rng, *a_classes[i % len(a_classes)])
        if i % 2:
            b = rand_elem(field, rng, float(k - 1))
        else:
            b = El(field, lazy(digits(rng.randrange((k - 1) * field.p)), lbmax, rng), *wide)
        cases.append((a, b))
    return cases


def _small_cases(field, rng, n_random):
    """{op: cases} for is_zero_mod and canonical: normalised values < 3p"""
    p, mod = field.p, field.mod
    vals = list(edge_values(field, 3.0))
    for kp in (0, p, 2 * p):
        d = digits(kp)
        for i in range(9):                       # one limb changed: for i >= 1 the low limb still passes is_zero_mod's filter
            for delta in (-1, 1, 12345):
                l = list(d)
                l[i] += delta
                if 0 <= l[i] <= (MASK29 if i < 8 else 1 << 28) and value(l) < 3 * p:
                    vals.append(value(l))
            for low in (0, MASK29):              # agrees with k p from limb i upwards (borrow chains of every length)
                l = [low] * i + d[i:]
                if value(l) < 3 * p:
                    vals.append(value(l))
            l = d[:i] + [0] * (9 - i)            # agrees with k p below limb i
            vals.append(value(l))
    for l0 in (0, mod[0], (2 * mod[0]) & MASK29):           # the filter's three low limbs over random upper limbs
        for _ in range(16):
            v = rng.randrange(3 * p)
            vals.append((v >> 29 << 29) | l0)
    vals = [v for v in vals if v < 3 * p]
    third = n_random // 3
    vals += [rng.randrange(k * p, (k + 1) * p) for k in range(3) for _ in range(third)]
    cases = [(elem(field, v, 3.0),) for v in vals]
    cases += [(El(field, [MASK29] * 8 + [field.top_bound(3.0) - 2], 3.0, MASK29),)]
    return {"UF_IS_ZERO_MOD": cases, "UF_CANONICAL": cases}


def _reduce_small_cases(field, rng, n_random):
    """any normalised value < 2^261.  The class is the widest the tracker can hold (tb = 2^29 - 1); 2^261 - 1 itself sits a hair above
    what a double value bound can state, so for this op alone the value bound is nominal (fe_reduce_small does not read it)."""
    p, step = field.p, field.topmod + 1
    vb = vb_max(field)
    vals = [RADIX - 1]
    k = 0
    while k * p < RADIX:
        vals += [v for v in (k * p - 1, k * p, k * p + 1) if 0 <= v < RADIX]
        k += 1
    mult = 1
    while mult * step - 1 <= MASK29:             # top limbs on both sides of every multiple of MOD[8] + 1
        for top in (mult * step - 1, mult * step, mult * step + 1):
            if top <= MASK29:
                for low in (0, (1 << 232) - 1, rng.getrandbits(232)):
                    vals.append((top << 232) | low)
        mult += 1
    vals += [rng.getrandbits(261) for _ in range(n_random)]
    return [(El(field, digits(v), vb, MASK29, MASK29, check_value=False),) for v in vals]


def _pack_cases(field, rng, n_random):
    """{op: (cases, words)}: unpack / from_ext read 8 words; pack / to_ext read an element"""
    p = field.p
    raw = [0, 1, p - 1, p, p + 1, 2 * p, (1 << 256) - 1, (1 << 255), (1 << 256) - p] + [((1 << 29 * i) - 1) for i in range(1, 9)]
    raw += [rng.getrandbits(256) for _ in range(n_random)]
    words = [[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for v in raw]
    canon = [0, 1, p - 1, p // 2, RADIX % p] + [rng.randrange(p) for _ in range(n_random)]
    # fe_pack admits a top limb below 2^24: the class whose value bound implies exactly that, and the canonical class
    vb24 = float(Fraction((((1 << 24) - 2) << 232) + (1 << 231), p))
    assert field.top_bound(vb24) == (1 << 24) - 1
    wide = [(((1 << 24) - 2) << 232) - 1, ((1 << 24) - 2) << 232, 1 << 255, int(Fraction(vb24) * p) - 1] + [rng.randrange(int(Fraction(vb24) * p)) for _ in range(n_random // 2)]
    packs = [(elem(field, v, 1.0),) for v in canon] + [(elem(field, v, vb24),) for v in wide]
    ext = [x for vb in (1.0, 2.0, 3.0, 12.0, 160.0) for x in edges(field, vb)]
    ext += [rand_elem(field, rng, vb) for vb in (2.0, 3.0, 16.0) for _ in range(n_random // 3)]
    return {"UF_UNPACK": words, "UF_FROM_EXT": words, "UF_PACK": packs, "UF_TO_EXT": [(x,) for x in ext]}


@functools.lru_cache(maxsize=None)
def field_tables(field, n_random=RANDOMS):
    """{op name: (n, FIELD_IN) uint32 records}; made once and shared: do not write to them"""
    rng = random.Random(1000 + field.index)
    t = {}
    mul, sqr, mul2 = _mul_cases(field, rng, n_random), _sqr_cases(field, rng, n_random), _mul2_cases(field, rng, n_random)
    t["UF_MUL"], t["UF_SQR"], t["UF_MUL2"] = mul, sqr, mul2
    # the lockstep forms: the same operands, products paired with a shifted copy of the list so that unlike classes meet
    n = len(mul)
    t["UF_MUL_X2"] = [mul[i] + mul[(i * 3 + 1) % n] for i in range(n)]
    t["UF_MUL_X3"] = [mul[i] + mul[(i * 5 + 2) % n] + mul[(n - 1 - i)] for i in range(n)]
    t["UF_SQR_X2"] = [sqr[i] + sqr[(i * 3 + 1) % len(sqr)] for i in range(len(sqr))]
    t["UF_MUL_MUL2"] = [mul[(i * 11 + 3) % n] + mul2[i] for i in range(len(mul2))]
    t.update(_linear_cases(field, rng, n_random))
    for k, bits in SUBS:
        t[f"UF_SUB_{k}_{bits}"] = _sub_cases(field, rng, k, bits, n_random)
    t.update(_small_cases(field, rng, n_random))
    t["UF_REDUCE_SMALL"] = _reduce_small_cases(field, rng, n_random)
    packs = _pack_cases(field, rng, n_random)
    out = {}
    for name, cases in t.items():
        out[name] = np.array([field_record(c) for c in cases], dtype=np.uint32)
    for name in ("UF_UNPACK", "UF_FROM_EXT"):
        out[name] = np.array([field_record((), w) for w in packs[name]], dtype=np.uint32)
    for name in ("UF_PACK", "UF_TO_EXT"):
        out[name] = np.array([field_record(c) for c in packs[name]], dtype=np.uint32)
    assert set(out) == {n for n in OPS if n.startswith("UF_") and n != "UF_OP_END"}, "an op of the field table has no cases"
    return out


def check_field(field, name, ins, outs):
    """compare every result record with the model; returns how many cases were compared"""
    assert ins.shape[0] == outs.shape[0] and outs.shape[1] == FIELD_OUT
    compared = 0
    for idx in range(ins.shape[0]):
        rec, out = ins[idx].tolist(), outs[idx].tolist()
        a = [rec[9 * i:9 * i + 9] for i in range(6)]
        got = [out[0:9], out[9:18], out[18:27]]
        where = f"{field.name} {name} case {idx}: operands {[[hex(x) for x in v] for v in a if any(v)]}"
        if name == "UF_MUL":
            exp = [field.mont((a[0], a[1]))]
        elif name == "UF_SQR":
            exp = [field.sqr(a[0])]
        elif name == "UF_MUL2":
            exp = [field.mont((a[0], a[1]), (a[2], a[3]))]
        elif name == "UF_MUL_X2":
            exp = [field.mont((a[0], a[1])), field.mont((a[2], a[3]))]
        elif name == "UF_MUL_X3":
            exp = [field.mont((a[0], a[1])), field.mont((a[2], a[3])), field.mont((a[4], a[5]))]
        elif name == "UF_SQR_X2":
            exp = [field.sqr(a[0]), field.sqr(a[1])]
        elif name == "UF_MUL_MUL2":
            exp = [field.mont((a[0], a[1])), field.mont((a[2], a[3]), (a[4], a[5]))]
        elif name == "UF_ADD":
            exp = [field.add(a[0], a[1])]
        elif name == "UF_DBL":
            exp = [field.shl(a[0], 1)]
        elif name == "UF_MUL4":
            exp = [field.shl(a[0], 2)]
        elif name == "UF_NORM":
            exp = [field.norm(a[0])]
        elif name.startswith("UF_SUB_"):
            k, bits = (int(x) for x in name.split("_")[2:])
            exp = [field.sub(k, bits, a[0], a[1])]
        elif name == "UF_IS_ZERO_MOD":
            assert out[27] == int(field.is_zero_mod(a[0])), where + f": got {out[27]}"
            exp = []
        elif name == "UF_CANONICAL":
            exp = [field.canonical(a[0])]
        elif name == "UF_REDUCE_SMALL":
            bad = field.reduce_small_ok(a[0], got[0])
            assert not bad, where + f": {bad}: got {[hex(x) for x in got[0]]}"
            exp = [field.reduce_small(a[0])]         # and the same limbs on the host and on the device
        elif name == "UF_UNPACK":
            exp = [field.unpack(rec[0:8])]
        elif name == "UF_FROM_EXT":
            exp = [field.from_ext(rec[0:8])]
        elif name == "UF_PACK":
            exp = [field.pack(a[0]) + [0]]
        elif name == "UF_TO_EXT":
            exp = [field.to_ext(a[0]) + [0]]
        else:
            raise AssertionError(f"no model for {name}")
        for j, e in enumerate(exp):
            assert got[j] == e, where + f": result {j}: got {[hex(x) for x in got[j]]}, expected {[hex(x) for x in e]}"
            if out[44] and name not in ("UF_PACK", "UF_TO_EXT"):
                # the -DHM_BOUNDS build: what the tracker derived for this result must hold for the result's exact value.  (<=, not <:
                # the tracker's own zero is "value < 0 * p", and top_bound_from_value is sound for value = vb * p.)
                lb, tb, lo, hi = out[32 + 4 * j:36 + 4 * j]
                vb = struct.unpack("<d", struct.pack("<II", lo, hi))[0]
                assert all(x <= lb for x in e[:8]) and e[8] <= tb, where + f": result {j} exceeds its tracked limb bounds ({lb}, {tb})"
                assert value(e) <= Fraction(vb) * field.p, where + f": result {j} exceeds its tracked value bound {vb} p"
        compared += 1
    return compared


# ---- the curve table ----------------------------------------------------------------------------------------------------------
X_LIFTS, Y_LIFTS, Z_LIFTS = (0, 5, 11), (0, 2, 4), (0, 1)
XX_LIFTS, XY_LIFTS = (0, 3, 7), (0, 1, 2)
JAC_LIFTS = [(a, b, c) for a in X_LIFTS for b in Y_LIFTS for c in Z_LIFTS]
XYZZ_LIFTS = [(a, b, c, d) for a in XX_LIFTS for b in XY_LIFTS for c in (0, 1) for d in (0, 1)]
AFF_LIFTS = [(a, b) for a in (0, 1) for b in (0, 1)]


def lifted(x, j):
    return digits(FQ.internal(x) + j * FQ.p)


def jac_rep(pt, z, lifts):
    """Jacobian limbs of the affine point under Z = z, each coordinate lifted by its multiple of p; None: the flagged identity"""
    if pt is None:
        return [0] * 27, 1
    x, y = pt
    return lifted(x * z * z % FQ.p, lifts[0]) + lifted(y * z * z * z % FQ.p, lifts[1]) + lifted(z, lifts[2]), 0


def xyzz_rep(pt, z, lifts):
    if pt is None:
        return [0] * 36, 1
    x, y = pt
    zz, zzz = z * z % FQ.p, z * z * z % FQ.p
    return lifted(x * zz % FQ.p, lifts[0]) + lifted(y * zzz % FQ.p, lifts[1]) + lifted(zz, lifts[2]) + lifted(zzz, lifts[3]), 0


def aff_rep(pt, lifts):
    return lifted(pt[0], lifts[0]) + lifted(pt[1], lifts[1])


def curve_record(first, first_form, second=None, second_form=None, neg=0):
    r = [0] * CURVE_IN
    limbs, inf = first if first is not None else ([0] * 27, 0)
    r[0:len(limbs)] = limbs
    r[36] = inf
    r[70:74] = list(m.XYZZ_CLASS if first_form == "xyzz" else m.JAC_CLASS + (0,))
    if second is not None:
        if second_form == "aff":
            r[40:58] = second
            r[74:77] = list(m.AFF_CLASS) + [0]
        else:
            r[40:67] = second[0]
            r[67] = second[1]
            r[74:77] = list(m.JAC_CLASS)
    r[68] = neg
    return r


def curve_points():
    g = o.G1_GEN
    rng = random.Random(77)
    ks = [1, 2, 3, o.R - 1, o.R - 2, (o.R + 1) // 2] + [rng.randrange(1, o.R) for _ in range(6)]
    return [o.g1_mul(k, g) for k in ks]


@functools.lru_cache(maxsize=None)
def curve_tables():
    """{op name: ((n, CURVE_IN) uint32 records, [per case: dict(exp=affine result or None, kind=...)])}"""
    rng = random.Random(4242)
    pts = curve_points()

    def z():
        return rng.randrange(1, FQ.p)

    def signed(q, neg):
        return o.g1_neg(q) if neg else q

    t = {n: ([], []) for n in OPS if n.startswith("UC_") and n != "UC_OP_END"}

    def put(name, rec, **meta):
        t[name][0].append(rec)
        t[name][1].append(meta)

    # --- one-operand ops: every point under every lift
    for pt in pts:
        for la in AFF_LIFTS:
            put("UC_NEG_AFFINE", curve_record(None, "jac", aff_rep(pt, la), "aff"), exp=o.g1_neg(pt))
        for lj in JAC_LIFTS:
            rep = jac_rep(pt, z(), lj)
            put("UC_DOUBLE_NZ", curve_record(rep, "jac"), exp=o.g1_add(pt, pt))
            put("UC_X_FROM_JAC", curve_record(rep, "jac"), exp=pt)
        for lx in XYZZ_LIFTS:
            put("UC_X_TO_JAC", curve_record(xyzz_rep(pt, z(), lx), "xyzz"), exp=pt)
    put("UC_X_FROM_JAC", curve_record(jac_rep(None, 1, None), "jac"), exp=None)
    put("UC_X_TO_JAC", curve_record(xyzz_rep(None, 1, None), "xyzz"), exp=None)

    # --- mixed additions: generic pairs, P + P and P + (-P) under both signs, every lift of the accumulator and of the operand
    def mixed(p1, q):
        kind = "equal" if p1[0] == q[0] else "generic"
        for neg in (0, 1):
            exp = o.g1_add(p1, signed(q, neg))
            for la in AFF_LIFTS:
                qa = aff_rep(q, la)
                for lj in JAC_LIFTS:
                    rec = curve_record(jac_rep(p1, z(), lj), "jac", qa, "aff", neg)
                    put("UC_MADD_NZ", rec, exp=exp, kind=kind)
                    put("UC_MADD", rec, exp=exp, kind=kind)
                for lx in XYZZ_LIFTS:
                    rec = curve_record(xyzz_rep(p1, z(), lx), "xyzz", qa, "aff", neg)
                    for name in ("UC_XMADD_FAST", "UC_XMADD_FAST_LOCKSTEP", "UC_XMADD"):
                        put(name, rec, exp=exp, kind=kind, same_x=kind != "generic")

    n = len(pts)
    for i in range(n):
        if i % 2 == 0:
            mixed(pts[i], pts[(i + 1) % n])
        mixed(pts[i], pts[i])                               # neg = 0 doubles, neg = 1 cancels
        mixed(pts[i], o.g1_neg(pts[i]))                     # and the other way round

    # --- the top-limb edge of P = U2 - X1 + K p: X1 in the last 2^232-block of its class (its top limb is that of 12p, for XYZZ of
    # 8p: the largest a stored X can have) against a U2 whose top limb is 0, the one operand pair that needs all of the constant's
    # top limb.  Constructed, not searched for: q.x is a SMALL internal integer (so that q.x * ZZ stays below c' * 2^261 and the
    # product comes out as c' itself), c' < 2^232 is the U2 wanted, ZZ = Z^2 must then stand for c' * 2^261 / q.x, which fixes Z
    # when that is a square; X1 = c + (K - 1) p for the largest c < p whose x1 = c / Z^2 is on the curve.
    def sqrt_fq(a):
        r = pow(a % FQ.p, (FQ.p + 1) // 4, FQ.p)
        return r if (r * r - a) % FQ.p == 0 else None

    def on_curve(x):
        y = sqrt_fq(x * x * x + o.B_COEFF)
        return None if y is None else (x, y)

    def top_limb_operands(k):
        """P1, z, Q, c', c for the class X < k p"""
        q, qx = None, rng.randrange(2, 1 << 20)
        while q is None:
            qx += 1
            q = on_curve(qx * FQ.rinv % FQ.p)                # the point whose internal x is the integer qx
        zv = None
        while zv is None:
            c2 = rng.randrange(1 << 231, 1 << 232)
            zsq = c2 * RADIX * pow(qx, -1, FQ.p) * FQ.rinv % FQ.p
            zv = sqrt_fq(zsq)
        lo = (digits(k * FQ.p)[8] << 232) - (k - 1) * FQ.p
        p1, c = None, FQ.p
        while p1 is None:
            c -= 1
            assert c >= lo, "no curve point in the top block of the class"
            p1 = on_curve(FQ.elem(digits(c)) * pow(zsq, -1, FQ.p) % FQ.p)
        assert lifted(q[0], 0) == digits(qx)
        return p1, zv, q, c2

    # The same for the Y subtractions, r0 = +-S2 - Y1 + 6p (XYZZ: R = +-S2 - Y1 + 4p) and -Y1 = 0 - Y1 + K p: Y1 in the last block of
    # its class against an S2 = q.y * Z^3 whose top limb is 0, so Z^3 must stand for c' * 2^261 / q.y with q.y a small integer: a cube
    # root.  The chord law uses neither curve coefficient, and the formulas are identities of it, so these operands need not lie
    # on the curve: x1 and q.x are random, y1 = c / Z^3.
    t9 = (FQ.p - 1) // 9
    assert (FQ.p - 1) % 27 and t9 % 3
    zeta = next(pow(h, t9, FQ.p) for h in range(2, 50) if pow(h, (FQ.p - 1) // 3, FQ.p) != 1)      # a primitive 9th root of unity

    def cbrt_fq(a):
        if pow(a, (FQ.p - 1) // 3, FQ.p) != 1:
            return None
        r = pow(a, pow(3, -1, t9), FQ.p)                     # r^3 = a * (a 9th root of unity): settle it among the nine
        return next(r * pow(zeta, j, FQ.p) % FQ.p for j in range(9) if pow(r * pow(zeta, j, FQ.p), 3, FQ.p) == a)

    def top_limb_y_operands(k):
        """(x1, y1), z, (q.x, q.y), c' for the class Y < k p"""
        qy = rng.randrange(2, 1 << 20)
        zv = None
        while zv is None:
            c2 = rng.randrange(1 << 231, 1 << 232)
            zcube = c2 * RADIX * pow(qy, -1, FQ.p) * FQ.rinv % FQ.p
            zv = cbrt_fq(zcube)
        lo = (digits(k * FQ.p)[8] << 232) - (k - 1) * FQ.p
        c = rng.randrange(lo, FQ.p)
        p1 = (rng.randrange(1, FQ.p), FQ.elem(digits(c)) * pow(zcube, -1, FQ.p) % FQ.p)
        q = (rng.randrange(1, FQ.p), qy * FQ.rinv % FQ.p)
        return p1, zv, q, c2

    for lx in X_LIFTS:
        for lz in Z_LIFTS:
            p1, zv, q, c2 = top_limb_y_operands(5)
            rep = jac_rep(p1, zv, (lx, 4, lz))
            zl = rep[0][18:27]
            assert rep[0][17] == digits(5 * FQ.p)[8] and FQ.mont((lifted(q[1], 0), FQ.mont((zl, FQ.sqr(zl))))) == digits(c2)
            for neg in (0, 1):
                rec = curve_record(rep, "jac", aff_rep(q, (lz, 0)), "aff", neg)
                put("UC_MADD_NZ", rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb")
                put("UC_MADD", rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb")
    for lx in XX_LIFTS:
        for lzzz in (0, 1):
            p1, zv, q, c2 = top_limb_y_operands(3)
            rep = xyzz_rep(p1, zv, (lx, 2, 1 - lzzz, lzzz))
            assert rep[0][17] == digits(3 * FQ.p)[8] and FQ.mont((lifted(q[1], 0), rep[0][27:36])) == digits(c2)
            for neg in (0, 1):
                rec = curve_record(rep, "xyzz", aff_rep(q, (lzzz, 0)), "aff", neg)
                for name in ("UC_XMADD_FAST", "UC_XMADD_FAST_LOCKSTEP", "UC_XMADD"):
                    put(name, rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb", same_x=False)
    # and y -> 3p - y of an affine operand whose y has the top limb of 2p (a field negation: the pair need not be a point)
    for lx in (0, 1):
        y = FQ.elem(digits(rng.randrange((digits(2 * FQ.p)[8] << 232) - FQ.p, FQ.p)))
        pt = (rng.randrange(1, FQ.p), y)
        rep = aff_rep(pt, (lx, 1))
        assert rep[17] == digits(2 * FQ.p)[8]
        put("UC_NEG_AFFINE", curve_record(None, "jac", rep, "aff"), exp=o.g1_neg(pt), kind="top_limb")

    for ly in Y_LIFTS:
        for lz in Z_LIFTS:
            p1, zv, q, c2 = top_limb_operands(12)
            rep = jac_rep(p1, zv, (11, ly, lz))
            assert rep[0][8] == digits(12 * FQ.p)[8] and FQ.mont((lifted(q[0], 0), FQ.sqr(rep[0][18:27]))) == digits(c2)
            for neg in (0, 1):
                rec = curve_record(rep, "jac", aff_rep(q, (0, lz)), "aff", neg)
                put("UC_MADD_NZ", rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb")
                put("UC_MADD", rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb")
    for ly in XY_LIFTS:
        for lzz in (0, 1):
            p1, zv, q, c2 = top_limb_operands(8)
            rep = xyzz_rep(p1, zv, (7, ly, lzz, 1 - lzz))
            assert rep[0][8] == digits(8 * FQ.p)[8] and FQ.mont((lifted(q[0], 0), rep[0][18:27])) == digits(c2)
            for neg in (0, 1):
                rec = curve_record(rep, "xyzz", aff_rep(q, (0, lzz)), "aff", neg)
                for name in ("UC_XMADD_FAST", "UC_XMADD_FAST_LOCKSTEP", "UC_XMADD"):
                    put(name, rec, exp=o.g1_add(p1, signed(q, neg)), kind="top_limb", same_x=False)

    # --- Jacobian additions: generic, the same point under different Z (doubling), a point and its negative (identity)
    def full(p1, q, count):
        kind = "equal" if p1[0] == q[0] else "generic"
        for c in range(count):
            l1, l2 = JAC_LIFTS[c % len(JAC_LIFTS)], JAC_LIFTS[(c * 7 + 5) % len(JAC_LIFTS)]
            rec = curve_record(jac_rep(p1, z(), l1), "jac", jac_rep(q, z(), l2), "jac")
            put("UC_ADD_NZ", rec, exp=o.g1_add(p1, q), kind=kind)
            put("UC_ADD", rec, exp=o.g1_add(p1, q), kind=kind)

    for i in range(n):
        full(pts[i], pts[(i + 3) % n], 36)                  # G and 2G meet their negatives here: labelled by their x
        full(pts[i], pts[i], 36)
        full(pts[i], o.g1_neg(pts[i]), 36)

    # --- identity operands of the general forms
    for i, pt in enumerate(pts):
        for la in AFF_LIFTS:
            for neg in (0, 1):
                exp = signed(pt, neg)
                put("UC_MADD", curve_record(jac_rep(None, 1, None), "jac", aff_rep(pt, la), "aff", neg), exp=exp, kind="restart")
                put("UC_XMADD", curve_record(xyzz_rep(None, 1, None), "xyzz", aff_rep(pt, la), "aff", neg), exp=exp, kind="restart", same_x=False)
        lj = JAC_LIFTS[i % len(JAC_LIFTS)]
        put("UC_ADD", curve_record(jac_rep(None, 1, None), "jac", jac_rep(pt, z(), lj), "jac"), exp=pt, kind="identity")
        put("UC_ADD", curve_record(jac_rep(pt, z(), lj), "jac", jac_rep(None, 1, None), "jac"), exp=pt, kind="identity")
    put("UC_ADD", curve_record(jac_rep(None, 1, None), "jac", jac_rep(None, 1, None), "jac"), exp=None, kind="identity")

    # --- chains through the identity and on: every step is a case whose accumulator stands for the model's running sum
    a, b, c = pts[6], pts[7], pts[8]
    chains = [[(a, 0), (b, 0), (a, 1), (b, 1), (c, 0), (c, 0), (c, 0)],            # (a + b) - a - b = identity, restart, double, go on
              [(a, 0), (a, 1), (b, 1), (b, 1), (b, 0), (b, 0), (a, 0)],            # a - a, restart from -b, double it, back down to the identity
              [(c, 1)] + [(c, 0)] * 9]
    for chain in chains:
        cur = None
        for step, (q, neg) in enumerate(chain):
            exp = o.g1_add(cur, signed(q, neg))
            la = AFF_LIFTS[step % 4]
            same_x = cur is not None and cur[0] == q[0]
            put("UC_MADD", curve_record(jac_rep(cur, z(), JAC_LIFTS[(step * 5) % len(JAC_LIFTS)]), "jac", aff_rep(q, la), "aff", neg),
                exp=exp, kind="chain")
            put("UC_XMADD", curve_record(xyzz_rep(cur, z(), XYZZ_LIFTS[(step * 5) % len(XYZZ_LIFTS)]), "xyzz", aff_rep(q, la), "aff", neg),
                exp=exp, kind="chain", same_x=same_x)
            cur = exp
    return {name: (np.array(recs, dtype=np.uint32), meta) for name, (recs, meta) in t.items()}


def check_curve(name, ins, meta, outs, outs_by_op=None):
    """compare every result with the affine group law and its class; returns how many cases were compared.  outs_by_op: the results
    of the other ops over the same table (g1x_madd_fast<true> must be bit-identical to <false>)."""
    assert ins.shape[0] == outs.shape[0] == len(meta) and outs.shape[1] == CURVE_OUT
    compared = 0
    for idx in range(ins.shape[0]):
        rec, out, exp = ins[idx].tolist(), outs[idx].tolist(), meta[idx]["exp"]
        where = f"{name} case {idx} ({meta[idx].get('kind', '')}): in {[hex(x) for x in rec[:37]]} / {[hex(x) for x in rec[40:69]]}"
        co = [out[0:9], out[9:18], out[18:27], out[27:36]]
        if name == "UC_NEG_AFFINE":
            assert co[0] == rec[40:49], where + ": x changed"
            assert m.is_normalised(co[1]) and value(co[1]) <= 3 * FQ.p, where + ": y outside (0, 3p]"
            assert (FQ.elem(co[0]), FQ.elem(co[1])) == exp, where
        elif name in ("UC_XMADD_FAST", "UC_XMADD_FAST_LOCKSTEP"):
            assert out[37] == int(not meta[idx]["same_x"]), where + f": returned {out[37]}"
            if not out[37]:
                assert out[0:37] == rec[0:37], where + ": the accumulator changed although the addition was refused"
            else:
                bad = m.in_class(co, m.XYZZ_CLASS)
                assert not bad and out[36] == 0, where + ": " + bad
                assert m.xyzz_to_affine(*co) == exp, where
            if name == "UC_XMADD_FAST_LOCKSTEP" and outs_by_op is not None:
                assert out == outs_by_op["UC_XMADD_FAST"][idx].tolist(), where + ": lockstep differs from the single products"
        else:
            xyzz = name in ("UC_X_FROM_JAC", "UC_XMADD")
            if out[36]:
                assert exp is None, where + ": identity returned"
            else:
                assert exp is not None, where + ": the identity was expected"
                bad = m.in_class(co, m.XYZZ_CLASS) if xyzz else m.in_class(co[:3], m.JAC_CLASS)
                assert not bad, where + ": " + bad
                got = m.xyzz_to_affine(*co) if xyzz else m.jac_to_affine(*co[:3])
                assert got == exp, where + f": got {got}, expected {exp}"
        compared += 1
    return compared


def branch_coverage(tables):
    """which multiples of p the squares behind the exceptional branches come out as, from the model alone:
    {'madd_hh': {1, 2}, 'madd_rr0': {...}, 'add_hh': ..., 'add_rr0': ..., 'xmadd_pp': ...}"""
    cov = {k: set() for k in ("madd_hh", "madd_rr0", "add_hh", "add_rr0", "xmadd_pp")}
    ins, meta = tables["UC_MADD_NZ"]
    for rec, mt in zip(ins.tolist(), meta):
        if mt["kind"] == "equal":
            hh, rr0 = m.madd_nz_squares(rec[0:9], rec[9:18], rec[18:27], rec[40:49], rec[49:58], rec[68])
            assert hh is not None, "an equal-x case whose h^2 is no multiple of p"
            cov["madd_hh"].add(hh)
            if mt["exp"] is not None:
                assert rr0 is not None
                cov["madd_rr0"].add(rr0)
            else:
                assert rr0 is None
    ins, meta = tables["UC_ADD_NZ"]
    for rec, mt in zip(ins.tolist(), meta):
        if mt["kind"] == "equal":
            hh, rr0 = m.add_nz_squares(rec[0:9], rec[9:18], rec[18:27], rec[40:49], rec[49:58], rec[58:67])
            assert hh is not None
            cov["add_hh"].add(hh)
            if mt["exp"] is not None:
                cov["add_rr0"].add(rr0)
    ins, meta = tables["UC_XMADD_FAST"]
    for rec, mt in zip(ins.tolist(), meta):
        pp = m.xmadd_fast_square(rec[0:9], rec[18:27], rec[40:49])
        assert (pp is not None) == mt["same_x"]
        if pp is not None:
            cov["xmadd_pp"].add(pp)
    return cov


# ---- the case file of the host runner ----------------------------------------------------------------------------------------
def write_blocks(path, blocks):
    """blocks: [(table, op number, (n, words) uint32 array)]"""
    with open(path, "wb") as f:
        for table, op, arr in blocks:
            f.write(np.array([table, op, arr.shape[0]], dtype=np.uint32).tobytes())
            f.write(np.ascontiguousarray(arr, dtype=np.uint32).tobytes())


def read_blocks(path, blocks):
    """the runner's results for `blocks`, in order: [(n, out words) uint32 array]"""
    data = np.fromfile(path, dtype=np.uint32)
    out, at = [], 0
    for table, op, arr in blocks:
        n, words = arr.shape[0], CURVE_OUT if table == 2 else FIELD_OUT
        assert data[at:at + 3].tolist() == [table, op, n], "the result file does not follow the case file"
        out.append(data[at + 3:at + 3 + n * words].reshape(n, words))
        at += 3 + n * words
    assert at == data.size
    return out
