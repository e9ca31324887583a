"""Raw evaluate_h programs for the tests of the lowering in csrc/graph_lower.h and of the interpreter in csrc/graph.hip.

``GraphEvaluator.add_expression`` only ever emits a narrow family of programs (every Store a leaf query ahead of its use,
subexpressions shared, operands ordered, nothing dead, the result the final Horner step); ``hm_graph_create`` accepts any valid
straight-line program.  The programs here fill ``calculations`` / ``constants`` / ``rotations`` of a ``GraphEvaluator`` DIRECTLY, so
that ``GraphEvaluator.lower`` / ``compile`` and ``oracle/graph_ref`` consume them unchanged:

    hand_written()          one named program per rule of the lowering (a failure says which rule broke)
    random_program(seed)    a seeded random program of 5 .. 120 calculations
    shapes(program)         which of the shapes listed in SHAPES a program contains
    make_data / oracle_values / host_replay / lowering_facts / device_against_oracle_and_replay
                            adversarial inputs, the oracle's values, the HM_BOUNDS replay of the lowered program
                            (hc_graph_replay, csrc/host_check.cpp) and what the lowering decided

A plain helper module (like mock_prover.py): tests/test_graph_lowering_host.py, tests/test_graph_programs_gpu.py and
``tools/fuzz.py graph`` share it.
"""
import ctypes
import os
import random
import subprocess
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from halo2_experiments_amd import _lib
from halo2_experiments_amd import evaluation as ev
from halo2_experiments_amd.domain import FR_MODULUS
from oracle import bn256_ref, graph_ref

R = FR_MODULUS

# the column table every program here is compiled for: fixed | advice | instance
NF, NA, NI, NCH = 3, 3, 2, 2
SHORT = {1: 0, 2: 2}                         # column table index -> log2(rows): Fixed(1) has period 1, Fixed(2) period 4
ROTATIONS = [0, 1, -1, 3, -2, 300, -300]     # 300 is larger than every segment used (1, 2, 64, 256 rows)
C_ZERO, C_ONE, C_TWO, C_MINUS1, C_SEVEN, C_BIG = (("Constant", i) for i in range(6))
CONSTANTS = [0, 1, 2, R - 1, 7, 0x2F5A6C1D3E4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEF % R]
PREV = ("PreviousValue",)
DYNAMIC = [("Challenge", 0), ("Challenge", 1), ("Beta",), ("Gamma",), ("Theta",), ("Y",)]

GE_CAP = 16.0                                # csrc/graph_lower.h
GOP = {"Add": 0, "Sub": 1, "Mul": 2, "Square": 3, "Double": 4, "Negate": 5, "Store": 6, "MulAdd": 7}
GF_A_PREV, GF_B_PREV, GF_C_PREV, GF_NO_STORE, GF_NO_REDUCE, GF_SUB_WIDE = (1 << b for b in (8, 9, 10, 11, 12, 13))

# ---- adversarial field values -------------------------------------------------------------------------------------------------
# A column word is the integer v * 2^256 mod r (external form) or v * 2^261 mod r (internal form: what fr_array(32 v) holds).
_ALL_ONES = (((R >> 232) - 1) << 232) | ((1 << 232) - 1)       # the largest canonical integer whose eight low 29-bit limbs are 2^29 - 1
assert _ALL_ONES < R
SPECIAL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
for _word in (R - 1, _ALL_ONES, 1):
    for _shift in (256, 261):
        SPECIAL.append(_word * pow(1 << _shift, -1, R) % R)


def field_value(rng: random.Random) -> int:
    return rng.choice(SPECIAL) if rng.random() < 0.5 else rng.randrange(R)


# ---- programs --------------------------------------------------------------------------------------------------------------------
@dataclass
class Program:
    name: str
    g: ev.GraphEvaluator
    note: str = ""
    _lowered: Dict = field(default=None, repr=False)

    def lower(self) -> Dict:
        """The arguments of hm_graph_create (GraphEvaluator.lower: the words CompiledGraph uploads)."""
        if self._lowered is None:
            self._lowered = self.g.lower(NF, NA, NI, num_challenges=NCH, rot_scale=1, short_columns=SHORT)
        return self._lowered

    def compile(self) -> ev.CompiledGraph:
        return self.g.compile(NF, NA, NI, num_challenges=NCH, rot_scale=1, short_columns=SHORT)

    def describe(self) -> str:
        return f"{self.name}: " + "; ".join(f"t{t} = {c}" for c, t in self.g.calculations)


class Builder:
    """Appends raw calculations; every one gets the next target unless a target order is given at the end."""

    def __init__(self, name: str, note: str = ""):
        self.name, self.note = name, note
        self.g = ev.GraphEvaluator()
        self.g.constants = list(CONSTANTS)
        self.g.rotations = list(ROTATIONS)

    def emit(self, *calc):
        t = len(self.g.calculations)
        self.g.calculations.append((tuple(calc), t))
        return ("Intermediate", t)

    def add(self, a, b): return self.emit("Add", a, b)
    def sub(self, a, b): return self.emit("Sub", a, b)
    def mul(self, a, b): return self.emit("Mul", a, b)
    def square(self, a): return self.emit("Square", a)
    def double(self, a): return self.emit("Double", a)
    def negate(self, a): return self.emit("Negate", a)
    def store(self, a): return self.emit("Store", a)
    def horner(self, start, parts, factor): return self.emit("Horner", start, tuple(parts), factor)

    def product(self):
        """A value of static bound 3 in both column formats: a product of two column cells."""
        return self.mul(("Advice", 0, 0), ("Advice", 1, 1))

    def finish(self, permute_targets: random.Random = None) -> Program:
        g = self.g
        n = len(g.calculations)
        if permute_targets is not None and n:
            perm = list(range(n))
            permute_targets.shuffle(perm)

            def ren(vs):
                if isinstance(vs, tuple) and vs and vs[0] == "Intermediate":
                    return ("Intermediate", perm[vs[1]])
                if isinstance(vs, tuple) and vs and isinstance(vs[0], tuple):       # Horner's parts
                    return tuple(ren(x) for x in vs)
                return vs
            g.calculations = [((c[0],) + tuple(ren(x) for x in c[1:]), perm[t]) for c, t in g.calculations]
        g.num_intermediates = n
        return Program(self.name, g, self.note)


def _col(kind, column, rot):
    return (kind, column, ROTATIONS.index(rot))


def hand_written() -> List[Program]:
    """One program per rule; every one ends in a value that depends on what the rule decides."""
    out = []
    A0, A1, A2 = _col("Advice", 0, 0), _col("Advice", 1, 1), _col("Advice", 2, -1)
    F0, F1r, F2r, I0, I1 = _col("Fixed", 0, 0), _col("Fixed", 1, 1), _col("Fixed", 2, -1), _col("Instance", 0, 3), _col("Instance", 1, -300)
    Y, BETA = ("Y",), ("Beta",)

    def fold(b, vals):
        """Everything that was computed reaches the result: Horner(PreviousValue, vals, Y) as the last calculation."""
        b.horner(PREV, vals, Y)
        return b.finish()

    # -- operations and sources
    b = Builder("every_operation", "each operation once, over leaves")
    v = [b.add(A0, F0), b.sub(A1, I0), b.mul(A2, BETA), b.square(A0), b.double(I1), b.negate(A1), b.store(A2)]
    out.append(fold(b, v))
    b = Builder("horner_0_1_many_parts", "Horner with no part is a copy of its start; with one part one MulAdd; with many a chain")
    h0 = b.horner(A0, [], Y)
    h1 = b.horner(h0, [A1], ("Theta",))
    h5 = b.horner(PREV, [h0, h1, C_SEVEN, A2, h1], ("Gamma",))
    b.horner(h5, [h0], h1)
    out.append(b.finish())
    b = Builder("constants_0_1_2_minus1", "constants 0, 1, 2, r - 1 and a large one in every operand position")
    v = [b.add(C_ZERO, C_MINUS1), b.mul(C_TWO, C_MINUS1), b.sub(C_ZERO, C_ONE), b.negate(C_ZERO), b.double(C_MINUS1), b.square(C_MINUS1),
         b.horner(C_MINUS1, [C_BIG, C_ZERO], C_MINUS1)]
    out.append(fold(b, v))
    b = Builder("columns_and_rotations", "fixed / advice / instance at positive, negative and larger-than-segment rotations; both short columns")
    v = [b.add(_col("Fixed", 0, 300), _col("Advice", 0, -300)), b.mul(_col("Instance", 0, -2), _col("Instance", 1, 3)), b.sub(F1r, F2r),
         b.mul(_col("Fixed", 1, 0), _col("Fixed", 2, 3)), b.add(_col("Fixed", 2, 0), _col("Fixed", 2, 1))]
    out.append(fold(b, v))
    b = Builder("per_call_constants", "Challenge, Beta, Gamma, Theta, Y as operands")
    v = [b.mul(("Challenge", 0), ("Challenge", 1)), b.add(("Beta",), ("Gamma",)), b.sub(("Theta",), Y), b.square(("Challenge", 1))]
    out.append(fold(b, v))
    b = Builder("previous_value_everywhere", "PreviousValue in every operand position and more than once in one calculation")
    v = [b.add(PREV, PREV), b.sub(A0, PREV), b.mul(PREV, A1), b.square(PREV), b.double(PREV), b.negate(PREV), b.horner(PREV, [PREV, PREV], PREV)]
    out.append(fold(b, v))
    # -- Store variants
    b = Builder("store_of_intermediate", "a Store of an intermediate stays an instruction")
    x = b.product()
    s = b.store(x)
    out.append(fold(b, [b.add(s, x), s]))
    b = Builder("store_of_previous_value")
    s = b.store(PREV)
    out.append(fold(b, [b.mul(s, s), s]))
    b = Builder("store_of_constant", "removed by copy propagation: the users read the constant")
    s = b.store(C_MINUS1)
    out.append(fold(b, [b.mul(s, A0), b.add(s, s)]))
    b = Builder("store_of_column_mid_program", "removed by copy propagation for internal-form columns only")
    x = b.product()
    s = b.store(_col("Advice", 2, 3))
    y = b.add(x, s)
    out.append(fold(b, [b.mul(y, s), s]))
    b = Builder("store_chain", "Store of Store of Store: of a column, of a constant, of an intermediate")
    s1 = b.store(b.store(b.store(A0)))
    s2 = b.store(b.store(C_SEVEN))
    s3 = b.store(b.store(b.product()))
    out.append(fold(b, [b.add(s1, s2), b.mul(s2, s3), s1, s3]))
    for nm, leaf in (("constant", C_BIG), ("column", _col("Instance", 1, -1)), ("previous_value", PREV)):
        b = Builder(f"last_store_of_{nm}", "the program's value is an alias of a leaf")
        b.mul(b.product(), A2)
        b.store(leaf)
        out.append(b.finish())
    b = Builder("last_store_of_intermediate", "the program's value is an alias of an earlier intermediate")
    x = b.product()
    b.add(x, A2)
    b.store(x)
    out.append(b.finish())
    b = Builder("only_stores_of_constants", "nothing is left after copy propagation")
    b.store(b.store(C_SEVEN))
    out.append(b.finish())
    # -- liveness
    b = Builder("read_by_next_only", "forwarded in registers, never stored")
    x = b.product()
    y = b.add(x, A2)
    z = b.sub(A0, y)
    b.horner(A1, [z], BETA)                                  # z arrives as MulAdd's third operand
    out.append(b.finish())
    b = Builder("read_by_next_and_much_later", "forwarded AND stored")
    x = b.product()
    y = b.add(x, A2)
    for _ in range(6):
        y = b.mul(y, A1)
    b.add(y, x)
    out.append(b.finish())
    b = Builder("same_value_in_every_position", "Mul(x, x), Add(x, x), MulAdd(x, x, x), forwarded and from a slot")
    x = b.product()
    m = b.mul(x, x)
    h = b.horner(m, [m], m)
    w = b.product()
    q = b.add(x, x)
    out.append(fold(b, [b.horner(x, [x], x), h, w, q, b.sub(w, w)]))
    b = Builder("never_read_values", "dead values in the middle: each still owns a slot for its own instruction")
    x = b.product()
    b.add(x, A2)
    b.mul(x, x)
    y = b.sub(x, A1)
    b.store(y)
    out.append(fold(b, [y, x]))
    b = Builder("dead_last_but_one", "the last calculation does not read the one before it")
    x = b.product()
    b.add(x, x)
    b.mul(x, A2)
    out.append(b.finish())
    b = Builder("final_value_read_earlier_as_alias", "the result is a Store of a value that other calculations read too")
    x = b.product()
    y = b.add(x, A0)
    b.mul(y, y)
    b.store(y)
    out.append(b.finish())
    b = Builder("many_live_then_recycled", "24 values live at once, consumed, then 24 more: the slots of the first group are reused")
    vals = []
    for rnd in range(2):
        grp = [b.mul(_col("Advice", i % 3, [0, 1, -1, 3][i % 4]), _col("Instance", i % 2, [-2, 0, 3][i % 3])) for i in range(24)]
        acc = grp[0]
        for x in grp[1:]:
            acc = b.mul(acc, x) if rnd else b.sub(acc, x)
        vals.append(acc)
    out.append(fold(b, vals))
    b = Builder("targets_in_any_order", "targets need not follow program order")
    x = b.product()
    y = b.add(x, A2)
    z = b.mul(y, x)
    b.horner(PREV, [z, y, x], Y)
    out.append(b.finish(permute_targets=random.Random(4)))
    b = Builder("empty_program", "no calculation: the value is zero")
    out.append(b.finish())
    # -- the static bound analysis at its thresholds (units of r; a product is 3, a constant 1, a column 3 external / 6 internal)
    b = Builder("add_chain_to_16_and_17", "3 + 3 + 3 + 3 + 3 + 1 = 16 stays lazy, + 1 = 17 is reduced")
    x = b.product()
    s = x
    for _ in range(4):
        s = b.add(s, x)
    s16 = b.add(s, C_MINUS1)
    s17 = b.add(s16, C_MINUS1)
    out.append(fold(b, [b.mul(s16, s16), b.mul(s17, s16), s16, s17]))
    b = Builder("double_chain", "1 -> 2 -> 4 -> 8 -> 16 lazy, 32 reduced; 3 -> 6 -> 12 lazy, 24 reduced")
    d, v = C_MINUS1, []
    for _ in range(6):
        d = b.double(d)
        v.append(d)
    d = b.product()
    for _ in range(4):
        d = b.double(d)
        v.append(d)
    out.append(fold(b, v + [b.mul(v[3], v[3])]))
    b = Builder("sub_and_negate_narrow_and_wide", "a subtrahend of bound 3 takes the 4r form, of bound 4 the 20r form")
    x, w = b.product(), b.product()
    y = b.add(w, C_MINUS1)                                    # bound 4
    v = [b.sub(x, w), b.sub(x, y), b.negate(w), b.negate(y), b.sub(y, y), b.sub(C_ZERO, y)]
    s16 = b.add(b.add(b.add(b.add(b.add(x, x), x), x), x), C_ONE)
    out.append(fold(b, v + [b.sub(x, s16), b.negate(s16), b.sub(s16, s16)]))
    b = Builder("sub_minuend_12_and_13", "12 + 4 = 16 stays lazy, 13 + 4 = 17 is reduced")
    x, w = b.product(), b.product()
    m12 = b.add(b.add(b.add(x, x), x), x)
    d16 = b.sub(m12, w)
    m13 = b.add(m12, C_MINUS1)
    d17 = b.sub(m13, w)
    out.append(fold(b, [b.square(d16), b.square(d17), d16, d17]))
    b = Builder("muladd_addend_13_and_14", "3 + 13 = 16 stays lazy, 3 + 14 = 17 is reduced")
    x, w = b.product(), b.product()
    m13 = b.add(b.add(b.add(b.add(x, x), x), x), C_MINUS1)
    m14 = b.add(m13, C_MINUS1)
    h16 = b.horner(w, [m13], x)
    h17 = b.horner(w, [m14], x)
    out.append(fold(b, [b.mul(h16, h16), b.mul(h17, h16), h16, h17]))
    b = Builder("chains_over_columns", "column operands: bound 3 external, 6 internal -- the same program crosses the cap at other places")
    s, v = A0, []
    for i in range(6):
        s = b.add(s, [A1, A2, I0][i % 3])                     # external 6 9 12 15 18> ; internal 12 18> ...
        v.append(s)
    v += [b.double(A0), b.double(b.double(A1)), b.sub(A0, A1), b.negate(A2), b.sub(b.add(A0, A0), A1), b.horner(A0, [A1, b.add(A1, A2)], A2)]
    m = b.add(b.add(b.add(b.product(), A0), A1), C_ONE)       # external 10, internal 16
    v += [b.sub(m, b.product()), b.horner(A0, [m], A1), b.add(m, C_ONE)]
    out.append(fold(b, v))
    return out


# ---- the random generator --------------------------------------------------------------------------------------------------------
_OPS = ["Add", "Sub", "Mul", "Square", "Double", "Negate", "Store", "Horner"]


def random_program(seed: int) -> Program:
    rng = random.Random(seed)
    n = rng.randint(5, 120)
    # one temperament per program, so that the sweep holds deep forwarding chains, wide live sets and lazy-sum ladders alike
    p_last = rng.choice([0.15, 0.4, 0.7])                  # an operand is the previous result
    p_inter = rng.choice([0.2, 0.5, 0.8])                  # ... else an earlier intermediate
    far = rng.choice([0.1, 0.5, 0.9])                      # ... taken uniformly (far) or from the last few
    linear = rng.choice([0.3, 0.6, 0.85])                  # share of Add / Sub / Double / Negate / Horner: walks the bounds up
    p_same = rng.choice([0.05, 0.25])
    b = Builder(f"random[{seed}]")

    def leaf():
        k = rng.randrange(10)
        if k < 2:
            return ("Constant", rng.randrange(len(CONSTANTS)))
        if k < 6:
            kind = rng.choice(["Fixed", "Advice", "Instance"])
            return (kind, rng.randrange({"Fixed": NF, "Advice": NA, "Instance": NI}[kind]), rng.randrange(len(ROTATIONS)))
        if k < 8:
            return rng.choice(DYNAMIC)
        return PREV

    def operand():
        done = len(b.g.calculations)
        if done and rng.random() < p_last:
            return ("Intermediate", done - 1)
        if done and rng.random() < p_inter:
            return ("Intermediate", rng.randrange(done) if rng.random() < far else rng.randrange(max(0, done - 4), done))
        return leaf()

    def operands(k):
        if rng.random() < p_same:
            return [operand()] * k
        return [operand() for _ in range(k)]

    tail = rng.choice(["any", "any", "store_leaf", "store_inter", "dead_before", "horner"])
    while len(b.g.calculations) < n:
        left = n - len(b.g.calculations)
        if left == 1 and tail != "any" and len(b.g.calculations) >= 2:
            done = len(b.g.calculations)
            if tail == "store_leaf":
                b.store(leaf())
            elif tail == "store_inter":
                b.store(("Intermediate", rng.randrange(done)))
            elif tail == "dead_before":
                b.add(("Intermediate", rng.randrange(done - 1)), leaf())
            else:
                b.horner(PREV, [("Intermediate", rng.randrange(done)) for _ in range(rng.randrange(1, 5))], ("Y",))
            break
        if rng.random() < linear:
            op = rng.choice(["Add", "Add", "Sub", "Sub", "Double", "Negate", "Horner"])
        else:
            op = rng.choice(["Mul", "Mul", "Square", "Store", "Store"])
        if op in ("Add", "Sub", "Mul"):
            b.emit(op, *operands(2))
        elif op == "Horner":
            parts = rng.choice([0, 1, 1, 2, 3, 6])
            xs = operands(parts + 2)
            b.horner(xs[0], xs[2:], xs[1])
        else:
            b.emit(op, operand())
    return b.finish(permute_targets=rng if rng.random() < 0.25 else None)


# ---- what a program contains -----------------------------------------------------------------------------------------------------
SHAPES = (["op:" + o for o in _OPS] + ["horner:0", "horner:1", "horner:many"] +
          ["src:" + s for s in ("Constant", "Intermediate", "Fixed", "Advice", "Instance", "Challenge", "Beta", "Gamma", "Theta", "Y", "PreviousValue")] +
          ["const:0", "const:1", "const:2", "const:r-1", "rot:positive", "rot:negative", "rot:beyond_segment", "short:period1", "short:period4",
           "prev:twice_in_one", "store:intermediate", "store:previous", "store:constant", "store:column_mid", "store:chain",
           "last:store_constant", "last:store_column", "last:store_intermediate",
           "live:next_only", "live:next_and_later", "live:same_value_twice", "live:never_read", "live:dead_last_but_one",
           "live:final_read_earlier", "live:many_at_once", "targets:out_of_order"])


def _sources(calc):
    if calc[0] == "Horner":
        return [calc[1], calc[3]] + list(calc[2])
    return list(calc[1:])


def shapes(p: Program) -> set:
    calcs = p.g.calculations
    out = set()
    pos = {t: k for k, (_, t) in enumerate(calcs)}
    readers: Dict[int, List[int]] = {t: [] for _, t in calcs}
    is_store_of = {}
    for k, (c, t) in enumerate(calcs):
        out.add("op:" + c[0])
        srcs = _sources(c)
        if c[0] == "Horner":
            out.add("horner:" + ("0" if not c[2] else "1" if len(c[2]) == 1 else "many"))
        if srcs.count(PREV) > 1:
            out.add("prev:twice_in_one")
        inter = [s[1] for s in srcs if s[0] == "Intermediate"]
        if len(inter) != len(set(inter)):
            out.add("live:same_value_twice")
        for s in srcs:
            out.add("src:" + s[0])
            if s[0] == "Constant" and s[1] < 4:
                out.add("const:" + ["0", "1", "2", "r-1"][s[1]])
            if s[0] in ("Fixed", "Advice", "Instance"):
                rot = p.g.rotations[s[2]]
                out.add("rot:positive" if rot > 0 else "rot:negative" if rot < 0 else "rot:zero")
                if abs(rot) >= 256:
                    out.add("rot:beyond_segment")
                if s[0] == "Fixed" and s[1] in SHORT and rot != 0:
                    out.add("short:period1" if SHORT[s[1]] == 0 else "short:period4")
            if s[0] == "Intermediate":
                readers[s[1]].append(k)
        if c[0] == "Store":
            s, last = c[1], k == len(calcs) - 1
            is_store_of[t] = s
            kind = {"Intermediate": "intermediate", "PreviousValue": "previous", "Constant": "constant"}.get(s[0], "column" if len(s) == 3 else "dynamic")
            if last and kind in ("constant", "column", "intermediate"):
                out.add("last:store_" + kind)
            if kind == "column" and 0 < k:
                out.add("store:column_mid")
            elif kind != "column":
                out.add("store:" + kind)
            if s[0] == "Intermediate" and s[1] in is_store_of:
                out.add("store:chain")
        if t != k:
            out.add("targets:out_of_order")
    n = len(calcs)
    live_ends = []
    for k, (c, t) in enumerate(calcs):
        rs = readers[t]
        if not rs and k < n - 1:
            out.add("live:never_read")
            if k == n - 2:
                out.add("live:dead_last_but_one")
        if rs and all(r == k + 1 for r in rs):
            out.add("live:next_only")
        if k + 1 in rs and any(r > k + 8 for r in rs):
            out.add("live:next_and_later")
        live_ends.append(max(rs) if rs else k)
    if n:
        last_c, last_t = calcs[-1]
        final = last_c[1][1] if last_c[0] == "Store" and last_c[1][0] == "Intermediate" else last_t
        if any(r < n - 1 for r in readers[final]):
            out.add("live:final_read_earlier")
    if any(sum(1 for j in range(k) if live_ends[j] > k) >= 12 for k in range(n)):
        out.add("live:many_at_once")
    return out


# ---- inputs, the oracle, the host replay ---------------------------------------------------------------------------------------
SEGMENT_ROWS, SEGMENT_COUNTS = (1, 2, 64, 256), (1, 2, 8)


@dataclass
class Data:
    seg: int
    segments: int
    table: List[List[int]]        # NF + NA + NI columns; a short column holds its period only
    previous: List[int]
    challenges: List[int]
    beta: int
    gamma: int
    theta: int
    y: int

    @property
    def size(self):
        return self.seg * self.segments

    def scalars(self):
        return dict(challenges=self.challenges, beta=self.beta, gamma=self.gamma, theta=self.theta, y=self.y)


def make_data(rng: random.Random, seg: int, segments: int, uniform: bool = False) -> Data:
    size = seg * segments
    val = (lambda: rng.randrange(R)) if uniform else (lambda: field_value(rng))
    table = [[val() for _ in range((1 << SHORT[i]) if i in SHORT else size)] for i in range(NF + NA + NI)]
    return Data(seg, segments, table, [val() for _ in range(size)], [field_value(rng) for _ in range(NCH)],
                *(field_value(rng) for _ in range(4)))


def oracle_rows(p: Program, d: Data, rows, previous=None) -> List[int]:
    """oracle/graph_ref on the listed rows: a rotation wraps inside its segment, a short column is read at row mod its length."""
    previous = d.previous if previous is None else previous
    base = {"Fixed": 0, "Advice": NF, "Instance": NF + NA}
    out = []
    for idx in rows:
        s0 = idx - idx % d.seg
        cell = lambda kind, col, row: d.table[base[kind] + col][(s0 + row) % len(d.table[base[kind] + col])]
        out += graph_ref.evaluate_graph_rows(p.g.calculations, p.g.constants, p.g.rotations, cell, d.challenges, d.beta, d.gamma, d.theta, d.y,
                                             {idx - s0: previous[idx]}, [idx - s0], 1, d.seg)
    return out


def oracle_values(p: Program, d: Data, previous=None) -> List[int]:
    return oracle_rows(p, d, range(d.size), previous)


def words(values) -> np.ndarray:
    """Python integers -> the (n, 4) external Montgomery words the library reads."""
    return np.ascontiguousarray(bn256_ref.fr_array(list(values))).reshape(-1, 4)


def column_words(d: Data, internal: bool) -> List[np.ndarray]:
    return [words([32 * v % R for v in c] if internal else c) for c in d.table]


def hostcheck():
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    hc = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    hc.hc_graph_replay.restype = ctypes.c_int
    hc.hc_graph_last_error.restype = ctypes.c_char_p
    return hc


@dataclass
class Replay:
    rc: int
    values: np.ndarray             # (size, 4) words
    lowered: np.ndarray            # (lowered calculations, 5) words: op | flags, a, b, c, target slot
    static_bound: np.ndarray
    tracked_bound: np.ndarray
    n_slots: int
    result_src: int
    result_prev: int
    removed_constant_stores: int
    removed_column_stores: int
    error: str = ""


def host_replay_raw(hc, calcs, constants, n_dynamic, rotations, n_columns, n_intermediates, columns, dyn, log_segment, segments, internal, previous) -> Replay:
    """hc_graph_replay on the arguments of hm_graph_create plus one call's inputs (numpy word arrays)."""
    P32, P64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    calcs = np.ascontiguousarray(calcs, dtype=np.uint32).reshape(-1, 5)
    n = calcs.shape[0]
    consts = words(constants) if len(constants) else np.zeros((1, 4), dtype=np.uint64)
    dyn = np.ascontiguousarray(dyn, dtype=np.uint64).reshape(-1, 4) if n_dynamic else np.zeros((1, 4), dtype=np.uint64)
    rots = np.array(list(rotations) or [0], dtype=np.int32)
    cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
    ptrs = (ctypes.c_void_p * max(len(cols), 1))(*[c.ctypes.data for c in cols])
    rows = np.array([c.shape[0] for c in cols] or [0], dtype=np.uint64)
    values = np.ascontiguousarray(previous, dtype=np.uint64).copy()
    lowered, sb, tb = np.zeros((max(n, 1), 5), dtype=np.uint32), np.zeros(max(n, 1)), np.zeros(max(n, 1))
    info = np.zeros(8, dtype=np.uint32)
    rc = hc.hc_graph_replay(calcs.ctypes.data_as(P32), ctypes.c_size_t(n), consts.ctypes.data_as(P64), ctypes.c_size_t(len(constants)),
                            dyn.ctypes.data_as(P64), ctypes.c_size_t(n_dynamic), rots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                            ctypes.c_size_t(len(rotations)), ptrs, rows.ctypes.data_as(P64), ctypes.c_size_t(n_columns),
                            ctypes.c_uint32(n_intermediates), ctypes.c_uint32(log_segment), ctypes.c_uint32(segments), ctypes.c_uint32(1 if internal else 0),
                            values.ctypes.data_as(P32), lowered.ctypes.data_as(P32), sb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                            tb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), info.ctypes.data_as(P32))
    k = int(info[0])
    return Replay(rc, values, lowered[:k], sb[:k], tb[:k], int(info[1]), int(info[2]), int(info[3]), int(info[4]), int(info[5]),
                  hc.hc_graph_last_error().decode() if rc == -1 else "")


def host_replay(hc, p: Program, d: Data, internal: bool, previous=None, scalars=None) -> Replay:
    low = p.lower()
    sc = scalars or d.scalars()
    cols = column_words(d, internal)
    for i, lg in SHORT.items():
        if lg == 0:
            cols[i] = np.repeat(cols[i], 2, axis=0)            # as CompiledGraph.evaluate passes a one-row column
    dyn = words(list(sc["challenges"]) + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]])
    return host_replay_raw(hc, low["calcs"], low["constants"], low["n_dynamic"], low["rotations"], low["n_columns"], low["n_intermediates"],
                           cols, dyn, d.seg.bit_length() - 1, d.segments, internal, words(d.previous if previous is None else previous))


def lowering_facts(r: Replay) -> set:
    """What the lowering decided for one program, as the coverage items of tests/test_graph_lowering_host.py."""
    names = {v: k for k, v in GOP.items()}
    out = {"result_prev:%d" % r.result_prev}
    if (r.result_src >> 30) != 1:
        out.add("result:not_intermediate")
    if r.removed_constant_stores:
        out.add("copy_propagated:constant")
    if r.removed_column_stores:
        out.add("copy_propagated:column")
    written = set()
    for op, a, b, c, target in r.lowered.tolist():
        name = names[op & 0xFF]
        out.add("op:" + name)
        if name in ("Add", "Double", "Sub", "Negate", "MulAdd"):          # GF_NO_REDUCE set / clear; a Negate is only ever reduced as a wide one
            out.add(f"{name}:{'lazy' if op & GF_NO_REDUCE else 'reduced'}")
            if name == "Sub" and not op & (GF_NO_REDUCE | GF_SUB_WIDE):
                out.add("Sub:reduced_narrow")
        if op & GF_SUB_WIDE:
            out.add("GF_SUB_WIDE:" + name)
        for flag, nm in ((GF_A_PREV, "GF_A_PREV"), (GF_B_PREV, "GF_B_PREV"), (GF_C_PREV, "GF_C_PREV"), (GF_NO_STORE, "GF_NO_STORE")):
            if op & flag:
                out.add(nm)
        if not op & GF_NO_STORE:
            if target in written:
                out.add("slot:recycled")
            written.add(target)
    return out


REQUIRED_FACTS = (["op:" + n for n in GOP] + [f"{n}:{m}" for n in ("Add", "Double", "Sub", "Negate", "MulAdd") for m in ("lazy", "reduced")] +
                  ["Sub:reduced_narrow", "GF_SUB_WIDE:Sub", "GF_SUB_WIDE:Negate", "GF_A_PREV", "GF_B_PREV", "GF_C_PREV", "GF_NO_STORE", "copy_propagated:constant",
                   "result_prev:0", "result_prev:1", "result:not_intermediate", "slot:recycled"])


def check_replay(p: Program, r: Replay, expected: List[int], what: str) -> List[str]:
    """The host file's assertions on one replay, as a list of failures (empty: all hold)."""
    bad = []
    if r.rc != 0:
        return [f"{what}: hc_graph_replay returned {r.rc} {r.error}"]
    if not np.array_equal(r.values, words(expected)):
        row = int(np.nonzero((r.values != words(expected)).any(axis=1))[0][0])
        bad.append(f"{what}: value differs from the oracle first at row {row}")
    for k, (row5, sb, tb) in enumerate(zip(r.lowered.tolist(), r.static_bound.tolist(), r.tracked_bound.tolist())):
        if tb > sb + 1e-9:
            bad.append(f"{what}: lowered calculation {k} (op {row5[0]:#x}): tracked bound {tb} above the static bound {sb}")
        if sb > GE_CAP:
            bad.append(f"{what}: lowered calculation {k} (op {row5[0]:#x}): static bound {sb} of a stored or forwarded value above GE_CAP")
    return bad


# ---- the device ------------------------------------------------------------------------------------------------------------------
def to_device(word_rows: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(word_rows).view(np.int64)).cuda()


def device_columns(d: Data, internal: bool):
    return [to_device(c) for c in column_words(d, internal)]


def device_values(values) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return values.cpu().numpy().view(np.uint64)


def other_scalars(rng: random.Random) -> Dict:
    return dict(challenges=[field_value(rng) for _ in range(NCH)], beta=field_value(rng), gamma=field_value(rng), theta=field_value(rng),
                y=field_value(rng))


def device_against_oracle_and_replay(hc, p: Program, d: Data, rng: random.Random) -> List[str]:
    """One program on the device, both column formats, and a second call on the same handle with other per-call constants chained
    through PreviousValue (the slots then hold the first call's leftovers): device == oracle, device == host replay, word for word.
    -> failures."""
    bad = []
    exp = oracle_values(p, d)
    sc2 = other_scalars(rng)
    d2 = Data(d.seg, d.segments, d.table, exp, **sc2)
    exp2 = oracle_values(p, d2)
    prog = p.compile()
    try:
        for internal in (False, True):
            fmt = "internal" if internal else "external"
            cols = device_columns(d, internal)
            values = to_device(words(d.previous))
            for call, (dd, want) in enumerate(((d, exp), (d2, exp2))):
                what = f"{p.name} seg={d.seg} segments={d.segments} {fmt} call {call}"
                prog.evaluate(cols, values, columns_internal=internal, segments=d.segments, **dd.scalars())
                got = device_values(values)
                if not np.array_equal(got, words(want)):
                    bad.append(f"{what}: device differs from the oracle first at row {int(np.nonzero((got != words(want)).any(axis=1))[0][0])}")
                if hc is not None:
                    r = host_replay(hc, p, dd, internal)
                    if r.rc != 0 or not np.array_equal(got, r.values):
                        bad.append(f"{what}: device differs from the host replay (rc {r.rc})")
    finally:
        prog.destroy()
    if bad:
        bad.append(p.describe())
    return bad
