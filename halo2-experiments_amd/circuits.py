"""The constraint systems of the reference's three `create_proof` configurations (BASELINE.json configs 2-4), as expression
lists for the ``GraphEvaluator`` mirror of evaluation.py -- what ``evaluate_h`` runs per row of the extended domain.

What is transcribed from files of the reference (read as text; cited per gate) and what is recalled:

    MerkleSumTree  /root/reference/src/chips/merkle_sum_tree.rs:32-138    bool / swap / sum gates, the `check == is_lt` gate, the
                   column set (5 chip columns + 5 hash inputs), equality columns: TRANSCRIBED
    MerkleTreeV3   /root/reference/src/chips/merkle_v3.rs:30-82           bool / swap gates, column set: TRANSCRIBED
    Poseidon       /root/reference/src/chips/poseidon/hash.rs:45-72       which columns PoseidonChip::configure allocates
                   (partial_sbox, rc_a, rc_b, equality on the hash inputs, constants in rc_b[0]): TRANSCRIBED
    OverflowCheckV2, SafeAccumulator   the reference's experiments 16 and 17 (``overflow_check_v2``, ``safe_accumulator`` below cite their
                   lines; IsZeroChip and range_check with the latter): TRANSCRIBED
    Pow5Chip       halo2_gadgets::poseidon::Pow5Chip::configure ("full round", "partial rounds", "pad-and-add" gates): RECALLED --
                   the crate is a git dependency that is not in this image (/root/reference/Cargo.toml:11)
    LtChip         zkevm-circuits gadgets::less_than::LtChip::configure ("lt gate": lhs - rhs - sum diff_i 256^i + lt * 2^(8 N);
                   bool check of lt; one u8-range lookup per diff byte): RECALLED (/root/reference/Cargo.toml:14)

The MDS matrix, its inverse and the round constants of the Spec are generic field elements here (halo2_gadgets derives
them with a Grain LFSR): the program's shape -- calculations, rotations, columns -- does not depend on their values.
With a ``poseidon.Spec`` (``merkle_sum_tree(spec)`` ...) the MDS matrix and its inverse are the spec's: the system a witness
can satisfy (synthesis.py fills the round-constant columns from the same spec).
Selectors are fixed columns, one each (what keygen gives with selector compression off; compression only merges columns).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Sequence, Tuple

from .evaluation import (Advice, Challenge, Constant, Expression, Fixed, GraphEvaluator, Instance, Negated, Product, Scaled, Sum,
                         logup_expressions, lookup_expressions, permutation_expressions)
from .domain import FR_MODULUS

R = FR_MODULUS


def degree(e: Expression) -> int:
    """Expression::degree (plonk/circuit.rs): columns 1, constants 0, products add, sums take the maximum."""
    if isinstance(e, (Fixed, Advice, Instance)):
        return 1
    if isinstance(e, Sum):
        return max(degree(e.a), degree(e.b))
    if isinstance(e, Product):
        return degree(e.a) + degree(e.b)
    if isinstance(e, Negated):
        return degree(e.a)
    if isinstance(e, Scaled):
        return degree(e.a)
    return 0


class _Columns:
    """meta.advice_column() / fixed_column() / selector() / instance_column() in allocation order."""

    def __init__(self):
        self.num_advice = self.num_fixed = self.num_instance = 0
        self.equality: List[Tuple[str, int]] = []          # columns in the permutation argument, in enabling order

    def advice(self) -> int:
        self.num_advice += 1
        return self.num_advice - 1

    def fixed(self) -> int:
        self.num_fixed += 1
        return self.num_fixed - 1

    selector = fixed

    def instance(self) -> int:
        self.num_instance += 1
        return self.num_instance - 1

    def enable_equality(self, kind: str, index: int) -> None:
        if (kind, index) not in self.equality:
            self.equality.append((kind, index))


@dataclass
class ConstraintSystem:
    name: str
    source: str
    num_fixed: int
    num_advice: int
    num_instance: int
    gates: List[Tuple[str, List[Expression]]]
    lookups: List[Tuple[List[Expression], List[Expression]]]          # (input expressions, table expressions)
    equality: List[Tuple[str, int]]
    blinding_factors: int = 5
    # advice columns whose last rows (row >= n - blinding_factors - 1) the prover leaves ZERO instead of drawing blinding for them:
    # their commitment is then ``commit_lagrange`` of the witness column itself -- deterministic, and not hiding
    unblinded_advice: Tuple[int, ...] = ()
    # what the system was built with, where a caller needs it back (overflow_check_v2: max_bits, acc_cols)
    parameters: Dict[str, int] = field(default_factory=dict)

    def polynomials(self) -> List[Expression]:
        return [p for _, polys in self.gates for p in polys]

    def degree(self) -> int:
        """ConstraintSystem::degree: max over the permutation argument (3), the lookup arguments (max(4, 2 + input + table
        degree)) and the gate polynomials."""
        d = 3 if self.equality else 1
        for ins, tabs in self.lookups:
            d = max(d, 4, 2 + max(degree(e) for e in ins) + max(degree(e) for e in tabs))
        for p in self.polynomials():
            d = max(d, degree(p))
        return d

    def queries(self) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]], List[Tuple[int, int]]]:
        """(advice, fixed, instance) queries as (column, rotation) lists: the evaluations a proof carries.  In order of first use in
        the gate polynomials, then in the lookups' input and table expressions, then every equality column at rotation 0 (upstream's
        ``enable_equality`` queries it).  Upstream's order is that of the ``meta.query_*`` calls inside its chips; this one is a
        function of the expressions alone."""
        found: Dict[str, List[Tuple[int, int]]] = {"advice": [], "fixed": [], "instance": []}
        kinds = {Advice: "advice", Fixed: "fixed", Instance: "instance"}

        def walk(e: Expression) -> None:
            if type(e) in kinds:
                q = (e.column, e.rotation)
                if q not in found[kinds[type(e)]]:
                    found[kinds[type(e)]].append(q)
            elif isinstance(e, (Sum, Product)):
                walk(e.a)
                walk(e.b)
            elif isinstance(e, (Negated, Scaled)):
                walk(e.a)

        for p in self.polynomials():
            walk(p)
        for ins, tabs in self.lookups:
            for e in list(ins) + list(tabs):
                walk(e)
        for kind, index in self.equality:
            if (index, 0) not in found[kind]:
                found[kind].append((index, 0))
        return found["advice"], found["fixed"], found["instance"]

    def logup_arguments(self) -> List[Tuple[List[Expression], List[List[Expression]]]]:
        """The arguments of ``lookup="logup"`` as (table expressions, [input expression lists]): a pure function
        of the lookups.  With D = ``degree()`` the lookups are walked in order; a lookup joins the open argument whose table expression
        list is structurally equal to its own if afterwards 2 + deg(table) + sum_j deg(input_j) <= D (the degree of a list is the
        maximum over its members), otherwise it opens a new argument for that table, which becomes the open one for that table.  A
        lookup alone always fits, by the definition of D, so asking never raises the degree: ``extended_k`` and the keys stay."""
        D = self.degree()
        deg = lambda exprs: max(degree(e) for e in exprs)
        out: List[Tuple[List[Expression], List[List[Expression]]]] = []
        open_for: List[int] = []                           # per distinct table, in order of first use: its open argument
        for ins, tabs in self.lookups:
            at = next((g for g in open_for if out[g][0] == list(tabs)), None)
            if at is not None and 2 + deg(tabs) + sum(deg(i) for i in out[at][1]) + deg(ins) <= D:
                out[at][1].append(list(ins))
                continue
            if at is not None:
                open_for.remove(at)
            open_for.append(len(out))
            out.append((list(tabs), [list(ins)]))
        return out

    def permutation_chunk_len(self) -> int:
        return self.degree() - 2

    def permutation_sets(self) -> int:
        c = self.permutation_chunk_len()
        return (len(self.equality) + c - 1) // c


def _rand_constants(count: int, seed: int) -> List[int]:
    x, out = seed, []
    for _ in range(count):
        x = pow(x, 5, R) * 7 % R + 1                      # any generic non-zero elements (see the module docstring)
        out.append(x)
    return out


def pow5_gates(state: Sequence[int], partial_sbox: int, rc_a: Sequence[int], rc_b: Sequence[int], s_full: int, s_partial: int,
               s_pad_and_add: int, rate: int, constants=None) -> List[Tuple[str, List[Expression]]]:
    """halo2_gadgets Pow5Chip::configure (recalled): the three gates of the Poseidon permutation chip over `state` (WIDTH
    advice columns), `partial_sbox`, the round-constant columns rc_a / rc_b and three selectors.
    constants: a ``poseidon.Spec`` whose ``mds`` / ``mds_inv`` become m_reg / m_inv (what a witness can satisfy: synthesis.py);
    None: generic elements, the shape-only form."""
    width = len(state)
    if constants is None:
        m_reg = [_rand_constants(width, 1000 + i) for i in range(width)]
        m_inv = [_rand_constants(width, 2000 + i) for i in range(width)]
    else:
        if constants.width != width:
            raise ValueError(f"pow5_gates: the spec has width {constants.width}, the chip has {width} state columns")
        _, mds, mds_inv = constants.constants()
        m_reg, m_inv = [list(row) for row in mds], [list(row) for row in mds_inv]

    def pow_5(v: Expression) -> Expression:
        v2 = v * v
        return v2 * v2 * v

    full = []
    for nxt in range(width):
        expr = None
        for idx in range(width):
            term = pow_5(Advice(state[idx]) + Fixed(rc_a[idx])) * m_reg[nxt][idx]
            expr = term if expr is None else expr + term
        full.append(Fixed(s_full) * (expr - Advice(state[nxt], 1)))

    cur_0, mid_0 = Advice(state[0]), Advice(partial_sbox)

    def mid(idx: int) -> Expression:
        acc = mid_0 * m_reg[idx][0]
        for j in range(1, width):
            acc = acc + (Advice(state[j]) + Fixed(rc_a[j])) * m_reg[idx][j]
        return acc

    def nxt_lin(idx: int) -> Expression:
        acc = None
        for j in range(width):
            t = Advice(state[j], 1) * m_inv[idx][j]
            acc = t if acc is None else acc + t
        return acc

    partial = [Fixed(s_partial) * (pow_5(cur_0 + Fixed(rc_a[0])) - mid_0),
               Fixed(s_partial) * (pow_5(mid(0) + Fixed(rc_b[0])) - nxt_lin(0))]
    for idx in range(1, width):
        partial.append(Fixed(s_partial) * (mid(idx) + Fixed(rc_b[idx]) - nxt_lin(idx)))

    pad = [Fixed(s_pad_and_add) * (Advice(state[i], -1) + Advice(state[i]) - Advice(state[i], 1)) for i in range(rate)]
    pad.append(Fixed(s_pad_and_add) * (Advice(state[rate], -1) - Advice(state[rate], 1)))
    return [("full round", full), ("partial rounds", partial), ("pad-and-add", pad)]


def _poseidon_chip(cols: _Columns, hash_inputs: Sequence[int], rate: int, spec=None):
    """PoseidonChip::configure, /root/reference/src/chips/poseidon/hash.rs:45-72: partial_sbox, rc_a, rc_b, equality on the
    hash inputs, constants in rc_b[0]; then Pow5Chip::configure (which allocates its three selectors)."""
    width = len(hash_inputs)
    partial_sbox = cols.advice()
    rc_a = [cols.fixed() for _ in range(width)]
    rc_b = [cols.fixed() for _ in range(width)]
    for c in hash_inputs:
        cols.enable_equality("advice", c)
    cols.enable_equality("fixed", rc_b[0])                 # meta.enable_constant(rc_b[0])
    s_full, s_partial, s_pad = cols.selector(), cols.selector(), cols.selector()
    return pow5_gates(hash_inputs, partial_sbox, rc_a, rc_b, s_full, s_partial, s_pad, rate, constants=spec)


def lt_chip(cols: _Columns, q_enable: Expression, lhs: Expression, rhs: Expression, n_bytes: int = 8):
    """gadgets::less_than::LtChip::configure (recalled): -> (gates, lookups, the `lt` column)."""
    lt = cols.advice()
    diff = [cols.advice() for _ in range(n_bytes)]
    u8 = cols.fixed()
    from_bytes = None
    for i, c in enumerate(diff):
        t = Advice(c) * pow(256, i, R)
        from_bytes = t if from_bytes is None else from_bytes + t
    check_a = lhs - rhs - from_bytes + Advice(lt) * pow(2, 8 * n_bytes, R)
    check_b = Advice(lt) * (Constant(1) - Advice(lt))
    gates = [("lt gate", [q_enable * check_a, q_enable * check_b])]
    lookups = [([Advice(c)], [Fixed(u8)]) for c in diff]
    return gates, lookups, lt


def merkle_sum_tree(spec=None) -> ConstraintSystem:
    """MerkleSumTreeChip::configure, /root/reference/src/chips/merkle_sum_tree.rs:32-138 (WIDTH 5, RATE 4, LtChip over 8 bytes).
    spec: the width-5 ``poseidon.Spec`` whose MDS matrix the Pow5 gates take (see pow5_gates)."""
    cols = _Columns()
    a, b, c, d, e = (cols.advice() for _ in range(5))      # circuits/merkle_sum_tree.rs:27-31
    inst = cols.instance()
    bool_s, swap_s, sum_s, lt_s = (cols.selector() for _ in range(4))          # :44-47
    for col in (a, b, c, d, e):                                                # :53-57
        cols.enable_equality("advice", col)
    cols.enable_equality("instance", inst)                                     # :58
    A = Advice
    gates = [
        ("bool constraint", [Fixed(bool_s) * A(e) * (Constant(1) - A(e))]),                                          # :62-66
        ("swap constraint", [Fixed(swap_s) * (A(e) * Constant(2) * (A(c) - A(a)) - (A(a, 1) - A(a)) - (A(c) - A(c, 1))),    # :70-92
                             Fixed(swap_s) * (A(e) * Constant(2) * (A(d) - A(b)) - (A(b, 1) - A(b)) - (A(d) - A(d, 1)))]),
        ("sum constraint", [Fixed(sum_s) * (A(b) + A(d) - A(e))]),                                                   # :95-101
    ]
    hash_inputs = [cols.advice() for _ in range(5)]                                                                  # :103
    gates += _poseidon_chip(cols, hash_inputs, rate=4, spec=spec)                                                    # :105-106
    lt_gates, lookups, lt = lt_chip(cols, Fixed(lt_s), A(a), A(b))                                                   # :109-114
    gates += lt_gates
    gates.append(("check == is_lt", [Fixed(lt_s) * (A(lt) - A(c))]))                                                 # :127-138
    return ConstraintSystem("MerkleSumTree depth 20 (config 4)", "chips/merkle_sum_tree.rs:32-138 (+ Pow5Chip, LtChip recalled)",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, lookups, cols.equality)


def merkle_v3(spec=None) -> ConstraintSystem:
    """MerkleTreeV3Chip::configure, /root/reference/src/chips/merkle_v3.rs:30-82 (WIDTH 3, RATE 2)."""
    cols = _Columns()
    a, b, c = (cols.advice() for _ in range(3))
    inst = cols.instance()
    bool_s, swap_s = cols.selector(), cols.selector()                          # :38-39
    for col in (a, b, c):                                                      # :41-43
        cols.enable_equality("advice", col)
    cols.enable_equality("instance", inst)                                     # :44
    A = Advice
    gates = [
        ("bool constraint", [Fixed(bool_s) * A(c) * (Constant(1) - A(c))]),                                          # :48-52
        ("swap constraint", [Fixed(swap_s) * (A(c) * Constant(2) * (A(b) - A(a)) - (A(a, 1) - A(a)) - (A(b) - A(b, 1)))]),  # :57-68
    ]
    hash_inputs = [cols.advice() for _ in range(3)]                                                                  # :70
    gates += _poseidon_chip(cols, hash_inputs, rate=2, spec=spec)                                                    # :72-73
    return ConstraintSystem("MerkleTreeV3 depth 20 (config 3)", "chips/merkle_v3.rs:30-82 (+ Pow5Chip recalled)",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, [], cols.equality)


def poseidon(spec=None) -> ConstraintSystem:
    """PoseidonCircuit::configure, /root/reference/src/circuits/poseidon.rs:36-41 with WIDTH 5, RATE 4 (:79-81): the hash
    inputs, an instance column for the digest, PoseidonChip (hash_with_instance.rs: the same allocations + equality on the
    instance column)."""
    cols = _Columns()
    inst = cols.instance()
    hash_inputs = [cols.advice() for _ in range(5)]
    gates = _poseidon_chip(cols, hash_inputs, rate=4, spec=spec)
    cols.enable_equality("instance", inst)
    return ConstraintSystem("Poseidon (config 2)", "circuits/poseidon.rs:36-41, chips/poseidon/hash_with_instance.rs (+ Pow5Chip recalled)",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, [], cols.equality)


def overflow_check_v2(max_bits: int = 4, acc_cols: int = 4, unblinded_value: bool = False) -> ConstraintSystem:
    """OverflowCheckCircuitV2::configure, /root/reference/src/circuits/overflow_check_v2.rs:21-39, with OverflowChipV2::configure,
    /root/reference/src/chips/overflow_check_v2.rs:31-78 (TRANSCRIBED; the reference instantiates <4, 4> only): advice 0 the value,
    advice 1 .. acc_cols its limbs of max_bits bits, most significant first; fixed 0 the range column 0 .. 2^max_bits - 1, fixed 1
    the selector; an instance column that stays empty; equality on the limb columns only, and no copies.  One gate,
    sum limb_i * 2^(max_bits * (acc_cols - 1 - i)) = value, and one lookup per limb column into the range column.  On every row where
    the selector is set the value is below 2^(max_bits * acc_cols); with max_bits * acc_cols <= 253 the limb sum cannot wrap mod r.

    unblinded_value: ``unblinded_advice = (0,)`` -- the prover leaves the last rows of the value column zero, so the proof's first
    commitment is ``params.commit_lagrange`` of the value column padded with zeros: the commitment ``open_all`` / ``open_at`` open.
    The trade-off: that commitment is deterministic, which is what a published balance commitment wants (every user checks an
    opening of the SAME point) and what blinding would break; it hides nothing beyond what the discrete logarithm hides, so equal
    columns give equal commitments and a guessed column can be confirmed."""
    if not 1 <= max_bits <= 16:
        raise ValueError("overflow_check_v2: max_bits must be 1 .. 16")
    if acc_cols < 1 or max_bits * acc_cols > 253:
        raise ValueError("overflow_check_v2: acc_cols must be at least 1 and max_bits * acc_cols at most 253 (the limb sum must not wrap mod r)")
    cols = _Columns()
    value = cols.advice()                                                      # circuits/overflow_check_v2.rs:22-26
    limbs = [cols.advice() for _ in range(acc_cols)]
    rng = cols.fixed()                                                         # :27
    selector = cols.selector()                                                 # :28
    cols.instance()                                                            # :29
    for col in limbs:                                                          # chips/overflow_check_v2.rs:39
        cols.enable_equality("advice", col)
    total: Expression = Advice(limbs[acc_cols - 1])                            # :50-56
    for i in range(acc_cols - 1):
        total = total + Advice(limbs[i]) * Constant(1 << (max_bits * (acc_cols - 1 - i)))
    gates = [("equality check between decomposed value and value", [Fixed(selector) * (total - Advice(value))])]   # :41-59
    lookups = [([Advice(col)], [Fixed(rng)]) for col in limbs]                 # :63-69
    return ConstraintSystem(f"OverflowCheckV2<{max_bits}, {acc_cols}>", "circuits/overflow_check_v2.rs:21-39, chips/overflow_check_v2.rs:31-78",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, lookups, cols.equality,
                            unblinded_advice=(value,) if unblinded_value else (), parameters=dict(max_bits=max_bits, acc_cols=acc_cols))


def sorted_column(max_bits: int = 4, acc_cols: int = 4) -> ConstraintSystem:
    """"This committed column holds pairwise distinct ids" (DESIGN.md section 32).  This circuit is the project's own: it is NOT
    transcribed from the reference, which has nothing of the kind; only its shape follows ``overflow_check_v2``, whose limb
    decomposition and range lookups it uses.  Advice 0 is the id, ``unblinded_advice = (0,)``, so a proof's first commitment is
    ``params.commit_lagrange`` of the id column padded with zeros -- the very point ``ledger.py`` publishes and ``open_all`` opens;
    advice 1 .. acc_cols are the limbs of the gap to the next row, max_bits bits each, most significant first; fixed 0 the range
    column 0 .. 2^max_bits - 1, fixed 1 the selector; an instance column that stays empty; equality on the limb columns only, and no
    copies.  One gate, with B = max_bits * acc_cols,

        sel * (id[i+1] - id[i] - 1 - sum_j limb_j[i] * 2^(max_bits * (acc_cols - 1 - j))),

    and one lookup per limb column into the range column, so every limb is in [0, 2^max_bits).  ``synthesis.SortedColumnLayout`` sets
    the selector on rows 0 .. rows - 2 of a column with ``rows`` live rows.

    What it proves.  On those rows id[i+1] - id[i] - 1 = d_i mod r for an integer 0 <= d_i < 2^B, so id[i] = id[0] + s_i mod r with
    the integers s_0 = 0 and s_i = s_(i-1) + d_(i-1) + 1: 0 = s_0 < s_1 < .. < s_(rows-1) <= (rows - 1) * 2^B < 2^(k + B).  With
    B + k <= 253 every s_i is below 2^253 < r, so no two of them agree mod r, and the ids are pairwise distinct WHATEVER id[0] is --
    a run that wraps past r (r - 2, r - 1, 0, 1) stays distinct.  B <= 253 is checked here, as in ``overflow_check_v2``; B + k <= 253
    needs k and is checked by the layout.  Nothing else is claimed: the ids need not be small, only apart by less than 2^B in sorted
    order, which ids below 2^B always are (128-bit hashes at (16, 8))."""
    if not 1 <= max_bits <= 16:
        raise ValueError("sorted_column: max_bits must be 1 .. 16")
    if acc_cols < 1 or max_bits * acc_cols > 253:
        raise ValueError("sorted_column: acc_cols must be at least 1 and max_bits * acc_cols at most 253 (the limb sum must not wrap mod r)")
    cols = _Columns()
    ident = cols.advice()
    limbs = [cols.advice() for _ in range(acc_cols)]
    rng = cols.fixed()
    selector = cols.selector()
    cols.instance()
    for col in limbs:
        cols.enable_equality("advice", col)
    total: Expression = Advice(limbs[acc_cols - 1])
    for i in range(acc_cols - 1):
        total = total + Advice(limbs[i]) * Constant(1 << (max_bits * (acc_cols - 1 - i)))
    gates = [("next id is this id plus one plus the decomposed gap", [Fixed(selector) * (Advice(ident, 1) - Advice(ident) - Constant(1) - total)])]
    lookups = [([Advice(col)], [Fixed(rng)]) for col in limbs]
    return ConstraintSystem(f"SortedColumn<{max_bits}, {acc_cols}>", "this project's own (DESIGN.md section 32)",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, lookups, cols.equality,
                            unblinded_advice=(ident,), parameters=dict(max_bits=max_bits, acc_cols=acc_cols, sorted=True))


def range_check(value: Expression, range_: int) -> Expression:
    """chips/utils.rs:73-77: value * (1 - value) * (2 - value) * ... * (range - 1 - value), zero exactly on 0 .. range - 1."""
    acc = value
    for i in range(1, range_):
        acc = acc * (Constant(i) - value)
    return acc


def safe_accumulator(max_bits: int = 4, acc_cols: int = 4) -> ConstraintSystem:
    """SafeAccumulatorCircuit::configure, /root/reference/src/circuits/safe_accumulator.rs:21-50, with SafeACcumulatorChip::configure,
    /root/reference/src/chips/safe_accumulator.rs:36-173, IsZeroChip::configure, /root/reference/src/chips/is_zero.rs:26-55, and
    range_check / range_check_vec, /root/reference/src/chips/utils.rs:73-90 (TRANSCRIBED; the reference instantiates <4, 4> only).

    A running total of ``acc_cols`` limbs of ``max_bits`` bits.  Advice 0 is update_value, advice 1 left_most_inv, advice
    2 .. 1 + A the carries add_carries[0 .. A - 1], advice 2 + A .. 1 + 2 A the limbs accumulate[0 .. A - 1], most significant first;
    fixed 0, 1, 2 the selectors add, overflow, bool (the circuit's allocation order); one instance column.  Equality in the chip's
    order: the accumulate columns, the carry columns, the instance column.  Gates in creation order:
        "is_zero"                   s_over * acc[0] * (1 - acc[0] * inv)                                            is_zero.rs:34-49
        "bool constraint"           s_bool * c * (1 - c), one per carry column                                      safe_accumulator.rs:62-73
        "accumulation constraint"   the list of :153-161 in its order: the add-value polynomial (:112-117), the range check of the
                                    value (:118), the A - 1 limb-carry polynomials (:141-148), s_over * (1 - is_zero_expr)
                                    (:150-151), the range checks of the previous row's limbs (:158) and of this row's (:159)
    The accumulate columns are queried at Rotation::prev and Rotation::cur.  range_check(v, 2^b) is a product of 2^b linear factors,
    so the degree is 2^max_bits + 1 (17 at <4, 4>) and the extended domain is 2^max_bits times the domain."""
    if not 1 <= max_bits <= 4:
        raise ValueError("safe_accumulator: max_bits must be 1 .. 4 (the gate degree is 2^max_bits + 1)")
    if acc_cols < 2 or max_bits * acc_cols > 64:
        raise ValueError("safe_accumulator: acc_cols must be at least 2 and max_bits * acc_cols at most 64")
    cols = _Columns()
    value = cols.advice()                                                      # circuits/safe_accumulator.rs:22
    inv = cols.advice()                                                        # :23
    carries = [cols.advice() for _ in range(acc_cols)]                         # :24-29
    acc = [cols.advice() for _ in range(acc_cols)]                             # :30-35
    s_add, s_over, s_bool = cols.selector(), cols.selector(), cols.selector()  # :36-38
    inst = cols.instance()                                                     # :39
    A, one = Advice, Constant(1)
    is_zero_expr = one - A(acc[0]) * A(inv)                                    # is_zero.rs:47
    gates = [("is_zero", [Fixed(s_over) * A(acc[0]) * is_zero_expr])]          # chips/safe_accumulator.rs:49-54, is_zero.rs:48
    for col in acc:                                                            # :57
        cols.enable_equality("advice", col)
    for col in carries:                                                        # :58
        cols.enable_equality("advice", col)
    cols.enable_equality("instance", inst)                                     # :60
    gates.append(("bool constraint", [Fixed(s_bool) * A(c) * (one - A(c)) for c in carries]))                        # :62-73
    prev = [A(c, -1) for c in acc]                                             # :82-84
    carry = [A(c) for c in carries]                                            # :85-87
    cur = [A(c) for c in acc]                                                  # :88-90
    shift = Constant(1 << max_bits)                                            # :92
    last = acc_cols - 1
    polys = [Fixed(s_add) * ((A(value) + prev[last]) - (carry[last] * shift + cur[last]))]                           # :112-117
    polys.append(Fixed(s_add) * range_check(A(value), 1 << max_bits))                                                # :118
    polys += [Fixed(s_add) * ((cur[i] + carry[i] * shift) - (prev[i] + carry[i + 1])) for i in range(acc_cols - 1)]  # :141-148
    polys.append(Fixed(s_over) * (one - is_zero_expr))                                                               # :150-151
    polys += [Fixed(s_over) * range_check(e, 1 << max_bits) for e in prev]                                           # :158
    polys += [Fixed(s_over) * range_check(e, 1 << max_bits) for e in cur]                                            # :159
    gates.append(("accumulation constraint", polys))
    return ConstraintSystem(f"SafeAccumulator<{max_bits}, {acc_cols}>",
                            "circuits/safe_accumulator.rs:21-50, chips/safe_accumulator.rs:36-173, chips/is_zero.rs:26-55, chips/utils.rs:73-90",
                            cols.num_fixed, cols.num_advice, cols.num_instance, gates, [], cols.equality,
                            parameters=dict(max_bits=max_bits, acc_cols=acc_cols))


CONSTRAINT_SYSTEMS: Dict[str, Callable[[], ConstraintSystem]] = {
    "poseidon_k11": poseidon, "merkle_v3_k17": merkle_v3, "merkle_sum_tree_k18": merkle_sum_tree,
    # the reference's own shape of the range check: MockProver at k = 5 (/root/reference/src/circuits/overflow_check_v2.rs:66-90)
    "overflow_check_v2_k5": overflow_check_v2,
    # the ONE configuration the reference proves for real: test_full_prover, k = 9, a depth-5 path
    # (/root/reference/src/circuits/merkle_sum_tree.rs:345-358, path :172-212) -- the same constraint system as k = 18
    "merkle_sum_tree_k9": merkle_sum_tree,
}


@dataclass
class EvaluateHLayout:
    """Column table of the whole evaluate_h program: the circuit's fixed columns, then (as further fixed-kind entries) the
    permutation sigmas, the permutation z polynomials, l0 / l_last / l_active, the coset column zeta * omega_ext^idx, per
    lookup (z, permuted input, permuted table), and the short inverse-vanishing pattern; then advice; then instance."""
    num_fixed_entries: int
    sigma0: int
    z0: int
    l0: int
    l_last: int
    l_active: int
    x_coset: int
    lookup0: int
    t_inv: int
    short_columns: Dict[int, int] = field(default_factory=dict)


def evaluate_h_program(cs: ConstraintSystem, k: int, extended_k: int, delta: int, with_arguments: bool = True, per_coset: bool = False,
                       divide: bool = True, lookup: str = "halo2"):
    """GraphEvaluator for evaluate_h of `cs`: the custom gates, then (with_arguments) the permutation argument over the
    equality columns, every lookup argument, and divide_by_vanishing_poly as the last multiplication.
    per_coset: the program for ONE coset of the n-th roots inside the extended domain (EvaluationDomain.coeff_to_coset;
    compile with rot_scale = 1, evaluate over 2^k rows): 1 / (X^n - 1) is a single constant there and enters as Challenge(0)
    (compile with num_challenges = 1; the t_inv entry of the column table stays, unread).
    divide=False: the numerator only -- the division rides on the recombination (EvaluationDomain.combine_cosets(...,
    divide_by_vanishing=True)), so one launch can take several cosets as segments (CompiledGraph.evaluate(segments=...)).
    lookup="logup": every argument of ``cs.logup_arguments()`` in the place of the lookups, its table entries (phi, m) from
    ``lookup0`` on -- two per argument where a lookup has three.
    -> (GraphEvaluator, EvaluateHLayout)."""
    if lookup not in ("halo2", "logup"):
        raise ValueError(f"evaluate_h_program: lookup must be \"halo2\" or \"logup\", got {lookup!r}")
    nf = cs.num_fixed
    P, nsets, L = len(cs.equality), cs.permutation_sets(), len(cs.lookups)
    groups = cs.logup_arguments() if lookup == "logup" else []
    lay = EvaluateHLayout(num_fixed_entries=nf, sigma0=nf, z0=nf + P, l0=nf + P + nsets, l_last=nf + P + nsets + 1,
                          l_active=nf + P + nsets + 2, x_coset=nf + P + nsets + 3, lookup0=nf + P + nsets + 4,
                          t_inv=nf + P + nsets + 4 + (2 * len(groups) if lookup == "logup" else 3 * L))
    lay.num_fixed_entries = lay.t_inv + 1
    lay.short_columns = {lay.t_inv: extended_k - k}
    polys = list(cs.polynomials())
    if with_arguments:
        kind = {"advice": Advice, "fixed": Fixed, "instance": Instance}
        perm_cols = [kind[kd](i) for kd, i in cs.equality]
        polys += permutation_expressions(perm_cols, [Fixed(lay.sigma0 + j) for j in range(P)],
                                         [lambda r, i=i: Fixed(lay.z0 + i, r) for i in range(nsets)], Fixed(lay.l0), Fixed(lay.l_last),
                                         Fixed(lay.l_active), Fixed(lay.x_coset), cs.permutation_chunk_len(), delta,
                                         -(cs.blinding_factors + 1))
        for g, (tabs, ins_list) in enumerate(groups):
            b = lay.lookup0 + 2 * g
            polys += logup_expressions(ins_list, tabs, lambda r, b=b: Fixed(b, r), lambda r, b=b: Fixed(b + 1, r), Fixed(lay.l0),
                                       Fixed(lay.l_last), Fixed(lay.l_active))
        for j, (ins, tabs) in enumerate(cs.lookups if lookup == "halo2" else []):
            b = lay.lookup0 + 3 * j
            polys += lookup_expressions(ins, tabs, lambda r, b=b: Fixed(b, r), lambda r, b=b: Fixed(b + 1, r),
                                        lambda r, b=b: Fixed(b + 2, r), Fixed(lay.l0), Fixed(lay.l_last), Fixed(lay.l_active))
    g = GraphEvaluator()
    g.add_custom_gates(polys)
    if with_arguments and divide:
        g.add_vanishing_division(Challenge(0) if per_coset else Fixed(lay.t_inv))
    if per_coset:
        lay.short_columns = {}
    return g, lay
