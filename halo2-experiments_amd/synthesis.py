"""What ``MerkleSumTreeCircuit::synthesize`` decides, for ``circuits.merkle_sum_tree(spec)``: where every region lies, what the fixed
columns hold, which cells are copy-constrained, and the advice columns themselves -- on Python integers here (``assign_ints``, the
CPU twin) and on the GPU through the C ABI (``merkle_sum_witness``, csrc/poseidon.inc: one lane per (user, level), the Pow5 chip's
trace of every Poseidon round written straight into the columns).  The Pow5 chip's regions of one hash are stated once, in
``_Pow5Layout``, for this circuit and the two below.  DESIGN.md section 13.

TRANSCRIBED from the reference (read as text):
    "assign leaf hash", "assign leaf balance"        /root/reference/src/chips/merkle_sum_tree.rs:140-171
    "merkle prove layer" (two rows per level)        :182-286   bool + swap selectors on row 0, sum selector on row 1, swap by index :227-263
    the hash of [left_hash, left_balance, right_hash, right_balance]   :289-300, src/chips/poseidon/hash.rs:75-89
    "enforce sum to be less than total assets"       :317-352   a = the sum (copied), b = the assets (from instance row 3), c = check = 1
    expose_public rows 0, 1, 2; instance row 3       src/circuits/merkle_sum_tree.rs:50-55,96, chips/merkle_sum_tree.rs:329-335
RECALLED (the crates are git dependencies that are not at hand, as for the gates in circuits.py):
    halo2_gadgets Pow5Chip -- "initial state": one row, the WIDTH state words assigned from constants (0 .. 0, RATE * 2^64), i.e.
    copy-constrained to cells of rc_b[0], the ``enable_constant`` column; "pad-and-add": the initial state copied to row 0, the
    message copied to row 1 (s_pad_and_add there), their sum on row 2; "permute state": the sum copied to row 0, then one row per
    full round and one per PAIR of partial rounds (partial_sbox = the first S-box output of the pair; rc_a / rc_b = the round
    constants of the first / second round), and the final state on the last row, whose word 0 is the digest.
    LtChip::assign -- lt = lhs < rhs, diff = lhs - rhs + lt * 2^64 as 8 little-endian bytes; the u8 table in rows 0 .. 255.

Row placement: the regions follow one another in ``synthesize`` order, each starting at the first row that no earlier region uses;
the two regions that touch fixed columns only are placed by column: the u8 table in rows 0 .. 255 of its own column, the constants
in rc_b[0] after the last region.  Upstream's ``SimpleFloorPlanner`` packs every region per column and may start some earlier; that
cannot be pinned without the crate.  Every legal placement gives a valid circuit and the gates only use rotations inside a region,
so this is A valid layout of the reference's circuit, not a row-for-row copy of upstream's.

The two other circuits of the reference, with the same placement rule and the same Pow5 regions (``_Pow5Layout``):
``MerkleTreeV3Layout`` for ``circuits.merkle_v3(spec)`` (``merkle_witness``, one lane per (user, level)) and ``PoseidonCircuitLayout``
for ``circuits.poseidon(spec)`` (``poseidon_circuit_witness``, one lane per hash).  TRANSCRIBED (read as text):
    "assign leaf" (column a, row 0)                  /root/reference/src/chips/merkle_v3.rs:84-95
    "merkle prove layer" (two rows per level)        :97-148    bool + swap selectors on row 0; swapped whenever the index is not zero :126-130
    the hash of [left, right]                        :150-161
    expose_public rows 0 (leaf) and 1 (root)         :165-172, src/circuits/merkle_v3.rs:29-59
    "load private inputs" (hash_inputs[0 .. L), row 0)            src/chips/poseidon/hash_with_instance.rs:78-101
    "copy input cells to hash input cells" (copies of those)      :106-139
    the digest exposed at instance row 0             :141-148, src/circuits/poseidon.rs:43-59
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _ptr, _stream_ptr, _tensor_rows, _u32p
from .bn256 import FR_MODULUS, fr_array, fr_words
from .circuits import ConstraintSystem, merkle_sum_tree
from .poseidon import Spec, default_spec, ints_to_words

R = FR_MODULUS
Cell = Tuple[str, int, int]            # (kind, column, row)

# circuits.merkle_sum_tree()'s allocation order (MerkleSumTreeLayout's columns; the names tests and tools import)
A, B, C, D, E = range(5)
STATE = tuple(range(5, 10))
PARTIAL_SBOX, LT = 10, 11
DIFF = tuple(range(12, 20))
N_ADVICE = 20
BOOL_S, SWAP_S, SUM_S, LT_S = range(4)
RC_A = tuple(range(4, 9))
RC_B = tuple(range(9, 14))
S_FULL, S_PARTIAL, S_PAD, U8 = 14, 15, 16, 17
N_FIXED = 18
BLINDING_ROWS = 6                       # blinding_factors + 1: the rows create_proof keeps for itself


@dataclass
class Region:
    name: str
    start: int
    height: int
    columns: Tuple[Tuple[str, int], ...]

    @property
    def rows(self) -> range:
        return range(self.start, self.start + self.height)


class _Pow5Layout:
    """What the three layouts below share: the Pow5 chip's regions of one hash ("initial state" 1 row, "pad-and-add" 3, "permute
    state" perm_rows), their selectors, rc_a / rc_b rows, constants, copies and the assignment of the trace.  A subclass names its
    columns (WIDTH, STATE, PARTIAL_SBOX, RC_A, RC_B, S_FULL, S_PARTIAL, S_PAD, N_ADVICE, N_FIXED) and lists ``hash_start``: the
    "initial state" row of every hash; the constants of hash h lie in rc_b[0] at const_row + WIDTH * h."""
    NAME = ""
    WIDTH = 0
    STATE: Tuple[int, ...] = ()
    PARTIAL_SBOX = 0
    RC_A: Tuple[int, ...] = ()
    RC_B: Tuple[int, ...] = ()
    S_FULL = S_PARTIAL = S_PAD = 0
    N_ADVICE = N_FIXED = N_INSTANCE_ROWS = 0

    def _init_pow5(self, k: int, spec: Optional[Spec]) -> Spec:
        spec = default_spec(self.WIDTH) if spec is None else spec
        if spec.width != self.WIDTH:
            raise ValueError(f"{self.NAME}: needs a width-{self.WIDTH} spec")
        if spec.r_f % 2 or spec.r_p % 2:
            raise ValueError(f"{self.NAME}: the Pow5 chip needs even r_f and r_p")
        self.k, self.n, self.spec = k, 1 << k, spec
        self.perm_rows = spec.r_f + spec.r_p // 2 + 1
        self.hash_start: List[int] = []
        return spec

    def _place_hash(self, place, tag: str) -> None:
        adv = tuple(("advice", c) for c in self.STATE)
        self.hash_start.append(place(f"initial state{tag}", 1, adv).start)
        place(f"pad-and-add{tag}", 3, adv + (("fixed", self.S_PAD),))
        place(f"permute state{tag}", self.perm_rows, adv + (("advice", self.PARTIAL_SBOX),) +
              tuple(("fixed", c) for c in self.RC_A + self.RC_B + (self.S_FULL, self.S_PARTIAL)))

    def _finish(self, row: int, place, min_rows: int = 0) -> None:
        self.const_row = row
        place("constants", self.WIDTH * len(self.hash_start), (("fixed", self.RC_B[0]),))
        self.used_rows = max(self.const_row + self.WIDTH * len(self.hash_start), min_rows)
        if self.used_rows > self.n - BLINDING_ROWS:
            raise ValueError(f"{self.NAME}: {self.used_rows} rows are needed, 2^{self.k} - {BLINDING_ROWS} is fewer")

    # rows of hash h
    def init_row(self, h: int = 0) -> int:
        return self.hash_start[h]

    def pad_row(self, h: int = 0) -> int:
        return self.hash_start[h] + 1

    def perm_row(self, h: int = 0) -> int:
        return self.hash_start[h] + 4

    def digest_cell(self, h: int = 0) -> Cell:
        return ("advice", self.STATE[0], self.perm_row(h) + self.perm_rows - 1)

    def _round_of_row(self, i: int) -> int:
        """the (first) round that row i of "permute state" holds"""
        half, r_p = self.spec.r_f // 2, self.spec.r_p
        if i < half:
            return i
        if i < half + r_p // 2:
            return half + 2 * (i - half)
        return half + r_p + (i - half - r_p // 2)

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        if (cs.num_advice, cs.num_fixed, cs.num_instance) != (self.N_ADVICE, self.N_FIXED, 1):
            raise ValueError(f"{self.NAME}: the constraint system is not the circuit's")

    def _pow5_selector_rows(self, out: Dict[int, List[int]]) -> Dict[int, List[int]]:
        half, pairs = self.spec.r_f // 2, self.spec.r_p // 2
        for c in (self.S_FULL, self.S_PARTIAL, self.S_PAD):
            out[c] = []
        for h in range(len(self.hash_start)):
            out[self.S_PAD].append(self.pad_row(h) + 1)
            p = self.perm_row(h)
            out[self.S_FULL] += [p + i for i in range(half)] + [p + half + pairs + i for i in range(half)]
            out[self.S_PARTIAL] += [p + half + i for i in range(pairs)]
        return out

    def selector_rows(self) -> Dict[int, List[int]]:
        """fixed column of a selector -> the rows where it is enabled"""
        return self._pow5_selector_rows({})

    def fixed_columns(self) -> List[List[int]]:
        """The N_FIXED fixed columns as integers: selectors, rc_a / rc_b per "permute state" row, the constants."""
        rc, _, _ = self.spec.constants()
        half, pairs, W = self.spec.r_f // 2, self.spec.r_p // 2, self.WIDTH
        cols = [[0] * self.n for _ in range(self.N_FIXED)]
        for c, rows in self.selector_rows().items():
            for r in rows:
                cols[c][r] = 1
        for h in range(len(self.hash_start)):
            p = self.perm_row(h)
            for i in range(self.perm_rows - 1):
                rnd = self._round_of_row(i)
                for j in range(W):
                    cols[self.RC_A[j]][p + i] = rc[rnd][j]
                    if half <= i < half + pairs:
                        cols[self.RC_B[j]][p + i] = rc[rnd + 1][j]
            cols[self.RC_B[0]][self.const_row + W * h + W - 1] = self.spec.rate << 64
        return cols

    def _pow5_copies(self, h: int, message: Sequence[Cell]) -> List[Tuple[Cell, Cell]]:
        """constants -> initial state -> pad-and-add row 0; the message cells -> row 1; row 2 -> the first permute row"""
        ini, pad, perm, W = self.init_row(h), self.pad_row(h), self.perm_row(h), self.WIDTH
        out: List[Tuple[Cell, Cell]] = []
        for j in range(W):
            out.append((("fixed", self.RC_B[0], self.const_row + W * h + j), ("advice", self.STATE[j], ini)))     # assign_advice_from_constant
            out.append((("advice", self.STATE[j], ini), ("advice", self.STATE[j], pad)))
            out.append((("advice", self.STATE[j], pad + 2), ("advice", self.STATE[j], perm)))
        for j, cell in enumerate(message):
            out.append((cell, ("advice", self.STATE[j], pad + 1)))
        return out

    def _pow5_assign(self, adv: List[List[int]], h: int, msg: Sequence[int]) -> int:
        """the rows of hash h for the message ``msg`` (WIDTH - 1 integers) -> the digest"""
        rc, mds, _ = self.spec.constants()
        half, r_p, rounds, W = self.spec.r_f // 2, self.spec.r_p, self.spec.r_f + self.spec.r_p, self.WIDTH
        ini, pad, perm, cap = self.init_row(h), self.pad_row(h), self.perm_row(h), self.spec.rate << 64
        for j in range(W - 1):
            adv[self.STATE[j]][pad + 1] = adv[self.STATE[j]][pad + 2] = msg[j]
        adv[self.STATE[W - 1]][ini] = adv[self.STATE[W - 1]][pad] = adv[self.STATE[W - 1]][pad + 2] = cap
        s, row = list(msg) + [cap], 0
        for r in range(rounds):
            full = r < half or r >= half + r_p
            first = full or (r - half) % 2 == 0
            if first:
                for j in range(W):
                    adv[self.STATE[j]][perm + row] = s[j]
            x = [(v + c) % R for v, c in zip(s, rc[r])]
            x[0] = pow(x[0], 5, R)
            if first and not full:
                adv[self.PARTIAL_SBOX][perm + row] = x[0]
            row += first
            if full:
                x[1:] = [pow(v, 5, R) for v in x[1:]]
            s = [sum(m * v for m, v in zip(mrow, x)) % R for mrow in mds]
        for j in range(W):
            adv[self.STATE[j]][perm + row] = s[j]
        return s[0]


class MerkleSumTreeLayout(_Pow5Layout):
    """``MerkleSumTreeCircuit::synthesize`` for ``circuits.merkle_sum_tree(spec)``: a pure function of (depth, k, spec); see the
    module docstring for what is transcribed and what is recalled.  Rows 0, 1 the leaf; level l at 2 + l * level_rows: "merkle prove
    layer" (2 rows), then the hash's three regions; the less-than row; 5 constants per level at the end; the u8 table in rows 0 .. 255."""
    NAME = "MerkleSumTreeLayout"
    WIDTH = 5
    STATE, PARTIAL_SBOX, N_ADVICE = STATE, PARTIAL_SBOX, N_ADVICE
    RC_A, RC_B, S_FULL, S_PARTIAL, S_PAD, N_FIXED = RC_A, RC_B, S_FULL, S_PARTIAL, S_PAD, N_FIXED
    N_INSTANCE_ROWS = 4

    def __init__(self, depth: int, k: int, spec: Optional[Spec] = None):
        if not 1 <= depth <= 32:
            raise ValueError("MerkleSumTreeLayout: depth must be 1 .. 32")
        spec = self._init_pow5(k, spec)
        self.depth = depth
        adv = lambda *cols: tuple(("advice", c) for c in cols)
        regions: List[Region] = [Region("load u8 range check table", 0, 256, (("fixed", U8),))]
        row = 0

        def place(name: str, height: int, columns) -> Region:
            nonlocal row
            regions.append(Region(name, row, height, tuple(columns)))
            row += height
            return regions[-1]

        place("assign leaf hash", 1, adv(A))
        place("assign leaf balance", 1, adv(B))
        self.level_start: List[int] = []
        for l in range(depth):
            self.level_start.append(row)
            place(f"merkle prove layer {l}", 2, adv(A, B, C, D, E) + (("fixed", BOOL_S), ("fixed", SWAP_S), ("fixed", SUM_S)))
            self._place_hash(place, f" {l}")
        self.level_rows = 6 + self.perm_rows
        self.lt_row = row
        place("enforce sum to be less than total assets", 1, adv(A, B, C, LT, *DIFF) + (("fixed", LT_S),))
        self.regions = regions
        try:
            self._finish(row, place, min_rows=256)
        except ValueError as e:
            raise ValueError(f"{e} (depth {depth}: min_k = {self.min_k(depth, spec)})") from None

    @staticmethod
    def rows_needed(depth: int, spec: Optional[Spec] = None) -> int:
        spec = default_spec(5) if spec is None else spec
        return max(2 + depth * (6 + spec.r_f + spec.r_p // 2 + 1) + 1 + 5 * depth, 256)

    @classmethod
    def min_k(cls, depth: int, spec: Optional[Spec] = None) -> int:
        return (cls.rows_needed(depth, spec) + BLINDING_ROWS - 1).bit_length()

    def prove_row(self, l: int) -> int:
        return self.level_start[l]

    def sum_cell(self, l: int) -> Cell:
        return ("advice", E, self.prove_row(l) + 1)

    def selector_rows(self) -> Dict[int, List[int]]:
        out = {BOOL_S: [self.prove_row(l) for l in range(self.depth)], SWAP_S: [self.prove_row(l) for l in range(self.depth)],
               SUM_S: [self.prove_row(l) + 1 for l in range(self.depth)], LT_S: [self.lt_row]}
        return self._pow5_selector_rows(out)

    def fixed_columns(self) -> List[List[int]]:
        """The N_FIXED fixed columns as integers: what every Pow5 layout has, and the u8 table."""
        cols = super().fixed_columns()
        cols[U8][:256] = range(256)
        return cols

    def copies(self) -> List[Tuple[Cell, Cell]]:
        out: List[Tuple[Cell, Cell]] = [(("advice", A, 0), ("instance", 0, 0)), (("advice", B, 1), ("instance", 0, 1))]   # expose_public 0, 1
        prev_hash, prev_balance = ("advice", A, 0), ("advice", B, 1)
        for l in range(self.depth):
            pr = self.prove_row(l)
            out += [(prev_hash, ("advice", A, pr)), (prev_balance, ("advice", B, pr))]
            out += self._pow5_copies(l, [("advice", j, pr + 1) for j in range(4)])
            prev_hash, prev_balance = self.digest_cell(l), self.sum_cell(l)
        out += [(prev_balance, ("advice", A, self.lt_row)), (("instance", 0, 3), ("advice", B, self.lt_row)),
                (prev_hash, ("instance", 0, 2))]
        return out

    def instance(self, leaf: Tuple[int, int], root: int, assets: int) -> List[List[int]]:
        col = [0] * self.n
        col[0], col[1], col[2], col[3] = int(leaf[0]) % R, int(leaf[1]) % R, int(root) % R, int(assets) % R
        return [col]

    def assign_ints(self, leaf: Tuple[int, int], siblings: Sequence[Tuple[int, int]], indices: Sequence[int], assets_sum: int) -> List[List[int]]:
        """The N_ADVICE advice columns as the chip assigns them.  Nothing is judged: an index of 2 or a sum above the assets
        gives an unsatisfied witness, as in the reference's negative tests."""
        if len(siblings) != self.depth or len(indices) != self.depth:
            raise ValueError("assign_ints: the path must have `depth` siblings and indices")
        adv = [[0] * self.n for _ in range(N_ADVICE)]
        h, b = int(leaf[0]) % R, int(leaf[1]) % R
        adv[A][0], adv[B][1] = h, b
        total = b
        for l, ((eh, eb), index) in enumerate(zip(siblings, indices)):
            eh, eb, index, pr = int(eh) % R, int(eb) % R, int(index) % R, self.prove_row(l)
            adv[A][pr], adv[B][pr], adv[C][pr], adv[D][pr], adv[E][pr] = h, b, eh, eb, index
            msg = [h, b, eh, eb] if index == 0 else [eh, eb, h, b]                         # :227-234
            for j in range(4):
                adv[j][pr + 1] = msg[j]
            adv[E][pr + 1] = b = (msg[1] + msg[3]) % R
            h = self._pow5_assign(adv, l, msg)
            total = (total + eb) % R
        assets = int(assets_sum) % R
        lt = int(total < assets)
        diff = (total - assets + (lt << 64)) % R
        adv[A][self.lt_row], adv[B][self.lt_row], adv[C][self.lt_row], adv[LT][self.lt_row] = b, assets, 1, lt
        for i, byte in enumerate(diff.to_bytes(32, "little")[:8]):
            adv[DIFF[i]][self.lt_row] = byte
        return adv


class MerkleTreeV3Layout(_Pow5Layout):
    """``MerkleTreeV3Circuit::synthesize`` for ``circuits.merkle_v3(spec)``: a pure function of (depth, k, spec).  Row 0 the leaf;
    level l at 1 + l * level_rows: "merkle prove layer" (2 rows), then the hash's three regions; 3 constants per level at the end."""
    NAME = "MerkleTreeV3Layout"
    WIDTH = 3
    A, B, C = range(3)                      # circuits.merkle_v3()'s allocation order (asserted in check_constraint_system)
    STATE = (3, 4, 5)
    PARTIAL_SBOX = 6
    N_ADVICE = 7
    BOOL_S, SWAP_S = 0, 1
    RC_A = (2, 3, 4)
    RC_B = (5, 6, 7)
    S_FULL, S_PARTIAL, S_PAD = 8, 9, 10
    N_FIXED = 11
    N_INSTANCE_ROWS = 2

    def __init__(self, depth: int, k: int, spec: Optional[Spec] = None):
        if not 1 <= depth <= 32:
            raise ValueError("MerkleTreeV3Layout: depth must be 1 .. 32")
        spec = self._init_pow5(k, spec)
        self.depth = depth
        adv = lambda *cols: tuple(("advice", c) for c in cols)
        regions: List[Region] = []
        row = 0

        def place(name: str, height: int, columns) -> Region:
            nonlocal row
            regions.append(Region(name, row, height, tuple(columns)))
            row += height
            return regions[-1]

        place("assign leaf", 1, adv(self.A))
        self.level_start: List[int] = []
        for l in range(depth):
            self.level_start.append(row)
            place(f"merkle prove layer {l}", 2, adv(self.A, self.B, self.C) + (("fixed", self.BOOL_S), ("fixed", self.SWAP_S)))
            self._place_hash(place, f" {l}")
        self.level_rows = 6 + self.perm_rows
        self.regions = regions
        try:
            self._finish(row, place)
        except ValueError as e:
            raise ValueError(f"{e} (depth {depth}: min_k = {self.min_k(depth, spec)})") from None

    @staticmethod
    def rows_needed(depth: int, spec: Optional[Spec] = None) -> int:
        spec = default_spec(3) if spec is None else spec
        return 1 + depth * (6 + spec.r_f + spec.r_p // 2 + 1) + 3 * depth

    @classmethod
    def min_k(cls, depth: int, spec: Optional[Spec] = None) -> int:
        return (cls.rows_needed(depth, spec) + BLINDING_ROWS - 1).bit_length()

    def prove_row(self, l: int) -> int:
        return self.level_start[l]

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        super().check_constraint_system(cs)
        want = [("advice", c) for c in (self.A, self.B, self.C)] + [("instance", 0)] + [("advice", c) for c in self.STATE] + [("fixed", self.RC_B[0])]
        if list(cs.equality) != want:
            raise ValueError("MerkleTreeV3Layout: the constraint system is not circuits.merkle_v3()")

    def selector_rows(self) -> Dict[int, List[int]]:
        out = {self.BOOL_S: [self.prove_row(l) for l in range(self.depth)], self.SWAP_S: [self.prove_row(l) for l in range(self.depth)]}
        return self._pow5_selector_rows(out)

    def copies(self) -> List[Tuple[Cell, Cell]]:
        out: List[Tuple[Cell, Cell]] = [(("advice", self.A, 0), ("instance", 0, 0))]                    # expose_public 0
        prev: Cell = ("advice", self.A, 0)
        for l in range(self.depth):
            pr = self.prove_row(l)
            out.append((prev, ("advice", self.A, pr)))
            out += self._pow5_copies(l, [("advice", self.A, pr + 1), ("advice", self.B, pr + 1)])
            prev = self.digest_cell(l)
        out.append((prev, ("instance", 0, 1)))                                                         # expose_public 1
        return out

    def instance(self, leaf: int, root: int) -> List[List[int]]:
        col = [0] * self.n
        col[0], col[1] = int(leaf) % R, int(root) % R
        return [col]

    def assign_ints(self, leaf: int, siblings: Sequence[int], indices: Sequence[int]) -> List[List[int]]:
        """The N_ADVICE advice columns as the chip assigns them.  Nothing is judged: an index of 2 gives an unsatisfied witness
        (the pair is swapped whenever the index is not zero, merkle_v3.rs:126-130)."""
        if len(siblings) != self.depth or len(indices) != self.depth:
            raise ValueError("assign_ints: the path must have `depth` siblings and indices")
        adv = [[0] * self.n for _ in range(self.N_ADVICE)]
        h = int(leaf) % R
        adv[self.A][0] = h
        for l, (e, index) in enumerate(zip(siblings, indices)):
            e, index, pr = int(e) % R, int(index) % R, self.prove_row(l)
            adv[self.A][pr], adv[self.B][pr], adv[self.C][pr] = h, e, index
            msg = [h, e] if index == 0 else [e, h]
            adv[self.A][pr + 1], adv[self.B][pr + 1] = msg
            h = self._pow5_assign(adv, l, msg)
        return adv


class PoseidonCircuitLayout(_Pow5Layout):
    """``PoseidonCircuit::synthesize`` for ``circuits.poseidon(spec)`` (WIDTH 5, L = 4): row 0 "load private inputs", row 1 "copy
    input cells to hash input cells", then the hash's three regions and 5 constants; the digest is instance row 0."""
    NAME = "PoseidonCircuitLayout"
    WIDTH = 5
    STATE = (0, 1, 2, 3, 4)                 # circuits.poseidon()'s allocation order (asserted in check_constraint_system)
    PARTIAL_SBOX = 5
    N_ADVICE = 6
    RC_A = (0, 1, 2, 3, 4)
    RC_B = (5, 6, 7, 8, 9)
    S_FULL, S_PARTIAL, S_PAD = 10, 11, 12
    N_FIXED = 13
    N_INSTANCE_ROWS = 1
    LOAD_ROW, COPY_ROW = 0, 1

    def __init__(self, k: int, spec: Optional[Spec] = None):
        spec = self._init_pow5(k, spec)
        regions: List[Region] = []
        row = 0

        def place(name: str, height: int, columns) -> Region:
            nonlocal row
            regions.append(Region(name, row, height, tuple(columns)))
            row += height
            return regions[-1]

        inputs = tuple(("advice", c) for c in self.STATE[:4])
        place("load private inputs", 1, inputs)
        place("copy input cells to hash input cells", 1, inputs)
        self._place_hash(place, "")
        self.level_rows = row
        self.regions = regions
        try:
            self._finish(row, place)
        except ValueError as e:
            raise ValueError(f"{e} (min_k = {self.min_k(spec)})") from None

    @staticmethod
    def rows_needed(spec: Optional[Spec] = None) -> int:
        spec = default_spec(5) if spec is None else spec
        return 2 + 4 + spec.r_f + spec.r_p // 2 + 1 + 5

    @classmethod
    def min_k(cls, spec: Optional[Spec] = None) -> int:
        return (cls.rows_needed(spec) + BLINDING_ROWS - 1).bit_length()

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        super().check_constraint_system(cs)
        if list(cs.equality) != [("advice", c) for c in self.STATE] + [("fixed", self.RC_B[0]), ("instance", 0)]:
            raise ValueError("PoseidonCircuitLayout: the constraint system is not circuits.poseidon()")

    def copies(self) -> List[Tuple[Cell, Cell]]:
        out: List[Tuple[Cell, Cell]] = [(("advice", c, self.LOAD_ROW), ("advice", c, self.COPY_ROW)) for c in self.STATE[:4]]
        out += self._pow5_copies(0, [("advice", c, self.COPY_ROW) for c in self.STATE[:4]])
        out.append((self.digest_cell(0), ("instance", 0, 0)))
        return out

    def instance(self, digest: int) -> List[List[int]]:
        col = [0] * self.n
        col[0] = int(digest) % R
        return [col]

    def assign_ints(self, message: Sequence[int]) -> List[List[int]]:
        if len(message) != 4:
            raise ValueError("assign_ints: the message must have 4 elements")
        msg = [int(v) % R for v in message]
        adv = [[0] * self.n for _ in range(self.N_ADVICE)]
        for j in range(4):
            adv[self.STATE[j]][self.LOAD_ROW] = adv[self.STATE[j]][self.COPY_ROW] = msg[j]
        self._pow5_assign(adv, 0, msg)
        return adv


class RangeCheckLayout:
    """``OverflowCheckCircuitV2::synthesize`` for ``circuits.overflow_check_v2(max_bits, acc_cols)``, with ``rows`` values instead of
    the reference's three.  TRANSCRIBED (read as text):
        chip.load: the range table, fixed column ``range`` rows 0 .. 2^max_bits - 1     /root/reference/src/chips/overflow_check_v2.rs:116-133
        chip.assign: one region of one row per value -- selector, value, limbs          :80-114, src/circuits/overflow_check_v2.rs:41-59
    The regions follow one another from row 0: value i on row i, the selector on rows 0 .. rows - 1.  There are no copies and the
    instance column is empty.  The rest of ``range`` is zero, which is a legal table entry, and so are the limbs of the unused rows.

    One deviation from the reference: it calls ``decompose_bigInt_to_ubits(value, MAX_BITS, ACC_COLS)`` against the signature
    (value, number_of_limbs, bit_len) (chips/utils.rs) -- the two arguments swapped, harmless at its only instantiation <4, 4>.  Here
    the decomposition is what the gate needs: ``acc_cols`` limbs of ``max_bits`` bits each."""
    NAME = "RangeCheckLayout"
    VALUE, RANGE, SELECTOR = 0, 0, 1          # advice 0; fixed 0, 1 (circuits.overflow_check_v2()'s allocation order)
    N_FIXED = 2

    def __init__(self, k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1):
        if not 1 <= max_bits <= 16:
            raise ValueError("RangeCheckLayout: max_bits must be 1 .. 16")
        if acc_cols < 1 or max_bits * acc_cols > 253:
            raise ValueError("RangeCheckLayout: acc_cols must be at least 1 and max_bits * acc_cols at most 253")
        if rows < 1:
            raise ValueError("RangeCheckLayout: rows must be at least 1")
        self.k, self.n, self.max_bits, self.acc_cols, self.rows = k, 1 << k, max_bits, acc_cols, rows
        self.N_ADVICE = 1 + acc_cols
        self.LIMBS = tuple(range(1, 1 + acc_cols))
        self.table_rows = 1 << max_bits
        self.used_rows = self.rows_needed(max_bits, rows)
        if self.used_rows > self.n - BLINDING_ROWS:
            raise ValueError(f"RangeCheckLayout: {self.used_rows} rows are needed, 2^{k} - {BLINDING_ROWS} is fewer "
                             f"(min_k = {self.min_k(max_bits, rows)})")
        cols = (("advice", self.VALUE),) + tuple(("advice", c) for c in self.LIMBS) + (("fixed", self.SELECTOR),)
        self.regions = [Region(f"load range check table of {max_bits} bits", 0, self.table_rows, (("fixed", self.RANGE),))]
        self.regions += [Region("assign decomposed values", i, 1, cols) for i in range(rows)]

    @staticmethod
    def rows_needed(max_bits: int, rows: int) -> int:
        return max(rows, 1 << max_bits)

    @classmethod
    def min_k(cls, max_bits: int, rows: int) -> int:
        return (cls.rows_needed(max_bits, rows) + BLINDING_ROWS - 1).bit_length()

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        if (cs.num_advice, cs.num_fixed, cs.num_instance) != (self.N_ADVICE, self.N_FIXED, 1) or \
                list(cs.equality) != [("advice", c) for c in self.LIMBS] or len(cs.lookups) != self.acc_cols:
            raise ValueError(f"RangeCheckLayout: the constraint system is not circuits.overflow_check_v2(max_bits, {self.acc_cols})")

    def selector_rows(self) -> Dict[int, List[int]]:
        return {self.SELECTOR: list(range(self.rows))}

    def fixed_columns(self) -> List[List[int]]:
        cols = [[0] * self.n for _ in range(self.N_FIXED)]
        cols[self.RANGE][:self.table_rows] = range(self.table_rows)
        cols[self.SELECTOR][:self.rows] = [1] * self.rows
        return cols

    def copies(self) -> List[Tuple[Cell, Cell]]:
        return []

    def instance(self) -> List[List[int]]:
        return [[]]

    def assign_ints(self, values: Sequence[int]) -> List[List[int]]:
        """The 1 + acc_cols advice columns as the chip assigns them.  Nothing is judged: the limbs are the low max_bits * acc_cols
        bits of the value, so a value at or above 2^(max_bits * acc_cols) gives a witness that fails the gate."""
        if len(values) != self.rows:
            raise ValueError(f"assign_ints: {self.rows} values expected")
        adv = [[0] * self.n for _ in range(self.N_ADVICE)]
        mask = (1 << self.max_bits) - 1
        for row, v in enumerate(values):
            v = int(v) % R
            adv[self.VALUE][row] = v
            for i, c in enumerate(self.LIMBS):
                adv[c][row] = (v >> (self.max_bits * (self.acc_cols - 1 - i))) & mask
        return adv


class SortedColumnLayout:
    """The rows of ``circuits.sorted_column(max_bits, acc_cols)`` for an id column with ``rows`` live rows; the
    project's own, modelled on ``RangeCheckLayout``.  The range table on rows 0 .. 2^max_bits - 1 of fixed 0; id i on row i, with the
    limbs of the gap to id i + 1 beside it and the selector set, for i = 0 .. rows - 2; row rows - 1 holds the last id alone (no
    selector: it has no next id, and the gate must not reach the zero padding).  No copies, an empty instance column.

    With B = max_bits * acc_cols the gate gives id[i] = id[0] + s_i mod r for integers 0 = s_0 < s_1 < .. < s_(rows-1) <
    2^(k + B); the layout refuses B + k > 253, under which those sums stay below r and the ids are pairwise distinct whatever id[0]
    is (the argument in full: ``circuits.sorted_column``)."""
    NAME = "SortedColumnLayout"
    ID, RANGE, SELECTOR = 0, 0, 1             # advice 0; fixed 0, 1 (circuits.sorted_column()'s allocation order)
    N_FIXED = 2

    def __init__(self, k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1):
        if not 1 <= max_bits <= 16:
            raise ValueError("SortedColumnLayout: max_bits must be 1 .. 16")
        if acc_cols < 1 or max_bits * acc_cols > 253:
            raise ValueError("SortedColumnLayout: acc_cols must be at least 1 and max_bits * acc_cols at most 253")
        if max_bits * acc_cols + k > 253:
            raise ValueError(f"SortedColumnLayout: max_bits * acc_cols + k = {max_bits * acc_cols + k} exceeds 253: the sum of up to 2^k "
                             "gaps of max_bits * acc_cols bits could reach r, and two ids could then agree mod r")
        if rows < 1:
            raise ValueError("SortedColumnLayout: rows must be at least 1")
        self.k, self.n, self.max_bits, self.acc_cols, self.rows = k, 1 << k, max_bits, acc_cols, rows
        self.width = max_bits * acc_cols
        self.N_ADVICE = 1 + acc_cols
        self.LIMBS = tuple(range(1, 1 + acc_cols))
        self.table_rows = 1 << max_bits
        self.used_rows = self.rows_needed(max_bits, rows)
        if self.used_rows > self.n - BLINDING_ROWS:
            raise ValueError(f"SortedColumnLayout: {self.used_rows} rows are needed, 2^{k} - {BLINDING_ROWS} is fewer "
                             f"(min_k = {self.min_k(max_bits, rows)})")
        cols = (("advice", self.ID),) + tuple(("advice", c) for c in self.LIMBS) + (("fixed", self.SELECTOR),)
        self.regions = [Region(f"load range check table of {max_bits} bits", 0, self.table_rows, (("fixed", self.RANGE),))]
        self.regions += [Region("assign id and decomposed gap", i, 1, cols) for i in range(rows - 1)]
        self.regions += [Region("assign last id", rows - 1, 1, (("advice", self.ID),))]

    @staticmethod
    def rows_needed(max_bits: int, rows: int) -> int:
        return max(rows, 1 << max_bits)

    @classmethod
    def min_k(cls, max_bits: int, rows: int) -> int:
        return (cls.rows_needed(max_bits, rows) + BLINDING_ROWS - 1).bit_length()

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        if (cs.num_advice, cs.num_fixed, cs.num_instance) != (self.N_ADVICE, self.N_FIXED, 1) or \
                list(cs.equality) != [("advice", c) for c in self.LIMBS] or len(cs.lookups) != self.acc_cols or \
                cs.parameters != dict(max_bits=self.max_bits, acc_cols=self.acc_cols, sorted=True):
            raise ValueError(f"SortedColumnLayout: the constraint system is not circuits.sorted_column({self.max_bits}, {self.acc_cols})")

    def selector_rows(self) -> Dict[int, List[int]]:
        return {self.SELECTOR: list(range(self.rows - 1))}

    def fixed_columns(self) -> List[List[int]]:
        cols = [[0] * self.n for _ in range(self.N_FIXED)]
        cols[self.RANGE][:self.table_rows] = range(self.table_rows)
        cols[self.SELECTOR][:self.rows - 1] = [1] * (self.rows - 1)
        return cols

    def copies(self) -> List[Tuple[Cell, Cell]]:
        return []

    def instance(self) -> List[List[int]]:
        return [[]]

    def gaps(self, ids: Sequence[int]) -> List[int]:
        """(id[i+1] - id[i] - 1) mod r for i = 0 .. rows - 2"""
        if len(ids) != self.rows:
            raise ValueError(f"SortedColumnLayout: {self.rows} ids expected")
        v = [int(x) % R for x in ids]
        return [(v[i + 1] - v[i] - 1) % R for i in range(self.rows - 1)]

    def assign_ints(self, ids: Sequence[int]) -> List[List[int]]:
        """The 1 + acc_cols advice columns.  Nothing is judged: the limbs are the low max_bits * acc_cols bits of the gap mod r, so ids
        that are not ascending, equal, or further apart than 2^(max_bits * acc_cols) give a witness that fails the gate.  The limbs of
        row rows - 1 and of every row behind it are zero."""
        gaps = self.gaps(ids)
        adv = [[0] * self.n for _ in range(self.N_ADVICE)]
        mask = (1 << self.max_bits) - 1
        for row, v in enumerate(ids):
            adv[self.ID][row] = int(v) % R
        for row, g in enumerate(gaps):
            for i, c in enumerate(self.LIMBS):
                adv[c][row] = (g >> (self.max_bits * (self.acc_cols - 1 - i))) & mask
        return adv

    def over(self, ids: Sequence[int]) -> int:
        """what the GPU witness counts: the rows i <= rows - 2 whose gap has a bit at or above max_bits * acc_cols -- unsorted,
        duplicate and too distant ids alike"""
        return sum(g >> self.width != 0 for g in self.gaps(ids))


class SafeAccumulatorLayout:
    """``SafeAccumulatorCircuit::synthesize`` for ``circuits.safe_accumulator(max_bits, acc_cols)`` with ``rows`` added values, as
    ONE running table -- the table the reference's README draws and its gate at ``Rotation::prev`` is written
    for.  TRANSCRIBED (read as text):
        chip.assign: value, previous limbs, carries, inverse, updated limbs         /root/reference/src/chips/safe_accumulator.rs:175-260
        the loop over the values and expose_public                                  /root/reference/src/circuits/safe_accumulator.rs:52-90
        is_zero_chip.assign: the inverse, or 0                                      /root/reference/src/chips/is_zero.rs:57-66
    Row 0 holds the initial accumulate limbs and nothing else; row r, 1 <= r <= rows, holds value r, the inverse of the top limb,
    the carries and the limbs after adding value r.  All three selectors are set on rows 1 .. rows.  There are ``acc_cols`` copies:
    accumulate column i on row ``rows`` to instance row i (instance row 0 is the most significant limb).  rows + 1 <= 2^k - 6.

    Two deviations from the reference:
      * it opens a new two-row region per value and assigns the previous limbs into it again without a copy constraint, and its
        ``offset`` arithmetic breaks from the third value on (circuits/safe_accumulator.rs:72-82, chips/safe_accumulator.rs:190-251:
        the value and the inverse go to row 1, the carries and limbs to row offset + 1).  For one value the running table is the
        reference's region cell for cell; for more it is one table whose row r - 1 IS the previous state of row r.
      * its config keeps only two of its three selectors and never enables ``bool_selector`` (chips/safe_accumulator.rs:170,
        :190-191), so the carries are not constrained to be bits and the accumulator is unsound (any field
        element that balances the limb polynomials passes as a carry).  Here the bool selector is set on every accumulating row, as the
        reference's README says it is meant to be."""
    NAME = "SafeAccumulatorLayout"
    VALUE, INV = 0, 1                         # advice 0, 1 (circuits.safe_accumulator()'s allocation order)
    S_ADD, S_OVER, S_BOOL = 0, 1, 2           # fixed 0 .. 2
    N_FIXED = 3

    def __init__(self, k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1):
        if not 1 <= max_bits <= 4:
            raise ValueError("SafeAccumulatorLayout: max_bits must be 1 .. 4")
        if acc_cols < 2 or max_bits * acc_cols > 64:
            raise ValueError("SafeAccumulatorLayout: acc_cols must be at least 2 and max_bits * acc_cols at most 64")
        if rows < 1:
            raise ValueError("SafeAccumulatorLayout: rows must be at least 1")
        self.k, self.n, self.max_bits, self.acc_cols, self.rows = k, 1 << k, max_bits, acc_cols, rows
        self.N_ADVICE = 2 + 2 * acc_cols
        self.CARRIES = tuple(range(2, 2 + acc_cols))
        self.ACC = tuple(range(2 + acc_cols, 2 + 2 * acc_cols))
        self.width = max_bits * acc_cols
        self.used_rows = self.rows_needed(rows)
        if self.used_rows > self.n - BLINDING_ROWS:
            raise ValueError(f"SafeAccumulatorLayout: {self.used_rows} rows are needed, 2^{k} - {BLINDING_ROWS} is fewer "
                             f"(min_k = {self.min_k(rows)})")
        cols = tuple(("advice", c) for c in range(self.N_ADVICE)) + tuple(("fixed", c) for c in range(self.N_FIXED))
        self.regions = [Region("calculate accumulates", 0, self.used_rows, cols)]

    @staticmethod
    def rows_needed(rows: int) -> int:
        return rows + 1

    @classmethod
    def min_k(cls, rows: int) -> int:
        return (cls.rows_needed(rows) + BLINDING_ROWS - 1).bit_length()

    def check_constraint_system(self, cs: ConstraintSystem) -> None:
        equality = [("advice", c) for c in self.ACC + self.CARRIES] + [("instance", 0)]
        if (cs.num_advice, cs.num_fixed, cs.num_instance) != (self.N_ADVICE, self.N_FIXED, 1) or list(cs.equality) != equality or \
                cs.parameters != dict(max_bits=self.max_bits, acc_cols=self.acc_cols):
            raise ValueError(f"SafeAccumulatorLayout: the constraint system is not circuits.safe_accumulator({self.max_bits}, {self.acc_cols})")

    def selector_rows(self) -> Dict[int, List[int]]:
        return {s: list(range(1, self.rows + 1)) for s in (self.S_ADD, self.S_OVER, self.S_BOOL)}

    def fixed_columns(self) -> List[List[int]]:
        cols = [[0] * self.n for _ in range(self.N_FIXED)]
        for s, rows in self.selector_rows().items():
            for r in rows:
                cols[s][r] = 1
        return cols

    def copies(self) -> List[Tuple[Cell, Cell]]:
        return [(("advice", c, self.rows), ("instance", 0, i)) for i, c in enumerate(self.ACC)]

    def state(self, initial: Sequence[int]) -> int:
        """the initial limbs read as one integer below 2^(max_bits * acc_cols)"""
        if len(initial) != self.acc_cols:
            raise ValueError(f"SafeAccumulatorLayout: {self.acc_cols} initial limbs expected")
        s = 0
        for limb in initial:
            s = (s << self.max_bits) + int(limb)
        return s % (1 << self.width)

    def limbs(self, s: int) -> List[int]:
        mask = (1 << self.max_bits) - 1
        return [(s >> (self.max_bits * (self.acc_cols - 1 - i))) & mask for i in range(self.acc_cols)]

    def finals(self, initial: Sequence[int], values: Sequence[int]) -> List[int]:
        """the limbs after the last value"""
        s = self.state(initial)
        for v in values:
            s = (s + int(v) % R) % (1 << self.width)
        return self.limbs(s)

    def instance(self, initial: Sequence[int], values: Sequence[int]) -> List[List[int]]:
        return [self.finals(initial, values)]

    def assign_ints(self, initial: Sequence[int], values: Sequence[int]) -> List[List[int]]:
        """The 2 + 2 acc_cols advice columns -- the definition of the witness.  Nothing is judged: with b = max_bits, A = acc_cols and
        W = b A, S_0 is the initial limbs read as one integer mod 2^W, v_r the value's plain integer mod 2^W, S_r = (S_(r-1) + v_r) mod
        2^W; the limbs of row r are those of S_r; c[A-1] = (prev[A-1] + v_r >= 2^b), c[i] = (prev[i] + c[i+1] >= 2^b) for
        1 <= i < A - 1, c[0] = 0 (the reference's ``idx > 0``); inv is the inverse of the top limb mod r, or 0; the value column holds
        the value as given, and row 0 the initial limbs as given.  The witness satisfies the system exactly when every value and every
        initial limb is below 2^b and the top limb is 0 on every row 0 .. rows: the usable capacity is b (A - 1) bits."""
        if len(values) != self.rows:
            raise ValueError(f"assign_ints: {self.rows} values expected")
        b, A = self.max_bits, self.acc_cols
        adv = [[0] * self.n for _ in range(self.N_ADVICE)]
        s = self.state(initial)
        for i, c in enumerate(self.ACC):
            adv[c][0] = int(initial[i]) % R
        for r, value in enumerate(values, start=1):
            value = int(value) % R
            v = value % (1 << self.width)
            prev = self.limbs(s)
            s = (s + v) % (1 << self.width)
            cur = self.limbs(s)
            carry = [0] * A
            carry[A - 1] = int(prev[A - 1] + v >= 1 << b)
            for i in range(A - 2, 0, -1):
                carry[i] = int(prev[i] + carry[i + 1] >= 1 << b)
            adv[self.VALUE][r] = value
            adv[self.INV][r] = pow(cur[0], R - 2, R) if cur[0] else 0
            for i in range(A):
                adv[self.CARRIES[i]][r] = carry[i]
                adv[self.ACC[i]][r] = cur[i]
        return adv

    def over(self, initial: Sequence[int], values: Sequence[int]) -> int:
        """what the GPU witness counts: the rows whose value is at or above 2^b or whose top limb is not zero, plus 1 when an initial
        limb is at or above 2^b or the initial top limb is not zero"""
        s = self.state(initial)
        count = int(any(int(x) >> self.max_bits for x in initial) or int(initial[0]) != 0)
        for v in values:
            v = int(v) % R
            s = (s + v) % (1 << self.width)
            count += int(v >> self.max_bits != 0 or self.limbs(s)[0] != 0)
        return count


# ---- keygen's permutation columns -----------------------------------------------------------------------------------------------
AnyLayout = Union[MerkleSumTreeLayout, MerkleTreeV3Layout, PoseidonCircuitLayout, RangeCheckLayout, SortedColumnLayout, SafeAccumulatorLayout]      # anything with ``n`` and ``copies()``


def permutation_cells(cs: ConstraintSystem, layout: "AnyLayout") -> List[List[Tuple[int, int]]]:
    """``permutation::keygen::Assembly``: sigma as cells -- out[j][i] = (j', i') for column j of ``cs.equality`` and row i; the
    identity outside the copy cycles, every cycle rotated by one."""
    index = {col: j for j, col in enumerate(cs.equality)}
    n = layout.n
    parent: Dict[Tuple[int, int], Tuple[int, int]] = {}

    def find(c):
        while parent.setdefault(c, c) != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for (ka, ca, ra), (kb, cb, rb) in layout.copies():
        if (ka, ca) not in index or (kb, cb) not in index:
            raise ValueError(f"permutation_cells: a copy touches a column without equality: {(ka, ca)} / {(kb, cb)}")
        a, b = find((index[(ka, ca)], ra)), find((index[(kb, cb)], rb))
        if a != b:
            parent[a] = b
    cycles: Dict[Tuple[int, int], List[Tuple[int, int]]] = {}
    for c in sorted(parent):
        cycles.setdefault(find(c), []).append(c)
    sigma = [[(j, i) for i in range(n)] for j in range(len(cs.equality))]
    for members in cycles.values():
        for c, nxt in zip(members, members[1:] + members[:1]):
            sigma[c[0]][c[1]] = nxt
    return sigma


def permutation_columns_ints(cs: ConstraintSystem, layout: "AnyLayout", omega: int, delta: int) -> List[List[int]]:
    """The sigma columns as integers: cell (j, i) stands for delta^j * omega^i."""
    n = layout.n
    w = [1] * n
    for i in range(1, n):
        w[i] = w[i - 1] * omega % R
    d = [pow(delta, j, R) for j in range(len(cs.equality))]
    return [[d[j2] * w[i2] % R for (j2, i2) in col] for col in permutation_cells(cs, layout)]


def permutation_columns(cs: ConstraintSystem, layout: "AnyLayout", omega: int, delta: int, device="cuda"):
    """The sigma columns as a (P, n, 4) int64 device tensor: the identity columns delta^j * omega^i from ``hm_fr_powers_dev`` /
    ``hm_fr_scale_dev``, the cells of the copy cycles scattered in."""
    import torch

    lib, n, P = _lib.load(), layout.n, len(cs.equality)
    out = torch.empty((P, n, 4), dtype=torch.int64, device=device)
    with torch.cuda.device(out.device):
        stream = ctypes.c_void_p(_stream_ptr(out))
        for j in range(P):
            _lib.check(lib.hm_fr_powers_dev(ctypes.c_void_p(out[j].data_ptr()), n, _ptr(fr_words(omega)), stream))
            if j:
                _lib.check(lib.hm_fr_scale_dev(ctypes.c_void_p(out[j].data_ptr()), n, _ptr(fr_words(pow(delta, j, R))), stream))
    moved = [(j, i, c) for j, col in enumerate(permutation_cells(cs, layout)) for i, c in enumerate(col) if c != (j, i)]
    if moved:
        w = {}
        vals = []
        for _, _, (j2, i2) in moved:
            if i2 not in w:
                w[i2] = pow(omega, i2, R)
            vals.append(pow(delta, j2, R) * w[i2] % R)
        at = torch.tensor([j * n + i for j, i, _ in moved], dtype=torch.int64, device=out.device)
        out.view(P * n, 4)[at] = torch.from_numpy(ints_to_words(vals).view(np.int64)).to(out.device)
    return out


# ---- the witnesses on the GPU -----------------------------------------------------------------------------------------------------
def _c_layout(entry: str, spec: Spec, args: Tuple[int, ...], names: Tuple[str, ...]) -> Dict[str, int]:
    rows, n_adv, reg = ctypes.c_uint32(0), ctypes.c_uint32(0), (ctypes.c_uint32 * len(names))()
    _lib.check(getattr(_lib.load(), entry)(spec.r_f, spec.r_p, *args, ctypes.byref(rows), ctypes.byref(n_adv), reg))
    return {"used_rows": rows.value, "n_advice": n_adv.value, **dict(zip(names, reg))}


def c_layout(depth: int, k: int, spec: Optional[Spec] = None) -> Dict[str, int]:
    """``hm_merkle_sum_witness_layout``: the placement the kernel uses (no device needed)."""
    return _c_layout("hm_merkle_sum_witness_layout", default_spec(5) if spec is None else spec, (depth, k),
                     ("perm_rows", "level_rows", "lt_row", "const_row"))


def merkle_c_layout(depth: int, k: int, spec: Optional[Spec] = None) -> Dict[str, int]:
    """``hm_merkle_witness_layout``: the placement the MerkleTreeV3 kernel uses (no device needed)."""
    return _c_layout("hm_merkle_witness_layout", default_spec(3) if spec is None else spec, (depth, k), ("perm_rows", "level_rows", "const_row"))


def poseidon_c_layout(k: int, spec: Optional[Spec] = None) -> Dict[str, int]:
    """``hm_poseidon_witness_layout``: the placement the Poseidon circuit's kernel uses (level_rows: the rows before the constants)."""
    return _c_layout("hm_poseidon_witness_layout", default_spec(5) if spec is None else spec, (k,), ("perm_rows", "level_rows", "const_row"))


def _witness_out(who: str, out, m: int, n_advice: int, n: int, device):
    import torch

    if out is None:
        return torch.empty((m, n_advice, n, 4), dtype=torch.int64, device=device)
    if not (out.is_cuda and out.is_contiguous() and out.element_size() == 8 and out.numel() == m * n_advice * n * 4):
        raise ValueError(f"{who}: out must be a contiguous (m, {n_advice}, 2^k, 4) GPU tensor")
    return out


def _path_tensors(who: str, elements: int, leaves, siblings, indices, nodes, out) -> Tuple[int, int]:
    """the checks of the path circuits' GPU tensors (``elements`` per node) -> (m, depth)"""
    m = _tensor_rows(leaves, 4 * elements, "leaves")
    if m == 0:
        raise ValueError(f"{who}: no paths")
    depth = _tensor_rows(siblings, 4 * elements * m, "siblings")
    if not (indices.is_cuda and indices.is_contiguous() and indices.element_size() == 8 and indices.numel() == m):
        raise ValueError(f"{who}: indices must be m 64-bit integers on the GPU")
    if nodes is not None and not (nodes.is_cuda and nodes.is_contiguous() and nodes.element_size() == 8
                                  and nodes.numel() == ((2 << depth) - 1) * 4 * elements):
        raise ValueError(f"{who}: nodes must be the contiguous (2^(depth+1) - 1, {elements}, 4) GPU tensor of a tree of depth {depth}")
    for name, t in (("siblings", siblings), ("indices", indices), ("nodes", nodes), ("out", out)):
        if t is not None and t.is_cuda and t.device != leaves.device:
            raise ValueError(f"{who}: {name} is on {t.device}, leaves on {leaves.device}")
    for name, t in (("leaves", leaves), ("siblings", siblings), ("nodes", nodes), ("out", out)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{who}: {name} must be 16-byte aligned")
    return m, depth


def merkle_sum_witness(spec: Optional[Spec], leaves, siblings, indices, assets_sum: int, k: int, nodes=None, out=None):
    """The witnesses of m inclusion paths: ``leaves`` (m, 2, 4), ``siblings`` (m, depth, 2, 4) as ``hm_merkle_paths_dev`` writes
    them and ``indices`` (m,) int64 (bit l = right child at level l) are GPU tensors of canonical Montgomery words; ``nodes`` is
    the built tree's node tensor (the path's nodes are read from it) or None (they are hashed from the siblings).
    -> (advice (m, N_ADVICE, 2^k, 4), instance (m, 4, 4)) int64 tensors, every word written; asynchronous on the current stream.
    ``out``: an advice tensor to fill instead of a new one (it may be uninitialised)."""
    import torch

    spec = default_spec(5) if spec is None else spec
    m, depth = _path_tensors("merkle_sum_witness", 2, leaves, siblings, indices, nodes, out)
    out = _witness_out("merkle_sum_witness", out, m, N_ADVICE, 1 << k, leaves.device)
    inst = torch.empty((m, 4, 4), dtype=torch.int64, device=leaves.device)
    assets = np.ascontiguousarray(fr_words(int(assets_sum) % R))
    with torch.cuda.device(leaves.device):
        spec.call(_lib.load().hm_merkle_sum_witness_bn256_dev, depth, k, m, ctypes.c_void_p(leaves.data_ptr()),
                  ctypes.c_void_p(siblings.data_ptr()), _dev_ptr(indices),
                  _ptr(assets), ctypes.c_void_p(nodes.data_ptr()) if nodes is not None else None,
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(inst.data_ptr()), ctypes.c_void_p(_stream_ptr(leaves)))
    return out, inst


def merkle_sum_witness_host(spec: Optional[Spec], leaves: np.ndarray, siblings: np.ndarray, indices: np.ndarray, assets_sum: int, k: int):
    """``merkle_sum_witness`` on numpy arrays through the host-pointer form (small m: the columns must stay below 256 MiB)."""
    spec = default_spec(5) if spec is None else spec
    lv = np.ascontiguousarray(np.asarray(leaves, dtype=np.uint64).reshape(-1, 2, 4))
    m = lv.shape[0]
    sb = np.ascontiguousarray(np.asarray(siblings, dtype=np.uint64).reshape(m, -1, 2, 4))
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(m))
    adv = np.zeros((m, N_ADVICE, 1 << k, 4), dtype=np.uint64)
    inst = np.zeros((m, 4, 4), dtype=np.uint64)
    p = _ptr
    spec.call(_lib.load().hm_merkle_sum_witness_bn256, sb.shape[1], k, m, p(lv), p(sb), p(idx), p(np.ascontiguousarray(fr_words(int(assets_sum) % R))),
              p(adv), p(inst))
    return adv, inst


def merkle_witness(spec: Optional[Spec], leaves, siblings, indices, k: int, nodes=None, out=None):
    """The MerkleTreeV3 witnesses of m inclusion paths: ``leaves`` (m, 4), ``siblings`` (m, depth, 4) as ``hm_merkle_paths_dev``
    writes them with one word per node and ``indices`` (m,) int64 (bit l = right child at level l) are GPU tensors of canonical
    Montgomery words; ``nodes`` is the built tree's node tensor or None (the path's nodes are hashed from the siblings).
    -> (advice (m, 7, 2^k, 4), instance (m, 2, 4)) int64 tensors, every word written; asynchronous on the current stream.
    ``out``: an advice tensor to fill instead of a new one (it may be uninitialised)."""
    import torch

    spec = default_spec(3) if spec is None else spec
    m, depth = _path_tensors("merkle_witness", 1, leaves, siblings, indices, nodes, out)
    out = _witness_out("merkle_witness", out, m, MerkleTreeV3Layout.N_ADVICE, 1 << k, leaves.device)
    inst = torch.empty((m, 2, 4), dtype=torch.int64, device=leaves.device)
    with torch.cuda.device(leaves.device):
        spec.call(_lib.load().hm_merkle_witness_bn256_dev, depth, k, m, ctypes.c_void_p(leaves.data_ptr()),
                  ctypes.c_void_p(siblings.data_ptr()), _dev_ptr(indices),
                  ctypes.c_void_p(nodes.data_ptr()) if nodes is not None else None,
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(inst.data_ptr()), ctypes.c_void_p(_stream_ptr(leaves)))
    return out, inst


def merkle_witness_host(spec: Optional[Spec], leaves: np.ndarray, siblings: np.ndarray, indices: np.ndarray, k: int):
    """``merkle_witness`` on numpy arrays through the host-pointer form (small m: the columns must stay below 256 MiB)."""
    spec = default_spec(3) if spec is None else spec
    lv = np.ascontiguousarray(np.asarray(leaves, dtype=np.uint64).reshape(-1, 4))
    m = lv.shape[0]
    if m == 0:
        raise ValueError("merkle_witness_host: no paths")
    sb = np.ascontiguousarray(np.asarray(siblings, dtype=np.uint64).reshape(m, -1, 4))
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(m))
    adv = np.zeros((m, MerkleTreeV3Layout.N_ADVICE, 1 << k, 4), dtype=np.uint64)
    inst = np.zeros((m, 2, 4), dtype=np.uint64)
    spec.call(_lib.load().hm_merkle_witness_bn256, sb.shape[1], k, m, _ptr(lv), _ptr(sb), _ptr(idx), _ptr(adv), _ptr(inst))
    return adv, inst


def poseidon_circuit_witness(spec: Optional[Spec], msgs, k: int, out=None):
    """The Poseidon circuit's witnesses of m messages: ``msgs`` (m, 4, 4) GPU tensor of canonical Montgomery words
    -> (advice (m, 6, 2^k, 4), instance (m, 1, 4)); every word written; asynchronous on the current stream."""
    import torch

    spec = default_spec(5) if spec is None else spec
    m = _tensor_rows(msgs, 16, "msgs")
    if m == 0:
        raise ValueError("poseidon_circuit_witness: no messages")
    if out is not None and out.is_cuda and out.device != msgs.device:
        raise ValueError(f"poseidon_circuit_witness: out is on {out.device}, msgs on {msgs.device}")
    for name, t in (("msgs", msgs), ("out", out)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"poseidon_circuit_witness: {name} must be 16-byte aligned")
    out = _witness_out("poseidon_circuit_witness", out, m, PoseidonCircuitLayout.N_ADVICE, 1 << k, msgs.device)
    inst = torch.empty((m, 1, 4), dtype=torch.int64, device=msgs.device)
    with torch.cuda.device(msgs.device):
        spec.call(_lib.load().hm_poseidon_witness_bn256_dev, k, m, ctypes.c_void_p(msgs.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                  ctypes.c_void_p(inst.data_ptr()), ctypes.c_void_p(_stream_ptr(msgs)))
    return out, inst


def poseidon_circuit_witness_host(spec: Optional[Spec], msgs: np.ndarray, k: int):
    """``poseidon_circuit_witness`` on a numpy (m, 4, 4) array through the host-pointer form (columns below 256 MiB)."""
    spec = default_spec(5) if spec is None else spec
    ms = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64).reshape(-1, 4, 4))
    m = ms.shape[0]
    if m == 0:
        raise ValueError("poseidon_circuit_witness_host: no messages")
    adv = np.zeros((m, PoseidonCircuitLayout.N_ADVICE, 1 << k, 4), dtype=np.uint64)
    inst = np.zeros((m, 1, 4), dtype=np.uint64)
    spec.call(_lib.load().hm_poseidon_witness_bn256, k, m, _ptr(ms), _ptr(adv), _ptr(inst))
    return adv, inst


def range_c_layout(k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1) -> Dict[str, int]:
    """``hm_range_witness_layout``: the numbers the range-check kernel uses (no device needed), beside ``RangeCheckLayout``'s;
    ValueError when the two differ."""
    n_adv, table_rows = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(_lib.load().hm_range_witness_layout(max_bits, acc_cols, k, rows, ctypes.byref(n_adv), ctypes.byref(table_rows)))
    lay = RangeCheckLayout(k, max_bits, acc_cols, rows)
    out = {"n_advice": n_adv.value, "table_rows": table_rows.value}
    if out != {"n_advice": lay.N_ADVICE, "table_rows": lay.table_rows}:
        raise ValueError(f"range_c_layout: the C layout {out} is not RangeCheckLayout's")
    return out


def range_witness(values, k: int, max_bits: int = 4, acc_cols: int = 4, out=None):
    """The range-check witnesses of m circuits: ``values`` (m, rows, 4) -- or (rows, 4), one circuit -- GPU tensor of canonical
    Montgomery words -> (advice (m, 1 + acc_cols, 2^k, 4), over (m,) int32: per circuit the values at or above
    2^(max_bits * acc_cols), whose limbs are their low bits only); every word written, rows >= ``rows`` zero; asynchronous on the
    current stream.  ``out``: an advice tensor to fill instead of a new one (it may be uninitialised)."""
    import torch

    if not (_is_cuda_words(values) and values.dim() in (2, 3) and values.shape[-1] == 4):
        raise ValueError("range_witness: values must be a contiguous (m, rows, 4) or (rows, 4) 64-bit GPU tensor")
    m, rows = (1, values.shape[0]) if values.dim() == 2 else (values.shape[0], values.shape[1])
    if m == 0 or rows == 0:
        raise ValueError("range_witness: no values")
    if out is not None and out.is_cuda and out.device != values.device:
        raise ValueError(f"range_witness: out is on {out.device}, values on {values.device}")
    for name, t in (("values", values), ("out", out)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"range_witness: {name} must be 16-byte aligned")
    out = _witness_out("range_witness", out, m, 1 + acc_cols, 1 << k, values.device)
    over = torch.empty(m, dtype=torch.int32, device=values.device)
    with torch.cuda.device(values.device):
        _lib.check(_lib.load().hm_range_witness_bn256_fr_dev(max_bits, acc_cols, k, m, rows, ctypes.c_void_p(values.data_ptr()),
                                                            ctypes.c_void_p(out.data_ptr()), _dev_ptr(over, _u32p),
                                                            ctypes.c_void_p(_stream_ptr(values))))
    return out, over


def range_witness_host(values: np.ndarray, k: int, max_bits: int = 4, acc_cols: int = 4):
    """``range_witness`` on a numpy (m, rows, 4) array through the host-pointer form (columns below 256 MiB)."""
    vs = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    if vs.ndim == 2:
        vs = vs.reshape(1, -1, 4)
    if vs.ndim != 3 or vs.shape[2] != 4 or vs.shape[0] == 0 or vs.shape[1] == 0:
        raise ValueError("range_witness_host: values must be a non-empty (m, rows, 4) array")
    m, rows = vs.shape[0], vs.shape[1]
    adv = np.zeros((m, 1 + acc_cols, 1 << k, 4), dtype=np.uint64)
    over = np.zeros(m, dtype=np.uint32)
    _lib.check(_lib.load().hm_range_witness_bn256_fr(max_bits, acc_cols, k, m, rows, _ptr(vs), _ptr(adv), over.ctypes.data_as(_u32p)))
    return adv, over


def sorted_c_layout(k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1) -> Dict[str, int]:
    """``hm_sorted_witness_layout``: the numbers the sorted-column kernel uses (no device needed), beside ``SortedColumnLayout``'s;
    ValueError when the two differ."""
    n_adv, table_rows = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(_lib.load().hm_sorted_witness_layout(max_bits, acc_cols, k, rows, ctypes.byref(n_adv), ctypes.byref(table_rows)))
    lay = SortedColumnLayout(k, max_bits, acc_cols, rows)
    out = {"n_advice": n_adv.value, "table_rows": table_rows.value}
    if out != {"n_advice": lay.N_ADVICE, "table_rows": lay.table_rows}:
        raise ValueError(f"sorted_c_layout: the C layout {out} is not SortedColumnLayout's")
    return out


def sorted_witness(ids, k: int, max_bits: int = 4, acc_cols: int = 4, out=None):
    """The sorted-column witnesses of m circuits: ``ids`` (m, rows, 4) -- or (rows, 4), one circuit -- GPU tensor of canonical
    Montgomery words -> (advice (m, 1 + acc_cols, 2^k, 4), over (m,) int32: per circuit the rows i <= rows - 2 whose gap
    id[i+1] - id[i] - 1 mod r is at or above 2^(max_bits * acc_cols) -- ids out of order, equal or too far apart -- whose limbs are
    the gap's low bits only); every word written, the limbs of rows >= ``rows`` - 1 zero; asynchronous on the current stream.
    ``out``: an advice tensor to fill instead of a new one (it may be uninitialised)."""
    import torch

    if not (_is_cuda_words(ids) and ids.dim() in (2, 3) and ids.shape[-1] == 4):
        raise ValueError("sorted_witness: ids must be a contiguous (m, rows, 4) or (rows, 4) 64-bit GPU tensor")
    m, rows = (1, ids.shape[0]) if ids.dim() == 2 else (ids.shape[0], ids.shape[1])
    if m == 0 or rows == 0:
        raise ValueError("sorted_witness: no ids")
    if out is not None and out.is_cuda and out.device != ids.device:
        raise ValueError(f"sorted_witness: out is on {out.device}, ids on {ids.device}")
    for name, t in (("ids", ids), ("out", out)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"sorted_witness: {name} must be 16-byte aligned")
    out = _witness_out("sorted_witness", out, m, 1 + acc_cols, 1 << k, ids.device)
    over = torch.empty(m, dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.load().hm_sorted_witness_bn256_fr_dev(max_bits, acc_cols, k, m, rows, ctypes.c_void_p(ids.data_ptr()),
                                                             ctypes.c_void_p(out.data_ptr()), _dev_ptr(over, _u32p),
                                                             ctypes.c_void_p(_stream_ptr(ids))))
    return out, over


def sorted_witness_host(ids: np.ndarray, k: int, max_bits: int = 4, acc_cols: int = 4):
    """``sorted_witness`` on a numpy (m, rows, 4) array through the host-pointer form (columns below 256 MiB)."""
    vs = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
    if vs.ndim == 2:
        vs = vs.reshape(1, -1, 4)
    if vs.ndim != 3 or vs.shape[2] != 4 or vs.shape[0] == 0 or vs.shape[1] == 0:
        raise ValueError("sorted_witness_host: ids must be a non-empty (m, rows, 4) array")
    m, rows = vs.shape[0], vs.shape[1]
    adv = np.zeros((m, 1 + acc_cols, 1 << k, 4), dtype=np.uint64)
    over = np.zeros(m, dtype=np.uint32)
    _lib.check(_lib.load().hm_sorted_witness_bn256_fr(max_bits, acc_cols, k, m, rows, _ptr(vs), _ptr(adv), over.ctypes.data_as(_u32p)))
    return adv, over


ACCUMULATOR_BLOCK_ROWS = 256          # csrc/accumulator.hip: ACC_THREADS, the table rows one block of the accumulator kernels takes


def accumulator_c_layout(k: int, max_bits: int = 4, acc_cols: int = 4, rows: int = 1) -> Dict[str, int]:
    """``hm_accumulator_witness_layout``: the numbers the accumulator kernels use (no device needed), beside
    ``SafeAccumulatorLayout``'s; ValueError when the two differ."""
    n_adv, used = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(_lib.load().hm_accumulator_witness_layout(max_bits, acc_cols, k, rows, ctypes.byref(n_adv), ctypes.byref(used)))
    lay = SafeAccumulatorLayout(k, max_bits, acc_cols, rows)
    out = {"n_advice": n_adv.value, "used_rows": used.value}
    if out != {"n_advice": lay.N_ADVICE, "used_rows": lay.used_rows}:
        raise ValueError(f"accumulator_c_layout: the C layout {out} is not SafeAccumulatorLayout's")
    return out


def _accumulator_shapes(who: str, values_shape, initial_shape, k: int, max_bits: int, acc_cols: int) -> Tuple[int, int]:
    """what both forms of the accumulator witness refuse before anything is launched -> (m, rows)"""
    SafeAccumulatorLayout(max(k, 3), max_bits, acc_cols, 1)          # the parameter limits, stated once
    if len(values_shape) != 3 or values_shape[2] != 4 or values_shape[0] == 0 or values_shape[1] == 0:
        raise ValueError(f"{who}: values must be a non-empty (m, rows, 4) array of 64-bit words")
    m, rows = values_shape[0], values_shape[1]
    if tuple(initial_shape) != (m, acc_cols):
        raise ValueError(f"{who}: initial must be (m, acc_cols) = ({m}, {acc_cols}) plain limbs, not {tuple(initial_shape)}")
    if m > 65535:
        raise ValueError(f"{who}: at most 65535 circuits a call")
    SafeAccumulatorLayout(k, max_bits, acc_cols, rows)               # rows + 1 <= 2^k - 6
    return m, rows


def accumulator_witness(values, initial, k: int, max_bits: int = 4, acc_cols: int = 4, out=None, parts: Optional[list] = None):
    """The SafeAccumulator witnesses of m circuits: ``values`` (m, rows, 4) GPU tensor of canonical Montgomery words, ``initial``
    (m, acc_cols) int64 GPU tensor of plain limb integers, most significant first -> (advice (m, 2 + 2 acc_cols, 2^k, 4), finals
    (m, acc_cols) int64: the plain final limbs, which are the instance, over (m,) int32: per circuit the rows whose value is at or
    above 2^max_bits or whose top limb is not zero, plus 1 for a bad initial state); every word written, rows above ``rows`` zero;
    asynchronous on the current stream.  ``out``: an advice tensor to fill instead of a new one (it may be uninitialised).
    ``parts``: a list that receives the device milliseconds of the call's four launches (block totals, their scan, the rows, the
    counters); the call then waits for the stream (``hm_accumulator_witness_timed_bn256_fr_dev``; tools/accumulator_witness_time.py).
    ValueError, with nothing launched: wrong shapes, rows + 1 > 2^k - 6, max_bits * acc_cols > 64."""
    import torch

    if not (_is_cuda_words(values) and _is_cuda_words(initial)):
        raise ValueError("accumulator_witness: values and initial must be contiguous 64-bit GPU tensors")
    m, rows = _accumulator_shapes("accumulator_witness", tuple(values.shape), tuple(initial.shape), k, max_bits, acc_cols)
    for name, t in (("initial", initial), ("out", out)):
        if t is not None and t.is_cuda and t.device != values.device:
            raise ValueError(f"accumulator_witness: {name} is on {t.device}, values on {values.device}")
    for name, t in (("values", values), ("out", out)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"accumulator_witness: {name} must be 16-byte aligned")
    out = _witness_out("accumulator_witness", out, m, 2 + 2 * acc_cols, 1 << k, values.device)
    finals = torch.empty((m, acc_cols), dtype=torch.int64, device=values.device)
    over = torch.empty(m, dtype=torch.int32, device=values.device)
    args = (max_bits, acc_cols, k, m, rows, ctypes.c_void_p(values.data_ptr()), _dev_ptr(initial), ctypes.c_void_p(out.data_ptr()),
            _dev_ptr(finals), _dev_ptr(over, _u32p), ctypes.c_void_p(_stream_ptr(values)))
    with torch.cuda.device(values.device):
        if parts is None:
            _lib.check(_lib.load().hm_accumulator_witness_bn256_fr_dev(*args))
        else:
            ms = (ctypes.c_double * 4)()
            _lib.check(_lib.load().hm_accumulator_witness_timed_bn256_fr_dev(*args, ms))
            parts[:] = list(ms)
    return out, finals, over


def accumulator_witness_host(values: np.ndarray, initial: np.ndarray, k: int, max_bits: int = 4, acc_cols: int = 4):
    """``accumulator_witness`` on numpy arrays, (m, rows, 4) words and (m, acc_cols) limbs, through the host-pointer form (columns
    below 256 MiB)."""
    vs = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    init = np.ascontiguousarray(np.asarray(initial, dtype=np.uint64))
    m, rows = _accumulator_shapes("accumulator_witness_host", vs.shape, init.shape, k, max_bits, acc_cols)
    adv = np.zeros((m, 2 + 2 * acc_cols, 1 << k, 4), dtype=np.uint64)
    finals = np.zeros((m, acc_cols), dtype=np.uint64)
    over = np.zeros(m, dtype=np.uint32)
    _lib.check(_lib.load().hm_accumulator_witness_bn256_fr(max_bits, acc_cols, k, m, rows, _ptr(vs), _ptr(init), _ptr(adv), _ptr(finals),
                                                          over.ctypes.data_as(_u32p)))
    return adv, finals, over


def _is_cuda_words(t) -> bool:
    return hasattr(t, "is_cuda") and t.is_cuda and t.is_contiguous() and t.element_size() == 8


columns_to_words = fr_array      # integer columns -> (len(cols), n, 4) uint64 Montgomery words (what the device tensors hold)
