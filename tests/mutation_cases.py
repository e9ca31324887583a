"""The mutation sweep's cases (tests/test_mutation_sweep.py, tests/test_mutation_sweep_gpu.py): one satisfied witness per circuit, built
from integers alone (``assign_ints``, ``instance``, ``fixed_columns``, ``copies``; no GPU), the list of single cells to change, the
yardstick's verdict on every such change (tests/mock_prover.py), and ``EXPECTED``: which cells the circuit constrains and by what --
a gate, a copy, a lookup -- written down as data, region by region, from the reference's chips.  ``EXPECTED`` is NOT computed from the
constraint system: it is what the transcription in circuits.py / synthesis.py is held against.

A mutant is one advice cell plus ``delta`` mod r.  Its verdict is the number of gate polynomials, copies and lookups that fail; a cell
is *constrained* when a gate or a copy does, whatever the delta.  The lookups are kept apart because they depend on the delta and
carry no selector: every usable row of a diff column (LtChip) or a limb column is range-checked, so such a cell plus 1 passes where
the sum stays in the table and a cell plus a random element never does (``LOOKUP_COLUMNS``, ``leaves_table``).

What a single-cell change cannot see: a constraint that only a joint change of several cells would break (the reference's own
``check`` / ``is_lt`` pair on the less-than row: changing both together to 0 satisfies "check == is_lt" -- and then only the
"lt gate" stands, which is what it is there for).

The sum tree's assets are NOT 2^50: with a total below the assets the chip's diff is 2^64 - (assets - total), whose top byte is 255
unless the assets exceed the total by 2^56 or more, and +1 on a byte of 255 leaves the u8 table.  The assets here are the total plus
a constant chosen so that every diff byte is in 1 .. 254 (asserted)."""
import random
from types import SimpleNamespace

from halo2_experiments_amd import circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R

import mock_prover as yardstick

NAMES = ["poseidon", "merkle_v3", "merkle_sum_tree", "overflow_check_v2"]
DELTAS = {"one": 1, "random": random.Random(0xD317A).randrange(1 << 200, R)}
KINDS = ("gate", "copy", "lookup")
SUM_DIFF = 0x5A3C96172B4D6E81                    # the sum tree's eight diff bytes, little-endian: none 0, none 255
# the table of the issue: (advice cells, constrained, constrained but zero)
TOTALS = {"poseidon": (384, 240, 8), "merkle_v3": (896, 311, 9), "merkle_sum_tree": (10240, 498, 17), "overflow_check_v2": (160, 130, None)}
SWEPT = {"poseidon": 384, "merkle_v3": 896, "merkle_sum_tree": 1980, "overflow_check_v2": 160}


def _case(name, cs, lay, advice, instance, inst_rows, proof_instance):
    n = lay.n
    inst_cols = [list(col) + [0] * (n - len(col)) for col in instance]
    fixed = lay.fixed_columns()
    usable = n - (cs.blinding_factors + 1)
    return SimpleNamespace(name=name, cs=cs, lay=lay, k=lay.k, n=n, usable=usable, advice=advice, instance=inst_cols, inst_rows=inst_rows,
                           proof_instance=proof_instance, fixed=fixed, copies=lay.copies(),
                           tables=yardstick.lookup_tables(cs, fixed, advice, inst_cols, n, usable))


def build(name):
    """-> the case: cs, lay, k, n, usable, advice / instance / fixed as integer columns of n rows, copies, the lookups' tables,
    inst_rows (the instance rows the circuit uses) and proof_instance (the instance in the form create_proof takes)"""
    rng = random.Random(NAMES.index(name) + 20240)
    if name == "poseidon":
        spec = ps.default_spec(5)
        cs, lay = circuits.poseidon(spec), sy.PoseidonCircuitLayout(6, spec)
        adv = lay.assign_ints([rng.randrange(1, R) for _ in range(4)])
        _, col, row = lay.digest_cell(0)
        inst = lay.instance(adv[col][row])
    elif name == "merkle_v3":
        spec, depth = ps.default_spec(3), 2
        k = sy.MerkleTreeV3Layout.min_k(depth, spec)
        assert k == 7
        cs, lay = circuits.merkle_v3(spec), sy.MerkleTreeV3Layout(depth, k, spec)
        leaf = rng.randrange(1, R)
        adv = lay.assign_ints(leaf, [rng.randrange(1, R) for _ in range(depth)], [1, 0])
        _, col, row = lay.digest_cell(depth - 1)
        inst = lay.instance(leaf, adv[col][row])
    elif name == "merkle_sum_tree":
        spec, depth = ps.default_spec(5), 2
        cs, lay = circuits.merkle_sum_tree(spec), sy.MerkleSumTreeLayout(depth, 9, spec)
        leaf = (rng.randrange(1, R), rng.randrange(1, 1 << 40))
        sib = [(rng.randrange(1, R), rng.randrange(1, 1 << 40)) for _ in range(depth)]
        total = leaf[1] + sum(b for _, b in sib)
        assets = total + (1 << 64) - SUM_DIFF                      # above the total; diff = total - assets + 2^64 = SUM_DIFF
        adv = lay.assign_ints(leaf, sib, [0, 1], assets)
        assert total < assets < 1 << 64 and adv[sy.LT][lay.lt_row] == 1
        diff = [adv[c][lay.lt_row] for c in sy.DIFF]
        assert diff == list(SUM_DIFF.to_bytes(8, "little")) and all(0 < b < 255 for b in diff)       # +1 stays a byte
        _, col, row = lay.digest_cell(depth - 1)
        inst = lay.instance(leaf, adv[col][row], assets)
    elif name == "overflow_check_v2":
        cs, lay = circuits.overflow_check_v2(4, 4), sy.RangeCheckLayout(5, 4, 4, 26)
        values = [rng.randrange(1 << 16) for _ in range(26)]
        values[0], values[25] = 0xF3AF, 0x1F0F                    # limbs of 15, where +1 leaves the table, on the first and last usable row
        adv = lay.assign_ints(values)
        inst = lay.instance()
    else:
        raise KeyError(name)
    lay.check_constraint_system(cs)
    rows = getattr(lay, "N_INSTANCE_ROWS", 0)
    case = _case(name, cs, lay, adv, inst, rows, [[]] if rows == 0 else list(inst[0][:rows]))
    assert yardstick.verify(cs, case.fixed, adv, case.instance, case.copies, case.n, case.usable) == [], name      # satisfied to begin with
    return case


_CASES = {}


def case(name):
    """``build(name)``, made once; the columns are changed in place by ``host_verdicts`` and always put back"""
    if name not in _CASES:
        _CASES[name] = build(name)
    return _CASES[name]


def swept_rows(c):
    """every row for the three small circuits; the sum tree: rows 0 .. lt_row + 2 and the last 8 rows -- every row between holds no
    advice assignment and no enabled selector (asserted from the regions and the selector rows)"""
    if c.name != "merkle_sum_tree":
        return list(range(c.n))
    lay = c.lay
    rows = list(range(lay.lt_row + 3)) + list(range(c.n - 8, c.n))
    left_out = set(range(c.n)) - set(rows)
    for region in lay.regions:
        if any(kind == "advice" for kind, _ in region.columns):
            assert not left_out & set(region.rows), region.name
    for column, enabled in lay.selector_rows().items():
        assert not left_out & set(enabled), column
    assert all(c.advice[col][row] == 0 for col in range(c.cs.num_advice) for row in left_out)
    return rows


def mutants(c, delta=1):
    """the advice cells to change, as (column, row): the same list for every delta"""
    cells = [(col, row) for row in swept_rows(c) for col in range(c.cs.num_advice)]
    assert len(cells) == SWEPT[c.name]
    return cells


def instance_mutants(c):
    return [(0, row) for row in range(c.inst_rows)]


def neighbours(c, row):
    return sorted({(row - 1) % c.n, row, (row + 1) % c.n})


def host_verdicts(c, cells, delta, cs=None, copies=None, tables=None, kind="advice"):
    """-> per cell, (gate polynomials, copies, lookups that fail with that cell plus delta, rows with a failing gate): the yardstick
    on the mutated row and its neighbours (every rotation of every gate here is -1, 0 or 1).  cs / copies / tables: a changed constraint system (negative controls)."""
    cs = c.cs if cs is None else cs
    copies = c.copies if copies is None else copies
    tables = c.tables if tables is None else tables
    columns = c.advice if kind == "advice" else c.instance
    out = []
    for col, row in cells:
        keep = columns[col][row]
        columns[col][row] = (keep + delta) % R
        try:
            fails = yardstick.verify(cs, c.fixed, c.advice, c.instance, copies, c.n, c.usable, rows=neighbours(c, row), tables=tables)
        finally:
            columns[col][row] = keep
        out.append(tuple(sum(f[0] == kd for f in fails) for kd in KINDS) + (len({f[3] for f in fails if f[0] == "gate"}),))
    return out


_VERDICTS = {}


def verdicts(name, delta_name):
    """(cells, verdicts) of ``mutants`` / ``host_verdicts`` for the case and ``DELTAS[delta_name]``: computed once, never changed"""
    if (name, delta_name) not in _VERDICTS:
        c = case(name)
        cells = mutants(c, DELTAS[delta_name])
        _VERDICTS[name, delta_name] = (cells, host_verdicts(c, cells, DELTAS[delta_name]))
    return _VERDICTS[name, delta_name]


def caught_by(cells, verdicts):
    """-> {kind: set of cells with a failure of that kind}, "constrained": gate or copy, "failing": any of the three"""
    sets = {kd: {cell for cell, v in zip(cells, verdicts) if v[i]} for i, kd in enumerate(KINDS)}
    sets["constrained"] = sets["gate"] | sets["copy"]
    sets["failing"] = sets["constrained"] | sets["lookup"]
    return sets


def leaves_table(c, col, row, delta):
    """does advice cell (col, row) plus delta leave the table of a lookup that reads it (every lookup here reads one advice cell at
    rotation 0 and a fixed table)"""
    for li, (ins, _) in enumerate(c.cs.lookups):
        if ins[0].column == col and row < c.usable and ((c.advice[col][row] + delta) % R,) not in c.tables[li]:
            return True
    return False


# ---- what the circuits constrain, as data ------------------------------------------------------------------------------------------
# (region name, advice columns, row offsets inside the region, caught by: g a gate / c a copy, where the reference assigns or
#  constrains the cell).  A name stands for every region of that name ("... 0", "... 1": one per level).
def _pow5(state, sbox, rate, digest_to):
    """halo2_gadgets Pow5Chip as synthesis.py's module docstring cites it (r_f = 8, r_p = 56: 4 + 28 + 4 rows and the final state)"""
    return [
        ("initial state", state, (0,), "c", "Pow5Chip initial_state: assign_advice_from_constant, copied into pad-and-add row 0"),
        ("pad-and-add", state, (0, 2), "gc", "Pow5Chip add_input: the initial state copied to row 0, the sum on row 2 copied to permute row 0; "
                                            "the pad-and-add gate reads both from row 1"),
        ("pad-and-add", state[:rate], (1,), "gc", "Pow5Chip add_input: the message copied to row 1 (the capacity word of row 1 is not read)"),
        ("permute state", state, (0,), "gc", "Pow5Chip permute: the sum copied in; the first full round reads it"),
        ("permute state", state, tuple(range(1, 36)), "g", "Pow5Chip full / partial rounds: every row is the next rotation of the row above"),
        ("permute state", state[:1], (36,), "gc", "the digest: the last round's output, " + digest_to),
        ("permute state", state[1:], (36,), "g", "Pow5Chip: the last full round's output"),
        ("permute state", (sbox,), tuple(range(4, 32)), "g", "Pow5Chip partial rounds: partial_sbox on the 28 rows of s_partial"),
    ]


EXPECTED = {
    "poseidon": [
        ("load private inputs", (0, 1, 2, 3), (0,), "c", "chips/poseidon/hash_with_instance.rs:83-101 assign_advice, copied at :119"),
        ("copy input cells to hash input cells", (0, 1, 2, 3), (0,), "c", "chips/poseidon/hash_with_instance.rs:112-139 copy_advice; the hash copies them on"),
    ] + _pow5((0, 1, 2, 3, 4), 5, 4, "constrain_instance chips/poseidon/hash_with_instance.rs:147"),
    "merkle_v3": [
        ("assign leaf", (0,), (0,), "c", "chips/merkle_v3.rs:89-91 assign_advice; :110 copy to level 0, :171 constrain_instance row 0"),
        ("merkle prove layer", (0,), (0,), "gc", "chips/merkle_v3.rs:110 copy_advice of the node; swap gate :56-68"),
        ("merkle prove layer", (1, 2), (0,), "g", "chips/merkle_v3.rs:116, :122 assign_advice; swap gate :56-68 (and the bool gate :47-52 on the index)"),
        ("merkle prove layer", (0, 1), (1,), "gc", "chips/merkle_v3.rs:133, :139 assign_advice; the swap gate's next rotation; copied into the hash :150-161"),
    ] + _pow5((3, 4, 5), 6, 2, "copied to the next level chips/merkle_v3.rs:110 or constrain_instance :171"),
    "merkle_sum_tree": [
        ("assign leaf hash", (0,), (0,), "c", "chips/merkle_sum_tree.rs:146-156 assign_advice; copied :189, exposed as instance row 0"),
        ("assign leaf balance", (1,), (0,), "c", "chips/merkle_sum_tree.rs:158-168 assign_advice; copied :195, exposed as instance row 1"),
        ("merkle prove layer", (0, 1), (0,), "gc", "chips/merkle_sum_tree.rs:189, :195 copy_advice; swap gates :70-92"),
        ("merkle prove layer", (2, 3, 4), (0,), "g", "chips/merkle_sum_tree.rs:201, :207, :213 assign_advice; swap gates :70-92, bool gate :62-66"),
        ("merkle prove layer", (0, 1, 2, 3), (1,), "gc", "chips/merkle_sum_tree.rs:237-263 assign_advice; the swap gates' next rotation; copied into the hash :297-300"),
        ("merkle prove layer", (4,), (1,), "gc", "chips/merkle_sum_tree.rs:271-276 the sum; sum gate :95-101; copied to the next level :195 or to the lt row :321"),
        ("enforce sum to be less than total assets", (0,), (0,), "gc", "chips/merkle_sum_tree.rs:321 copy_advice of the sum; lhs of the lt gate"),
        ("enforce sum to be less than total assets", (1,), (0,), "gc", "chips/merkle_sum_tree.rs:329-335 assign_advice_from_instance row 3; rhs of the lt gate"),
        ("enforce sum to be less than total assets", (2,), (0,), "g", "chips/merkle_sum_tree.rs:338-343 check = 1; the gate check == is_lt :127-138"),
        ("enforce sum to be less than total assets", (11,), (0,), "g", "chips/merkle_sum_tree.rs:348 LtChip::assign lt; lt gate and check == is_lt"),
        ("enforce sum to be less than total assets", tuple(range(12, 20)), (0,), "g", "chips/merkle_sum_tree.rs:348 LtChip::assign diff bytes; lt gate (and LOOKUP_COLUMNS)"),
    ] + _pow5((5, 6, 7, 8, 9), 10, 4, "copied to the next level chips/merkle_sum_tree.rs:189 or exposed as instance row 2"),
    "overflow_check_v2": [
        ("assign decomposed values", (0,), (0,), "g", "chips/overflow_check_v2.rs:92 assign value; the gate :41-59"),
        ("assign decomposed values", (1, 2, 3, 4), (0,), "g", "chips/overflow_check_v2.rs:103 the limbs; the gate :41-59 (and LOOKUP_COLUMNS)"),
    ],
}
# cells the reference assigns that are legitimately free: none at these shapes.  (With fewer values than usable rows the range check's
# unused rows would be: selector off, limbs zero -- rows = 26 uses every usable row.)  Every free cell here is unassigned and zero.
FREE_ASSIGNED = {name: [] for name in NAMES}
# advice columns that a lookup reads, on EVERY usable row (no selector multiplies the input): LtChip's one u8 lookup per diff byte
# (chips/merkle_sum_tree.rs:109-114 configures it), the range lookup per limb column (chips/overflow_check_v2.rs:63-69)
LOOKUP_COLUMNS = {"poseidon": (), "merkle_v3": (), "merkle_sum_tree": tuple(range(12, 20)), "overflow_check_v2": (1, 2, 3, 4)}
LETTER = {"g": "gate", "c": "copy"}


def expected_sets(c):
    """-> {"gate" / "copy": the cells ``EXPECTED`` says that kind catches, "constrained": their union}"""
    out = {"gate": set(), "copy": set()}
    for name, columns, offsets, letters, _ in EXPECTED[c.name]:
        regions = [r for r in c.lay.regions if r.name == name or (r.name.startswith(name + " ") and r.name[len(name) + 1:].isdigit())]
        assert regions, name
        for region in regions:
            assert all(("advice", col) in region.columns for col in columns) and all(off < region.height for off in offsets), name
            for letter in letters:
                out[LETTER[letter]] |= {(col, region.start + off) for col in columns for off in offsets}
    out["constrained"] = out["gate"] | out["copy"]
    return out


def expected_lookup_set(c, cells, delta):
    """the cells of ``LOOKUP_COLUMNS`` on usable rows whose value plus delta is not in the table"""
    assert sorted(LOOKUP_COLUMNS[c.name]) == sorted(ins[0].column for ins, _ in c.cs.lookups)
    return {(col, row) for col, row in cells if col in LOOKUP_COLUMNS[c.name] and leaves_table(c, col, row, delta)}


def free_cells(c, count, blinding, seed=7):
    """`count` cells that no gate and no copy constrains and whose value plus 1 stays in every table, `blinding` of them in blinding
    rows: drawn with a fixed seed from the swept cells"""
    cells, judged = verdicts(c.name, "one")
    free = [cell for cell, v in zip(cells, judged) if not any(v[:3])]
    rng = random.Random(seed)
    tail = rng.sample([cell for cell in free if cell[1] >= c.usable], blinding)
    return sorted(rng.sample([cell for cell in free if cell[1] < c.usable], count - blinding) + tail)


def sum_tree_sample(c, seed=11):
    """The sum tree's stratified sample for the prover (at most 128 cells): every constrained cell of both "merkle prove layer" regions
    and of the lt row; one constrained cell per (region, column) elsewhere; every cell that only a copy constrains; 16 free cells, four
    of them in blinding rows."""
    assert c.name == "merkle_sum_tree"
    sets = caught_by(*verdicts(c.name, "one"))
    rng = random.Random(seed)
    picked = set()
    for region in c.lay.regions:
        inside = sorted(cell for cell in sets["constrained"] if cell[1] in region.rows and ("advice", cell[0]) in region.columns)
        if region.name.startswith("merkle prove layer") or region.name.startswith("enforce sum"):
            picked |= set(inside)
        else:
            for col in sorted({cell[0] for cell in inside}):
                picked.add(rng.choice([cell for cell in inside if cell[0] == col]))
    picked |= sets["copy"] - sets["gate"]
    picked |= set(free_cells(c, 16, 4))
    assert len(picked) <= 128
    return sorted(picked)
