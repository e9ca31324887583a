"""Helper of tests/test_sorted_column.py, tests/test_sorted_column_gpu.py and the ledger's distinctness tests: the id columns a
sorted-column witness is tried on, each with the verdict written beside it, and the mutation sweep's case and expectation."""
import random
from types import SimpleNamespace

from halo2_experiments_amd import circuits, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R

import mock_prover as yardstick

GATE = "next id is this id plus one plus the decomposed gap"


def ascending(rows, width, seed, start=None):
    """`rows` ids in ascending order, neighbours between 1 and 2^width apart (both ends occur when rows allows), from `start`"""
    rnd = random.Random(seed)
    out = [rnd.randrange(1 << 200) if start is None else start]
    for i in range(rows - 1):
        step = (1, 1 << width)[i] if i < 2 else rnd.randrange(1, (1 << width) + 1)
        out.append((out[-1] + step) % R)
    return out


def columns_at_4_4(rows):
    """(name, ids, satisfied, over) at (max_bits, acc_cols) = (4, 4): B = 16.  The verdicts are written by hand: a gap d = id[i+1] -
    id[i] - 1 fits 16 bits exactly when the ids are 1 .. 2^16 apart."""
    good = ascending(rows, 16, seed=rows)
    cases = [("ascending", good, True, 0)]
    if rows >= 2:
        dup = list(good)
        dup[rows - 1] = dup[rows - 2]
        cases.append(("duplicate", dup, False, 1))
        swap = list(good)
        swap[0], swap[1] = swap[1], swap[0]
        # rows 0 | 1: the first gap is negative; the second, from the smaller id to id[2], is 1 + 2^16 at rows >= 3: too wide as well
        cases.append(("swapped", swap, False, 1 if rows == 2 else 2))
        base = 12345
        cases.append(("gap 2^16 + 1", [base] + ascending(rows - 1, 16, seed=7, start=base + (1 << 16) + 1), False, 1))
        cases.append(("gap 2^16", [base] + ascending(rows - 1, 16, seed=7, start=base + (1 << 16)), True, 0))
    if rows >= 4:
        wrap = [R - 2, R - 1, 0, 1] + ascending(rows - 3, 16, seed=9, start=1)[1:]
        cases.append(("wraps mod r", wrap, True, 0))
    return cases


def verify(lay, cs, adv):
    return yardstick.verify(cs, lay.fixed_columns(), adv, [[0] * lay.n], lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS)


def host_ids(max_bits, acc_cols, rows, seed):
    """ids for the word-for-word comparisons: 0, r - 1, equal neighbours, a descending pair, gaps of exactly 2^B and 2^B + 1, then
    ascending runs with random gaps below 2^B broken by random elements"""
    B = max_bits * acc_cols
    rnd = random.Random(seed)
    out = [R - 1, 0, 5, 5, 9, 3, 3 + (1 << B), 3 + (1 << B) + (1 << B) + 1]
    while len(out) < rows:
        out.append(rnd.randrange(R) if len(out) % 16 == 0 else (out[-1] + rnd.randrange(1, 1 << B)) % R)
    return out[:rows]


# ---- the mutation sweep: (4, 4), k = 5, rows = 5 -----------------------------------------------------------------------------------------
SWEEP_ROWS = 5
DELTAS = {"one": 1, "random": random.Random(0x50A7ED).randrange(1 << 200, R)}


def sweep_case():
    cs, lay = circuits.sorted_column(4, 4), sy.SortedColumnLayout(5, 4, 4, SWEEP_ROWS)
    # gaps (d = id[i+1] - id[i] - 1): 0xF3AF, 0x0000, 0x1F0F, 0x8421 -- limbs of 15, where +1 leaves the table, and of 0
    ids = [1000]
    for d in (0xF3AF, 0x0000, 0x1F0F, 0x8421):
        ids.append(ids[-1] + d + 1)
    adv = lay.assign_ints(ids)
    n, usable = lay.n, lay.n - (cs.blinding_factors + 1)
    fixed, inst = lay.fixed_columns(), [[0] * n]
    assert yardstick.verify(cs, fixed, adv, inst, lay.copies(), n, usable) == []
    return SimpleNamespace(name="sorted_column", cs=cs, lay=lay, k=5, n=n, usable=usable, advice=adv, instance=inst, inst_rows=0,
                           proof_instance=[[]], fixed=fixed, copies=lay.copies(), ids=ids,
                           tables=yardstick.lookup_tables(cs, fixed, adv, inst, n, usable))


# Written by hand, from the gate and the layout, not computed from the constraint system.  (column, row) -> the number of gate rows
# that fail when that cell changes, whatever the delta:
#   the id column: id[i] is read by the gate of row i (as "this id") and of row i - 1 (as "next id"); the selector is on rows 0 .. 3,
#   so id[0] fails 1 row, id[1] .. id[3] fail 2, id[4] (the last live row: read by row 3 only) fails 1, id[5] and behind none;
#   the limb columns: limb[j][i] is read by the gate of row i alone: rows 0 .. 3 fail 1, row 4 (no selector) and behind none.
EXPECTED_GATE_ROWS = {(0, 0): 1, (0, 1): 2, (0, 2): 2, (0, 3): 2, (0, 4): 1}
EXPECTED_GATE_ROWS.update({(col, row): 1 for col in (1, 2, 3, 4) for row in range(4)})
# the lookups carry no selector: every usable row (0 .. 25) of a limb column is range-checked.  A random element always leaves the
# table; plus 1 leaves it only from 15: the limbs of 0xF3AF, 0x0000, 0x1F0F, 0x8421, most significant first, on rows 0 .. 3
EXPECTED_LOOKUP_ONE = {(1, 0), (4, 0), (2, 2), (4, 2)}
EXPECTED_LOOKUP_RANDOM = {(col, row) for col in (1, 2, 3, 4) for row in range(26)}
