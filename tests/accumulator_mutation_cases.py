"""The mutation sweep's SafeAccumulator case (tests/test_mutation_sweep_accumulator.py, tests/test_mutation_sweep_accumulator_gpu.py), on
the helpers of tests/mutation_cases.py: SafeAccumulator<2, 3> at k = 5 with three values, a satisfied witness built from integers alone,
and ``EXPECTED``: which cells the circuit constrains, written down by hand from the reference's chip -- NOT computed from the constraint
system.  DESIGN.md section 26 says why each free cell is free."""
from halo2_experiments_amd import circuits, synthesis as sy

import mutation_cases as mc

NAME = "safe_accumulator"
B, A, K, ROWS = 2, 3, 5, 3
INITIAL, VALUES = [0, 1, 3], [1, 3, 2]                       # 7 -> 8 (a carry out of the low limb) -> 11 -> 13: the top limb stays 0
VALUE, INV, CARRIES, ACC = 0, 1, (2, 3, 4), (5, 6, 7)

# (advice columns, rows, caught by: g a gate / c a copy, where the reference assigns or constrains the cell)
EXPECTED = [
    (ACC, (0,), "g", "chips/safe_accumulator.rs:204-211 the previous limbs; row 1 reads them at Rotation::prev (:82-84): the add-value and "
                     "limb polynomials and the range checks of :158"),
    (ACC, (1, 2), "g", "chips/safe_accumulator.rs:247-252 the updated limbs; the polynomials of their own row (:88-90, :159) and, as the "
                       "previous limbs, of the next"),
    (ACC, (3,), "gc", "the last row's limbs: the same gates, and expose_public (circuits/safe_accumulator.rs:85-87) copies each to the instance"),
    ((VALUE,), (1, 2, 3), "g", "chips/safe_accumulator.rs:196-201 the value; the add-value polynomial :112-117 and its range check :118"),
    (CARRIES, (1, 2, 3), "g", "chips/safe_accumulator.rs:226-231 the carries; add_carries[A-1] in the add-value polynomial, every other one in "
                              "two limb polynomials (:141-148) -- add_carries[0], which the chip always assigns 0, in the top limb's"),
]
# free: left_most_inv on every row (the top limb is 0 on every row of a satisfied witness, so acc[0] * (1 - acc[0] * inv) and
# acc[0] * inv vanish whatever inv is: is_zero.rs:36-41 "yes | 0 | y"); everything on row 0 outside the accumulate columns (no selector
# on row 0); every row above ROWS.
N_CONSTRAINED, N_CELLS = 24, 8 * 32


def build():
    cs, lay = circuits.safe_accumulator(B, A), sy.SafeAccumulatorLayout(K, B, A, ROWS)
    lay.check_constraint_system(cs)
    adv = lay.assign_ints(INITIAL, VALUES)
    inst = lay.instance(INITIAL, VALUES)
    assert inst == [[0, 3, 1]]
    c = mc._case(NAME, cs, lay, adv, inst, A, list(inst[0]))
    assert mc.yardstick.verify(cs, c.fixed, adv, c.instance, c.copies, c.n, c.usable) == []
    return c


_CASE = []


def case():
    if not _CASE:
        _CASE.append(build())
    return _CASE[0]


def cells(c):
    """every advice cell, as (column, row)"""
    return [(col, row) for row in range(c.n) for col in range(c.cs.num_advice)]


def expected_sets():
    out = {"gate": set(), "copy": set()}
    for columns, rows, letters, _ in EXPECTED:
        for letter in letters:
            out[mc.LETTER[letter]] |= {(col, row) for col in columns for row in rows}
    out["constrained"] = out["gate"] | out["copy"]
    return out


_VERDICTS = {}


def verdicts(delta_name):
    if delta_name not in _VERDICTS:
        c = case()
        _VERDICTS[delta_name] = (cells(c), mc.host_verdicts(c, cells(c), mc.DELTAS[delta_name]))
    return _VERDICTS[delta_name]


def unsound_witness():
    """The second deviation, by hand: from the state [0, 0, 1] the value 1 "gives" [0, 0, 3] (1 + 1 = 3) with the carries
    c[2] = (1 + 1 - 3) / 4, c[1] = c[2] / 4, c[0] = c[1] / 4 -- field elements that balance every accumulation polynomial.  Only
    "bool constraint" rejects them.  -> (layout, advice, instance)"""
    from halo2_experiments_amd.domain import FR_MODULUS as R

    lay = sy.SafeAccumulatorLayout(K, B, A, 1)
    adv = lay.assign_ints([0, 0, 1], [1])
    quarter = pow(4, R - 2, R)
    c2 = (1 + 1 - 3) * quarter % R
    c1 = c2 * quarter % R
    c0 = c1 * quarter % R
    for col, v in zip(CARRIES, (c0, c1, c2)):
        adv[col][1] = v
    for col, v in zip(ACC, (0, 0, 3)):
        adv[col][1] = v
    return lay, adv, [[0, 0, 3]]
