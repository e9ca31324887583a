"""Helper of tests/test_safe_accumulator.py and tests/test_safe_accumulator_gpu.py: the shapes and the carry patterns a SafeAccumulator
witness is tried on, and the plain big-integer accumulation the layout's ``assign_ints`` is held against."""
import random

from halo2_experiments_amd.domain import FR_MODULUS as R

# (max_bits, acc_cols): the reference's shape; small, degree 5; the smallest; an odd limb width; the full 64-bit budget
SHAPES = [(4, 4), (2, 3), (1, 2), (3, 5), (4, 16)]
PATTERNS = ("zeros", "max", "ripple", "overflow", "random", "wrap")
# the index of a polynomial inside "accumulation constraint" (circuits.safe_accumulator's docstring gives the order)
GATE = "accumulation constraint"


def poly_index(acc_cols, what, limb=0):
    return {"add": 0, "value_range": 1, "limb": 2 + limb, "overflow": 1 + acc_cols, "prev_range": 2 + acc_cols + limb,
            "cur_range": 2 + 2 * acc_cols + limb}[what]


def limbs_of(s, b, A):
    out = []
    for _ in range(A):
        s, low = divmod(s, 1 << b)
        out.append(low)
    return out[::-1]


def pattern(name, b, A, rows, at=None, seed=0):
    """-> (initial limbs, values).  ``at`` (1 .. rows) is the row whose value 1 starts the carry chain of "ripple" / "overflow" /
    "wrap": the state on row at - 1 is 0x00ff..f, 0x0fff..f or 2^W - 1, reached from the initial limbs through seeded values below 2^b
    on the rows before (as many of them non-zero as the target allows); the rows after ``at`` add seeded values too."""
    rng = random.Random(seed * 7919 + b * 100 + A)
    W, top = b * A, (1 << b) - 1
    if name == "zeros":
        return [0] + [rng.randrange(top + 1) for _ in range(A - 1)], [0] * rows
    if name == "max":
        return [0] * A, [top] * rows
    if name == "random":
        return [0] + [rng.randrange(top + 1) for _ in range(A - 1)], [rng.randrange(top + 1) for _ in range(rows)]
    target = {"ripple": (1 << (b * (A - 2))) - 1, "overflow": (1 << (b * (A - 1))) - 1, "wrap": (1 << W) - 1}[name]
    at = rows if at is None else at
    assert 1 <= at <= rows
    before, room = [], target
    for _ in range(at - 1):
        v = min(rng.randrange(top + 1), room)
        before.append(v)
        room -= v
    # after a legal ripple the rows that follow go on adding where that cannot reach the top limb; otherwise they add zero
    fits = name == "ripple" and (rows - at) * top < (1 << (b * (A - 1))) - (1 << (b * (A - 2)))
    after = [rng.randrange(top + 1) if fits else 0 for _ in range(rows - at)]
    return limbs_of(room, b, A), before + [1] + after


def accumulate(b, A, initial, values):
    """The plain big-integer accumulation: per row r >= 1 -> (S_r, the carry out of every limb position when the value is below 2^b,
    else None).  The carry out of position i is whether the low b (A - i) bits of S_(r-1) plus the value reach 2^(b (A - i)): one
    comparison of integers per position, no ripple."""
    W = b * A
    s = sum(int(x) << (b * (A - 1 - i)) for i, x in enumerate(initial)) % (1 << W)
    out = []
    for v in values:
        v = int(v) % R
        carries = None
        if v < 1 << b:
            carries = [0] + [int((s % (1 << (b * (A - i)))) + v >= 1 << (b * (A - i))) for i in range(1, A)]
        s = (s + v) % (1 << W)
        out.append((s, carries))
    return out


def satisfied(b, A, initial, values):
    """what the issue states: every value and initial limb below 2^b, the top limb 0 on every row"""
    if any(int(x) >> b for x in initial) or any(int(v) % R >> b for v in values) or initial[0]:
        return False
    return all(s >> (b * (A - 1)) == 0 for s, _ in accumulate(b, A, initial, values))


def numpy_columns(b, A, initial, values, n):
    """``SafeAccumulatorLayout.assign_ints`` as Montgomery words for values below 2^b and initial limbs below 2^b, by numpy on wrapping
    64-bit integers: for row counts where the integer twin and its conversion would take many seconds.  tests/test_safe_accumulator.py
    holds it against assign_ints.  values: (rows,) uint64 -> (2 + 2 A, n, 4) uint64"""
    import numpy as np
    from halo2_experiments_amd import poseidon as ps

    top = (1 << b) - 1
    assert values.dtype == np.uint64 and int(values.max()) <= top and all(0 <= int(x) <= top for x in initial)
    small = ps.ints_to_words(list(range(top + 2)))                                   # carries and limbs: 0 .. 2^b
    inverse = ps.ints_to_words([0] + [pow(j, R - 2, R) for j in range(1, top + 1)])
    rows, mask = len(values), np.uint64(top)
    wmask = np.uint64((1 << (b * A)) - 1)
    s0 = np.uint64(sum(int(x) << (b * (A - 1 - i)) for i, x in enumerate(initial)) & int(wmask))
    with np.errstate(over="ignore"):
        s = (s0 + np.cumsum(values, dtype=np.uint64)) & wmask
    prev = np.concatenate([np.array([s0], dtype=np.uint64), s[:-1]])
    cols = np.zeros((2 + 2 * A, n, 4), dtype=np.uint64)
    cols[0, 1:rows + 1] = small[values.astype(np.int64)]
    carry = None
    for j in range(A - 1, -1, -1):
        shift = np.uint64(b * (A - 1 - j))
        p, c = (prev >> shift) & mask, (s >> shift) & mask
        carry = (p + values) >> np.uint64(b) if j == A - 1 else (p + carry) >> np.uint64(b) if j else np.zeros(rows, dtype=np.uint64)
        cols[2 + j, 1:rows + 1] = small[carry.astype(np.int64)]
        cols[2 + A + j, 1:rows + 1] = small[c.astype(np.int64)]
        cols[2 + A + j, 0] = small[int(initial[j])]
        if j == 0:
            cols[1, 1:rows + 1] = inverse[c.astype(np.int64)]
    finals = [int((s[-1] >> np.uint64(b * (A - 1 - i))) & mask) for i in range(A)]
    over = int(np.count_nonzero((s >> np.uint64(b * (A - 1))) & mask)) + int(initial[0] != 0)
    return cols, finals, over
