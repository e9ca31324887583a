"""The pure-integer twin of the logUp argument's two columns, the oracle of tests/test_logup_host.py and
tests/test_logup_gpu.py: the multiplicity column m and the running sum phi of ONE argument with compressed table t and compressed
inputs f_1 .. f_c on the usable rows 0 .. u - 1, and the argument's third polynomial on a row.  Python integers mod r, no device, no
library of the project but the modulus."""
from halo2_experiments_amd.domain import FR_MODULUS as R


def multiplicities(table, inputs):
    """m[i] = the number of (j, row) with inputs[j][row] == table[i] if i is the first row of the table holding that value, else 0;
    -> (m, missing): missing is True when some input value is not in the table"""
    first = {}
    for i, v in enumerate(table):
        first.setdefault(v % R, i)
    m, missing = [0] * len(table), False
    for f in inputs:
        for v in f:
            if v % R in first:
                m[first[v % R]] += 1
            else:
                missing = True
    return m, missing


def inverse(v):
    return pow(v, -1, R) if v % R else 0                       # batch_invert leaves a zero denominator zero


def running_sum(table, inputs, m, beta):
    """phi[0] = 0, phi[i + 1] = phi[i] + sum_j 1 / (f_j[i] + beta) - m[i] / (t[i] + beta): u + 1 values"""
    phi = [0]
    for i, t in enumerate(table):
        term = sum(inverse(f[i] + beta) for f in inputs) - m[i] * inverse(t + beta)
        phi.append((phi[-1] + term) % R)
    return phi


def prefix_sums(terms):
    """out[i] = sum_{j < i} terms[j] mod r: what grand_sum_batch computes on one column"""
    out, run = [], 0
    for v in terms:
        out.append(run)
        run = (run + v) % R
    return out


def third_polynomial(table, inputs, m, phi, beta, i):
    """(phi[i+1] - phi[i]) (t + beta) prod_j (f_j + beta) - ((t + beta) sum_j prod_{l != j} (f_l + beta) - m prod_j (f_j + beta)) on row i"""
    t = (table[i] + beta) % R
    f = [(col[i] + beta) % R for col in inputs]
    prod = 1
    for v in f:
        prod = prod * v % R
    others = 0
    for j in range(len(f)):
        term = 1
        for l, v in enumerate(f):
            if l != j:
                term = term * v % R
        others = (others + term) % R
    return ((phi[i + 1] - phi[i]) * t * prod - (t * others - m[i] * prod)) % R


# ---- the shapes both the host twins (under bound tracking) and the kernels are held to -------------------------------------------------
import random

SCAN_ROWS = 256                                     # csrc/logup.inc LU_SCAN_ROWS: the rows one workgroup of the scan covers
COUNT_BITS = 20                                     # csrc/logup.inc LU_COUNT_BITS: table keys below 2^this are counted in value bins
GRAND_SUM_LENGTHS = [1, 2, 63, 64, 65, SCAN_ROWS - 1, SCAN_ROWS, SCAN_ROWS + 1, 2 * SCAN_ROWS + 1,
                     65 * SCAN_ROWS + 1]            # the last: 66 block totals, so the middle launch carries between its waves
GRAND_SUM_VALUES = ["wrap", "zero", "random"]
MULTIPLICITY_ROWS = [1, 2, 64, 65, 26, 506]         # the last two are 2^5 - 6 and 2^9 - 6
MULTIPLICITY_TABLES = ["range", "hot", "below_switch", "at_switch", "wide"]


def grand_sum_columns(n, values, count, seed=0):
    rng = random.Random(1000 * n + 10 * count + seed)
    if values == "wrap":
        return [[R - 1] * n for _ in range(count)]            # every addition wraps
    if values == "zero":
        return [[0] * n for _ in range(count)]
    return [[rng.randrange(R) for _ in range(n)] for _ in range(count)]


def multiplicity_case(rows, c, kind, seed=0):
    """-> (table, inputs): `rows` table values, one of them repeated where rows allow, and c input columns drawn from the table.
    range: small values; hot: every input holds one value; below_switch / at_switch: the largest table key is 2^COUNT_BITS - 1 /
    2^COUNT_BITS (the value bins / the sorted records); wide: r - 1, random 254-bit values and a repeated one"""
    rng = random.Random(100000 * rows + 100 * c + MULTIPLICITY_TABLES.index(kind) + seed)
    at = 0 if rows == 2 else rows // 2                            # not the row the repeated value below is written to
    if kind == "wide":
        table = [rng.randrange(1 << 253, R) for _ in range(rows)]
        table[0] = R - 1
    else:
        table = [rng.randrange(min(rows, 251)) for _ in range(rows)]
        if kind == "below_switch":
            table[at] = (1 << COUNT_BITS) - 1
        if kind == "at_switch":
            table[at] = 1 << COUNT_BITS
    if rows >= 2:
        table[rows - 1] = table[rows // 3]                        # a repeated value: m stands on its first row
    inputs = [[rng.choice(table) for _ in range(rows)] for _ in range(c)]
    if kind == "hot":
        inputs = [[table[at]] * rows for _ in range(c)]
    if kind in ("below_switch", "at_switch"):
        inputs[0][0] = table[at]                           # the key at the switch is looked up
    return table, inputs
