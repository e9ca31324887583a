"""Helper of tests/test_range_check.py and tests/test_range_check_gpu.py: the values a range-check witness is tried on."""
import random

from halo2_experiments_amd.domain import FR_MODULUS as R


def values(max_bits, acc_cols, rows, seed):
    """0, 2^bits - 1, 2^bits, r - 1, a single bit at every 64-bit word boundary (both sides), then seeded random values below 2^bits
    and below r -- `rows` of them"""
    bits = max_bits * acc_cols
    rnd = random.Random(seed)
    out = [0, (1 << bits) - 1, (1 << bits) % R, R - 1]
    for b in (63, 64, 127, 128, 191, 192):
        out += [1 << b, (1 << b) | 1]
    while len(out) < rows:
        out.append(rnd.randrange(1 << bits) if len(out) % 2 else rnd.randrange(R))
    return out[:rows]
