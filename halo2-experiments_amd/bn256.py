"""BN256 on the host: the constants of the two fields and the one statement of the data format of the C ABI -- a field element is
4 x u64 little-endian words of v * 2^256 mod p (Montgomery form, fully reduced: the bytes Rust's ``Fr`` / ``Fq`` hold), a G1Affine
is x then y (8 words, (0, 0) = the identity), a G1 adds z (12 words, z = 0: the identity).

Python integers and numpy only: nothing here loads the library or touches a GPU.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FQ_MODULUS = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
FR_S = 28
FR_GENERATOR = 7
FR_ROOT_OF_UNITY = pow(FR_GENERATOR, (FR_MODULUS - 1) >> FR_S, FR_MODULUS)
FR_ZETA = 0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23

_RADIX = 1 << 256
FR_RADIX = _RADIX % FR_MODULUS            # multiplying by it takes canonical words to Montgomery words
_FR_RINV = pow(_RADIX, -1, FR_MODULUS)
_FQ_RINV = pow(_RADIX, -1, FQ_MODULUS)


def _words(v: int, p: int) -> np.ndarray:
    m = (v % p) * _RADIX % p
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _array(values, p: int) -> np.ndarray:
    a = np.asarray(values, dtype=object)
    raw = b"".join((int(v) % p * _RADIX % p).to_bytes(32, "little") for v in a.reshape(-1))
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64).reshape(a.shape + (4,))


def _ints(words, p: int, rinv: int) -> List[int]:
    w = np.ascontiguousarray(np.asarray(words).view(np.uint64).reshape(-1, 4))
    return [int.from_bytes(row.tobytes(), "little") * rinv % p for row in w]


def fr_words(v: int) -> np.ndarray:
    """Canonical integer -> 4 Montgomery limbs (the bytes Rust's ``Fr`` holds)."""
    return _words(v, FR_MODULUS)


def fq_words(v: int) -> np.ndarray:
    """Canonical integer -> 4 Montgomery limbs of Fq (the bytes Rust's ``Fq`` holds)."""
    return _words(v, FQ_MODULUS)


def fr_array(values) -> np.ndarray:
    """Canonical integers of any nesting (shape s) -> s + (4,) uint64 Montgomery words of Fr"""
    return _array(values, FR_MODULUS)


def fq_array(values) -> np.ndarray:
    return _array(values, FQ_MODULUS)


def fr_ints(words) -> List[int]:
    """(..., 4) 64-bit Montgomery words of Fr -> canonical integers, flattened."""
    return _ints(words, FR_MODULUS, _FR_RINV)


def fq_ints(words) -> List[int]:
    return _ints(words, FQ_MODULUS, _FQ_RINV)


def fr_int(words) -> int:
    return fr_ints(words)[0]


def fq_int(words) -> int:
    return fq_ints(words)[0]


def g1_words(point: Optional[Tuple[int, int]]) -> np.ndarray:
    """(x, y) integers -> the 8 words of a G1Affine; None (the identity) -> (0, 0)"""
    return np.zeros(8, dtype=np.uint64) if point is None else fq_array(point).reshape(8)


def g1_ints(words) -> Optional[Tuple[int, int]]:
    """(x, y) integers of 12 (or 8) Montgomery words of a normalised G1; None for the identity (all-zero z, or (0, 0))"""
    w = np.asarray(words, dtype=np.uint64).reshape(-1)
    if len(w) == 12 and not w[8:].any():
        return None
    x, y = fq_ints(w[:8])
    return None if (x, y) == (0, 0) else (x, y)


# Montgomery one of Fq (2^256 mod p): the z coordinate of a normalised G1
FQ_ONE_MONT = fq_words(1)
# bn256::G1Affine::generator() = (1, 2)
G1_GENERATOR = g1_words((1, 2))
