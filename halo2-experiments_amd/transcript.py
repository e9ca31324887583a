"""``halo2_proofs::transcript``: ``Blake2bWrite`` / ``Blake2bRead`` with ``Challenge255`` over BN256 G1, on host integers.

RECALLED from upstream (tag v2023_02_02), item by item; nothing here is pinned against upstream's bytes:
  - the hash is Blake2b with a 64-byte digest and the personalisation ``b"Halo2-Transcript"`` (RECALLED);
  - every absorption is preceded by a one-byte prefix: 0 before a challenge is squeezed, 1 before a point, 2 before a scalar (RECALLED);
  - a point is absorbed as its affine x then y, 32 bytes little-endian canonical each, and WRITTEN compressed: x little-endian with
    bit 7 of byte 31 = the parity of y, the encoding of ``g1_compress_host`` (RECALLED; the identity cannot be absorbed upstream and is
    refused here too);
  - a scalar is absorbed and written as its 32 canonical bytes little-endian (RECALLED);
  - a challenge: the prefix byte 0 is absorbed into the running state, a COPY of the state is finalised, and the 64 digest bytes,
    read as a little-endian integer, are reduced mod r (``Challenge255`` / ``from_bytes_wide``; RECALLED).  The running state keeps the
    prefix byte, so two squeezes in a row differ.

Points are (x, y) tuples of integers, as in ``pairing``."""
from __future__ import annotations

import hashlib

from .bn256 import FQ_MODULUS, FR_MODULUS

PREFIX_CHALLENGE, PREFIX_POINT, PREFIX_SCALAR = b"\x00", b"\x01", b"\x02"
PERSONAL = b"Halo2-Transcript"
_P, _R = FQ_MODULUS, FR_MODULUS


class TranscriptError(ValueError):
    """A short read, bytes that are no curve point, or a scalar that is not below r."""


def g1_compress_int(p) -> bytes:
    if p is None:
        return bytes(32)
    x, y = p
    return (x | ((y & 1) << 255)).to_bytes(32, "little")


def g1_decompress_int(data: bytes):
    """The point of 32 compressed bytes; raises TranscriptError when x is not canonical or not the x of a curve point.  All-zero
    bytes are the identity (None)."""
    if len(data) != 32:
        raise TranscriptError("a point takes 32 bytes")
    v = int.from_bytes(data, "little")
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if v == 0:
        return None
    if x >= _P:
        raise TranscriptError("point: x is not canonical")
    y = pow((x * x * x + 3) % _P, (_P + 1) // 4, _P)              # p = 3 mod 4
    if (y * y - x * x * x - 3) % _P:
        raise TranscriptError("point: x is not on the curve")
    if y & 1 != sign:
        y = _P - y
    return (x, y)


class _Transcript:
    def __init__(self):
        self._state = hashlib.blake2b(digest_size=64, person=PERSONAL)

    def common_point(self, p) -> None:
        if p is None:
            raise TranscriptError("cannot absorb the identity")
        self._state.update(PREFIX_POINT + (p[0] % _P).to_bytes(32, "little") + (p[1] % _P).to_bytes(32, "little"))

    def common_scalar(self, s: int) -> None:
        self._state.update(PREFIX_SCALAR + (s % _R).to_bytes(32, "little"))

    def squeeze_challenge(self) -> int:
        self._state.update(PREFIX_CHALLENGE)
        return int.from_bytes(self._state.copy().digest(), "little") % _R


class Blake2bWrite(_Transcript):
    def __init__(self):
        super().__init__()
        self._out = bytearray()

    def write_point(self, p) -> None:
        self.common_point(p)
        self._out += g1_compress_int(p)

    def write_scalar(self, s: int) -> None:
        self.common_scalar(s)
        self._out += (s % _R).to_bytes(32, "little")

    def finalize(self) -> bytes:
        return bytes(self._out)


class Blake2bRead(_Transcript):
    def __init__(self, proof: bytes):
        super().__init__()
        self._data, self._at = bytes(proof), 0

    def _take(self) -> bytes:
        if self._at + 32 > len(self._data):
            raise TranscriptError("the proof ends early")
        self._at += 32
        return self._data[self._at - 32:self._at]

    def read_point(self):
        p = g1_decompress_int(self._take())
        self.common_point(p)
        return p

    def read_scalar(self) -> int:
        s = int.from_bytes(self._take(), "little")
        if s >= _R:
            raise TranscriptError("scalar: not below r")
        self.common_scalar(s)
        return s

    def remaining(self) -> int:
        return len(self._data) - self._at
