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

Points are (x, y) tuples of integers, as in ``pairing``.

The second encoding, ``encoding="evm"``: ``KeccakWrite`` / ``KeccakRead``, what a Solidity verifier reads.  RECALLED from
snark-verifier's ``EvmTranscript<_, NativeLoader, _, _>``, item by item; snark-verifier is not at hand and nothing here is pinned
against its bytes:
  - the state is a byte buffer ``buf``, empty at the start (RECALLED);
  - ``common_scalar(s)`` appends the 32 canonical bytes of s, big-endian (RECALLED);
  - ``common_point(P)`` appends x then y, 32 canonical bytes each, big-endian; the identity cannot be absorbed and is refused (RECALLED);
  - ``write_point`` absorbs the point and writes the same 64 bytes to the proof, ``write_scalar`` absorbs the scalar and writes the
    same 32 bytes: a proof is absorbed verbatim, and its length is 64 per point + 32 per scalar (RECALLED);
  - reading refuses a coordinate >= p, a point off y^2 = x^3 + 3 -- the 64 zero bytes fall under this rule -- and a scalar >= r
    (RECALLED);
  - ``squeeze_challenge``: data = buf, with one byte 0x01 appended if and only if len(buf) == 32; h = keccak256(data); buf = h; the
    challenge is h read as a big-endian integer, reduced mod r.  Two squeezes in a row differ, and every later hash chains the
    previous digest (RECALLED);
  - ``keccak256`` is Keccak-f[1600] with rate 136, the padding's domain byte 0x01 (not SHA-3's 0x06) and a 32-byte output (RECALLED;
    the permutation and the padding are held to ``hashlib.sha3_256`` through the domain byte, tests/test_keccak_host.py);
  - the preamble is the other encoding's: the digest of the verifying key (the Blake2b-derived integer it is), then the instance
    values, absorbed as scalars (RECALLED)."""
from __future__ import annotations

import hashlib

from .bn256 import FQ_MODULUS, FR_MODULUS

PREFIX_CHALLENGE, PREFIX_POINT, PREFIX_SCALAR = b"\x00", b"\x01", b"\x02"
PERSONAL = b"Halo2-Transcript"
_P, _R = FQ_MODULUS, FR_MODULUS


ENCODINGS = ("halo2", "evm")


def check_encoding(encoding, who: str) -> str:
    """``encoding`` when it names one of ``ENCODINGS``; ValueError otherwise, before any other work of ``who``"""
    if encoding not in ENCODINGS:
        raise ValueError(f"{who}: encoding must be one of {ENCODINGS}, got {encoding!r}")
    return encoding


MULTIOPENS = ("shplonk", "gwc")


def check_multiopen(multiopen, who: str) -> str:
    """``multiopen`` when it names one of ``MULTIOPENS``; ValueError otherwise, before any other work of ``who``"""
    if multiopen not in MULTIOPENS:
        raise ValueError(f"{who}: multiopen must be one of {MULTIOPENS}, got {multiopen!r}")
    return multiopen


LOOKUPS = ("halo2", "logup")


def check_lookup(lookup, who: str) -> str:
    """``lookup`` when it names one of ``LOOKUPS`` -- "halo2", the permutation-based lookup argument, or "logup", the
    logarithmic-derivative one; ValueError otherwise, before any other work of ``who``"""
    if lookup not in LOOKUPS:
        raise ValueError(f"{who}: lookup must be one of {LOOKUPS}, got {lookup!r}")
    return lookup


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


# ---- the EVM encoding ------------------------------------------------------------------------------------------------------------------
_KECCAK_RC = []
_KECCAK_ROT = [[0] * 5 for _ in range(5)]                        # [x][y]


def _keccak_tables() -> None:
    lfsr = 1
    for _ in range(24):                                          # the round constants: bit 2^j - 1 from the degree-8 LFSR
        rc = 0
        for j in range(7):
            if lfsr & 1:
                rc |= 1 << ((1 << j) - 1)
            lfsr = (lfsr << 1) ^ (0x171 if lfsr & 0x80 else 0)
        _KECCAK_RC.append(rc)
    x, y = 1, 0
    for t in range(24):                                          # the rotation offsets: (t + 1)(t + 2) / 2 along (x, y) -> (y, 2x + 3y)
        _KECCAK_ROT[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5


_keccak_tables()
_M64 = (1 << 64) - 1
KECCAK_RATE = 136


# rho and pi as one table: (source lane, its column, destination lane, left rotation, 64 - rotation)
_KECCAK_MOVES = [(x + 5 * y, x, y + 5 * ((2 * x + 3 * y) % 5), _KECCAK_ROT[x][y], 64 - _KECCAK_ROT[x][y]) for y in range(5) for x in range(5)]


def _keccak_f1600(a: list) -> None:
    """Keccak-f[1600] on 25 lanes of 64 bits, lane (x, y) at a[x + 5 y], in place"""
    m64, moves = _M64, _KECCAK_MOVES
    b = [0] * 25
    for rc in _KECCAK_RC:
        c0, c1, c2 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20], a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21], a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22]
        c3, c4 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23], a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24]
        d = (c4 ^ ((c1 << 1) & m64 | c1 >> 63), c0 ^ ((c2 << 1) & m64 | c2 >> 63), c1 ^ ((c3 << 1) & m64 | c3 >> 63),
             c2 ^ ((c4 << 1) & m64 | c4 >> 63), c3 ^ ((c0 << 1) & m64 | c0 >> 63))
        for src, x, dst, left, right in moves:
            v = a[src] ^ d[x]
            b[dst] = (v << left) & m64 | v >> right                # left = 0: v | v >> 64 = v
        for y in (0, 5, 10, 15, 20):
            b0, b1, b2, b3, b4 = b[y], b[y + 1], b[y + 2], b[y + 3], b[y + 4]
            a[y], a[y + 1], a[y + 2] = b0 ^ (~b1 & b2) & m64, b1 ^ (~b2 & b3) & m64, b2 ^ (~b3 & b4) & m64
            a[y + 3], a[y + 4] = b3 ^ (~b4 & b0) & m64, b4 ^ (~b0 & b1) & m64
        a[0] ^= rc


def keccak256(data: bytes, domain: int = 0x01) -> bytes:
    """Keccak with rate 136 and a 32-byte output: ``domain`` is the byte the padding starts with -- 0x01 is Keccak-256 as Ethereum
    uses it (the default), 0x06 gives ``hashlib.sha3_256``."""
    if not 0 < domain < 0x80:
        raise ValueError("keccak256: the domain byte must lie in 1 .. 127")
    data = bytes(data)
    pad = KECCAK_RATE - len(data) % KECCAK_RATE
    tail = bytearray(pad)
    tail[0] = domain
    tail[-1] |= 0x80                                             # pad == 1: the two bytes merge
    data += bytes(tail)
    a = [0] * 25
    for at in range(0, len(data), KECCAK_RATE):
        for i in range(KECCAK_RATE // 8):
            a[i] ^= int.from_bytes(data[at + 8 * i:at + 8 * i + 8], "little")
        _keccak_f1600(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def g1_uncompressed_int(data: bytes):
    """The point of 64 bytes, x then y big-endian; raises TranscriptError when a coordinate is not canonical or the point is off the
    curve, which the 64 zero bytes are."""
    if len(data) != 64:
        raise TranscriptError("a point takes 64 bytes")
    x, y = int.from_bytes(data[:32], "big"), int.from_bytes(data[32:], "big")
    if x >= _P or y >= _P:
        raise TranscriptError("point: a coordinate is not canonical")
    if (y * y - x * x * x - 3) % _P:
        raise TranscriptError("point: not on the curve")
    return (x, y)


class _KeccakTranscript:
    def __init__(self):
        self._buf = bytearray()

    def common_point(self, p) -> None:
        if p is None:
            raise TranscriptError("cannot absorb the identity")
        self._buf += (p[0] % _P).to_bytes(32, "big") + (p[1] % _P).to_bytes(32, "big")

    def common_scalar(self, s: int) -> None:
        self._buf += (s % _R).to_bytes(32, "big")

    def squeeze_challenge(self) -> int:
        data = bytes(self._buf) + (b"\x01" if len(self._buf) == 32 else b"")
        h = keccak256(data)
        self._buf = bytearray(h)
        return int.from_bytes(h, "big") % _R


class KeccakWrite(_KeccakTranscript):
    def __init__(self):
        super().__init__()
        self._out = bytearray()

    def write_point(self, p) -> None:
        self.common_point(p)
        self._out += self._buf[-64:]

    def write_scalar(self, s: int) -> None:
        self.common_scalar(s)
        self._out += self._buf[-32:]

    def finalize(self) -> bytes:
        return bytes(self._out)


class KeccakRead(_KeccakTranscript):
    def __init__(self, proof: bytes):
        super().__init__()
        self._data, self._at = bytes(proof), 0

    def _take(self, size: int) -> bytes:
        if self._at + size > len(self._data):
            raise TranscriptError("the proof ends early")
        self._at += size
        return self._data[self._at - size:self._at]

    def read_point(self):
        p = g1_uncompressed_int(self._take(64))
        self.common_point(p)
        return p

    def read_scalar(self) -> int:
        s = int.from_bytes(self._take(32), "big")
        if s >= _R:
            raise TranscriptError("scalar: not below r")
        self.common_scalar(s)
        return s

    def remaining(self) -> int:
        return len(self._data) - self._at


WRITERS = {"halo2": Blake2bWrite, "evm": KeccakWrite}
READERS = {"halo2": Blake2bRead, "evm": KeccakRead}
