"""Keccak-256 without a GPU: ``transcript.keccak256`` against ``hashlib.sha3_256`` through the domain byte -- the independent anchor of
the EVM encoding, whose rules are otherwise recalled -- and its two known answers; then the lane functions of csrc/keccak.inc, compiled
for the host with the bound tracking on (libhm_hostcheck.so), against the Python function: whole messages on the byte path and the word
path, the transcript's absorb / squeeze stream against a Python twin of the buffer rules, the big-endian reduction at its edges."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from halo2_experiments_amd import _lib
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fr_array, fr_ints
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.transcript import KECCAK_RATE, KeccakWrite, keccak256

u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
LENGTHS = (0, 1, 31, 32, 33, 135, 136, 137, 271, 272, 273, 1000)     # the block boundaries +- 1; at 135 the padding bytes merge into 0x81


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_keccak256.restype = None
    lib.hc_keccak256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p, ctypes.c_size_t, ctypes.c_uint32, u8p]
    lib.hc_keccak_stream.restype = None
    lib.hc_keccak_stream.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p, u8p, u32p]
    lib.hc_keccak_challenge.restype = None
    lib.hc_keccak_challenge.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p]
    return lib


def message(length: int, salt: int = 0) -> bytes:
    return bytes((7 * i + 13 * salt + (i >> 8)) & 0xFF for i in range(length))


# ---- the Python function ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS)
def test_permutation_and_padding_against_sha3(length):
    m = message(length, length)
    assert keccak256(m, domain=0x06) == hashlib.sha3_256(m).digest()
    assert keccak256(m) != keccak256(m, domain=0x06)                       # the domain byte is part of the hash


def test_known_answers_of_the_keccak_domain():
    assert keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert KECCAK_RATE == 136
    for bad in (0, 0x80, 0x100):
        with pytest.raises(ValueError, match="domain"):
            keccak256(b"", domain=bad)


# ---- the lane functions: whole messages ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [0x01, 0x06])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_whole_messages_against_the_python_function(hc, domain, shift):
    """every length of the list, the messages `shift` bytes off a word boundary: the byte path and the word path of the lane"""
    stride = 1004
    msgs = [message(n, n) for n in LENGTHS]
    raw = bytearray(shift + stride * len(msgs))
    for i, m in enumerate(msgs):
        raw[shift + i * stride:shift + i * stride + len(m)] = m
    buf = (ctypes.c_char * (len(raw) + 8)).from_buffer_copy(bytes(raw) + bytes(8))
    base = ctypes.addressof(buf)
    assert base % 4 == 0
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    out = np.zeros((len(msgs), 32), dtype=np.uint8)
    hc.hc_keccak256(ctypes.cast(base + shift, ctypes.c_char_p), stride, lens.ctypes.data_as(u32p), len(msgs), domain, out.ctypes.data_as(u8p))
    assert [bytes(row) for row in out] == [keccak256(m, domain) for m in msgs]
    if domain == 0x06:
        assert [bytes(row) for row in out] == [hashlib.sha3_256(m).digest() for m in msgs]


# ---- the transcript's stream ---------------------------------------------------------------------------------------------------------------------
def run_stream(hc, ops, data):
    """hc_keccak_stream: 1 a word of 32 bytes absorbed (8 words of data), 0 a squeeze -> (digests, the block position after each op)"""
    digests = np.zeros((ops.count(0), 32), dtype=np.uint8)
    positions = np.zeros(len(ops), dtype=np.uint32)
    hc.hc_keccak_stream(bytes(ops), len(ops), data.ctypes.data_as(u32p), digests.ctypes.data_as(u8p), positions.ctypes.data_as(u32p))
    return [bytes(row) for row in digests], positions.tolist()


def twin(ops, data):
    """the buffer rules of ``transcript`` on the same stream -> (digests, len(buf) at each squeeze, len(buf) % rate after each op)"""
    buf, at, digests, lengths, positions = bytearray(), 0, [], [], []
    for o in ops:
        if o:
            buf += data[at:at + 8].tobytes()
            at += 8
        else:
            lengths.append(len(buf))
            digests.append(keccak256(bytes(buf) + (b"\x01" if len(buf) == 32 else b"")))
            buf = bytearray(digests[-1])
        positions.append(len(buf) % KECCAK_RATE)
    return digests, lengths, positions


def stream_case(seed: int):
    """Opens on a lone word absorbed into the EMPTY buffer and a squeeze (32 bytes that do not follow a squeeze), then three more
    squeezes in a row, then 16 words behind the digest -- 17 * 32 bytes, 4 blocks exactly -- and a squeeze, then a random tail"""
    rng = random.Random(seed)
    return [1, 0, 0, 0, 0] + [1] * 16 + [0] + [rng.choice((0, 1, 1, 1)) for _ in range(90)] + [0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_stream_against_a_python_twin_of_the_buffer_rules(hc, seed):
    ops = stream_case(seed)
    data = np.random.default_rng(seed).integers(0, 1 << 32, size=8 * ops.count(1), dtype=np.uint64).astype(np.uint32)
    got, positions = run_stream(hc, ops, data)
    want, lengths, want_positions = twin(ops, data)
    assert got == want and positions == want_positions
    # what the stream must contain: the lone word, squeezes in a row (which differ), a squeeze that pads a block of its own
    assert ops[:2] == [1, 0] and lengths[:4] == [32, 32, 32, 32] and len(set(got[:4])) == 4
    assert lengths[4] == 4 * KECCAK_RATE and want_positions[20] == 0


def test_the_extra_byte_hangs_on_the_length_alone(hc):
    """18 words are 4 blocks and 32 bytes: the block position is 32 as behind a squeeze, the length is not, and no 0x01 is appended;
    a lone word in the empty buffer takes it, though no squeeze came before"""
    data = np.random.default_rng(9).integers(0, 1 << 32, size=8 * 18, dtype=np.uint64).astype(np.uint32)
    got, positions = run_stream(hc, [1] * 18 + [0], data)
    assert positions[17] == 32 and 18 * 32 == 4 * KECCAK_RATE + 32
    assert got[0] == keccak256(data.tobytes()) != keccak256(data.tobytes() + b"\x01")
    got, _ = run_stream(hc, [1, 0], data)
    assert got[0] == keccak256(data[:8].tobytes() + b"\x01") != keccak256(data[:8].tobytes())


def test_write_transcript_is_the_twin(hc):
    """``KeccakWrite`` on scalars and the stream on their big-endian bytes squeeze the same challenges"""
    rng = random.Random(4)
    t = KeccakWrite()
    ops, words, want = [], [], []
    for count in (1, 0, 3, 17, 2):
        for _ in range(count):
            s = rng.randrange(R)
            t.write_scalar(s)
            ops.append(1)
            words.append(s.to_bytes(32, "big"))
        want.append(t.squeeze_challenge())
        ops.append(0)
    digests, _ = run_stream(hc, ops, np.frombuffer(b"".join(words), dtype=np.uint32).copy())
    out = np.zeros((len(want), 8), dtype=np.uint32)
    hc.hc_keccak_challenge(b"".join(digests), len(want), out.ctypes.data_as(u32p))
    assert fr_ints(out.view(np.uint64)) == want
    assert t.finalize() == b"".join(words)


# ---- the reduction -------------------------------------------------------------------------------------------------------------------------------
def test_big_endian_reduction_against_the_integers(hc):
    rng = random.Random(5)
    cases = [R - 1, R, 2 ** 256 - 1, 0, P, 1, 2 * R, 2 ** 255] + [rng.getrandbits(256) for _ in range(64)]
    raw = b"".join(v.to_bytes(32, "big") for v in cases)
    out = np.zeros((len(cases), 8), dtype=np.uint32)
    hc.hc_keccak_challenge(raw, len(cases), out.ctypes.data_as(u32p))
    assert fr_ints(out.view(np.uint64)) == [v % R for v in cases]
    assert np.array_equal(out.view(np.uint64), fr_array([v % R for v in cases]))          # canonical Montgomery words, bit for bit
