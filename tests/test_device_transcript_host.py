"""The device transcript without a GPU: the lane functions of csrc/transcript.inc, compiled for the host with the bound tracking on
(libhm_hostcheck.so), against ``hashlib`` and ``batch_verifier.transcript_challenges`` -- the compression, whole messages, the
streaming absorber at every byte offset and at the block boundaries, the wide reduction at its edges, a whole proof's lane on the
golden proofs -- and what ``hm_blake2b512_dev`` / ``hm_verify_transcript_dev`` refuse before a device is needed."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

from halo2_experiments_amd import _lib, batch_verifier as bvm, device_transcript as dt, poseidon as ps
from halo2_experiments_amd.bn256 import fr_array, fr_ints
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.transcript import PERSONAL
from halo2_experiments_amd.verifier import _instance_columns, _vk_digest

import prover_cases as pc
from conftest import GOLDEN

u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
LENGTHS = (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 1000)
HM_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_blake2b_compress.restype = None
    lib.hc_blake2b_compress.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int]
    lib.hc_blake2b.restype = None
    lib.hc_blake2b.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p, ctypes.c_size_t, ctypes.c_char_p, u8p]
    lib.hc_transcript_stream.restype = None
    lib.hc_transcript_stream.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p, u8p, u32p]
    lib.hc_fr_from_wide.restype = None
    lib.hc_fr_from_wide.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p]
    lib.hc_verify_transcript.restype = None
    lib.hc_verify_transcript.argtypes = [ctypes.c_size_t, u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, ctypes.c_uint32, u32p,
                                         ctypes.c_uint32, u32p, u32p, ctypes.c_uint32]
    lib.hc_transcript_schedule_problem.restype = ctypes.c_char_p
    lib.hc_transcript_schedule_problem.argtypes = [u32p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
    return lib


def message(length: int, salt: int = 0) -> bytes:
    return bytes((7 * i + 13 * salt + (i >> 8)) & 0xFF for i in range(length))


# ---- the compression and whole messages ---------------------------------------------------------------------------------------------------------
IV = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
      0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]


@pytest.mark.parametrize("person", [b"", PERSONAL], ids=["plain", "personal"])
def test_one_compression_is_a_one_block_hash(hc, person):
    """a message of 1 .. 128 bytes is one final compression of the padded block from the parameter block's state"""
    for length in (1, 63, 64, 127, 128):
        msg = message(length, 3)
        h = list(IV)
        h[0] ^= 0x01010040
        h[6] ^= int.from_bytes(person.ljust(16, b"\0")[:8], "little")
        h[7] ^= int.from_bytes(person.ljust(16, b"\0")[8:], "little")
        state = (ctypes.c_uint64 * 8)(*h)
        hc.hc_blake2b_compress(state, msg.ljust(128, b"\0"), length, 1)
        assert b"".join(int(w).to_bytes(8, "little") for w in state) == hashlib.blake2b(msg, digest_size=64, person=person).digest()


@pytest.mark.parametrize("person", [b"", PERSONAL], ids=["plain", "personal"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_whole_messages_against_hashlib(hc, person, shift):
    """every length of the list, the messages `shift` bytes off a word boundary: the byte path and the word path of the lane"""
    stride = 1004
    msgs = [message(n, n) for n in LENGTHS]
    raw = bytearray(shift + stride * len(msgs))
    for i, m in enumerate(msgs):
        raw[shift + i * stride:shift + i * stride + len(m)] = m
    buf = (ctypes.c_char * (len(raw) + 8)).from_buffer_copy(bytes(raw) + bytes(8))
    base = ctypes.addressof(buf)
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    out = np.zeros((len(msgs), 64), dtype=np.uint8)
    assert base % 4 == 0
    hc.hc_blake2b(ctypes.cast(base + shift, ctypes.c_char_p), stride, lens.ctypes.data_as(u32p), len(msgs),
                  person.ljust(16, b"\0") if person else None, out.ctypes.data_as(u8p))
    assert [bytes(row) for row in out] == [hashlib.blake2b(m, digest_size=64, person=person).digest() for m in msgs]


# ---- the streaming absorber ---------------------------------------------------------------------------------------------------------------------
def buffered(total: int) -> int:
    """the bytes Blake2b holds back after `total` bytes: a full block waits for the next byte"""
    return 0 if total == 0 else (total - 1) % 128 + 1


def stream_case(seed: int):
    """random 33- and 65-byte records and squeezes, then squeezes until one was taken at each of the three positions"""
    rng = random.Random(seed)
    ops = [rng.choice((0, 1, 1, 2, 2)) for _ in range(120)] + [0, 0]          # ends on two squeezes in a row
    total = sum({0: 1, 1: 65, 2: 33}[o] for o in ops)
    for target in (128, 1, 127):
        ops.append(rng.choice((1, 2)))
        total += {1: 65, 2: 33}[ops[-1]]
        while True:
            ops.append(0)
            total += 1
            if buffered(total) == target:
                break
    return ops


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_streaming_absorber_against_a_hashlib_twin(hc, seed):
    ops = stream_case(seed)
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 1 << 32, size=sum({0: 0, 1: 16, 2: 8}[o] for o in ops), dtype=np.uint64).astype(np.uint32)
    n_squeeze = ops.count(0)
    digests = np.zeros((n_squeeze, 64), dtype=np.uint8)
    positions = np.zeros(len(ops), dtype=np.uint32)
    hc.hc_transcript_stream(bytes(ops), len(ops), data.ctypes.data_as(u32p), digests.ctypes.data_as(u8p), positions.ctypes.data_as(u32p))
    twin, at, total, expected, where, residues = hashlib.blake2b(digest_size=64, person=PERSONAL), 0, 0, [], [], set()
    for i, o in enumerate(ops):
        words = {0: 0, 1: 16, 2: 8}[o]
        twin.update(bytes([o]) + data[at:at + words].tobytes())
        at += words
        total += 1 + 4 * words
        residues.add(total % 4)
        assert positions[i] == buffered(total)
        if o == 0:
            expected.append(twin.copy().digest())                             # the twin goes on from the state WITH the prefix byte
            where.append(buffered(total))
    assert {128, 1, 127} <= set(where) and residues == {0, 1, 2, 3}           # the three positions, and records at every byte offset
    got = [bytes(row) for row in digests]
    # every later digest equals the twin's, so the running state behind each squeeze was the twin's: the copy was finalised, not it
    assert got == expected
    in_a_row = [k for k in range(1, len(ops)) if ops[k] == 0 and ops[k - 1] == 0]
    index = {k: j for j, k in enumerate(i for i, o in enumerate(ops) if o == 0)}
    assert in_a_row and all(got[index[k]] != got[index[k - 1]] for k in in_a_row)   # two squeezes in a row differ


# ---- the wide reduction -------------------------------------------------------------------------------------------------------------------------
def test_wide_reduction_against_the_integers(hc):
    rng = random.Random(5)
    cases = [R, R - 1, (2 ** 256 - 1) << 256, R << 256, 2 ** 512 - 1, 0, 1, 2 ** 256, (R - 1) << 256 | (R - 1)]
    cases += [rng.getrandbits(512) for _ in range(64)]
    raw = b"".join(v.to_bytes(64, "little") for v in cases)
    out = np.zeros((len(cases), 8), dtype=np.uint32)
    hc.hc_fr_from_wide(raw, len(cases), out.ctypes.data_as(u32p))
    assert fr_ints(out.view(np.uint64)) == [v % R for v in cases]
    assert np.array_equal(out.view(np.uint64), fr_array([v % R for v in cases]))          # canonical Montgomery words, bit for bit


# ---- a whole proof's lane -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("poseidon_k6", "poseidon_k6", 88), ("merkle_sum_d5_k9", "merkle_sum_k9", 10)], ids=lambda p: p[1])
def golden_proof(request):
    name, short, boundary = request.param
    cs, k = pc.constraint_system(name)
    meta = np.load(os.path.join(GOLDEN, f"proof_{short}.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, f"proof_{short}.bin"), "rb").read()
    return cs, vk, ps.words_to_ints(meta["instance"]), proof, bvm.ProofLayout(cs, k), boundary


def lane(hc, lay, proofs, ybytes, preambles, stride=None, bad=None, record_elems=9, schedule=None, fill=0xA5A5A5A5):
    """hc_verify_transcript on every proof of a host batch -> (records (B, record_elems, 8) u32, bad flags)"""
    B = len(proofs)
    raw = np.frombuffer(b"".join(proofs), dtype=np.uint32).copy()
    yb = np.frombuffer(b"".join(b"".join(rows) for rows in ybytes), dtype=np.uint32).copy()
    counts = np.array([len(p) for p in preambles], dtype=np.uint32)
    stride = stride or max(int(counts.max()), 1)
    pre = np.zeros((B, stride, 8), dtype=np.uint32)
    for b, values in enumerate(preambles):
        if len(values) <= stride:
            pre[b, :len(values)] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint32).reshape(-1, 8)
    sched = np.ascontiguousarray(schedule if schedule is not None else lay.transcript_schedule(), dtype=np.uint32)
    flags = np.array(bad if bad is not None else [0] * B, dtype=np.uint32)
    records = np.full((B, record_elems, 8), fill, dtype=np.uint32)
    table = np.ascontiguousarray(lay.slot_table)
    for b in range(B):
        hc.hc_verify_transcript(b, raw.ctypes.data_as(u32p), table.ctypes.data_as(u32p), lay.slots, lay.n_points, yb.ctypes.data_as(u32p),
                                pre.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), stride, sched.ctypes.data_as(u32p), len(sched),
                                flags.ctypes.data_as(u32p), records.ctypes.data_as(u32p), record_elems)
    return records, flags


def test_the_lane_gives_the_challenges_of_the_golden_proofs(hc, golden_proof):
    """all 8 challenges word for word, for the proof as recorded and with a preamble that puts the theta squeeze on a block boundary.
    (1 + 88 scalars for Poseidon k = 6 and 1 + 10 for MerkleSumTree k = 9: with the squeeze's own prefix byte the transcript then
    holds 3328 = 26 * 128 and 1664 = 13 * 128 bytes -- recomputed below from ProofLayout -- and the digest is taken over a FULL block.)"""
    cs, vk, instance, proof, lay, boundary = golden_proof
    inst_cols = _instance_columns(cs, instance)
    digest = _vk_digest(vk)
    points, _ = bvm.read_proof_ints(lay, proof)
    ybytes = [y.to_bytes(32, "little") for _, y in points]
    rng = random.Random(boundary)
    on_boundary = [[rng.randrange(R) for _ in range(boundary)]]
    at_theta = 33 * (1 + boundary) + 65 * cs.num_advice + 1
    assert at_theta % 128 == 0 and at_theta == {88: 3328, 10: 1664}[boundary]
    cases = [inst_cols, on_boundary, [[]]]
    preambles = [[digest] + [v for col in cols for v in col] for cols in cases]
    records, flags = lane(hc, lay, [proof] * len(cases), [ybytes] * len(cases), preambles)
    assert not flags.any()
    for b, cols in enumerate(cases):
        ch = bvm.transcript_challenges(lay, digest, cols, proof, ybytes)
        assert np.array_equal(records[b, :8].view(np.uint64), fr_array([ch[name] for name in bvm.RECORD]))
        assert (records[b, 8] == 0xA5A5A5A5).all()                             # the element behind the challenges is the caller's
    assert len({records[b, :8].tobytes() for b in range(len(cases))}) == len(cases)


def test_the_lane_flags_and_zeroes(hc, golden_proof):
    cs, vk, instance, proof, lay, _ = golden_proof
    digest = _vk_digest(vk)
    points, _ = bvm.read_proof_ints(lay, proof)
    ybytes = [y.to_bytes(32, "little") for _, y in points]
    pre = [digest, 1, 2]
    # proof 1 is flagged on entry, proof 2 counts more preamble scalars than a row holds; 0 and 3 are their exact neighbours
    records, flags = lane(hc, lay, [proof] * 4, [ybytes] * 4, [pre, pre, pre + [3], pre], stride=3, bad=[0, 1, 0, 0])
    assert flags.tolist() == [0, 1, 1, 0]
    assert not records[1, :8].any() and not records[2, :8].any() and (records[:, 8] == 0xA5A5A5A5).all()
    ch = bvm.transcript_challenges(lay, digest, [[1, 2]], proof, ybytes)
    want = fr_array([ch[name] for name in bvm.RECORD])
    assert np.array_equal(records[0, :8].view(np.uint64), want) and np.array_equal(records[3, :8].view(np.uint64), want)


# ---- the schedule and the boundary's refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"])
def test_transcript_schedule_covers_slots_and_challenges(hc, name):
    cs, k = pc.constraint_system(name)
    lay = bvm.ProofLayout(cs, k)
    sched = lay.transcript_schedule()
    assert sum(a for a, _ in sched) == lay.slots and sum(s for _, s in sched) == 8 == len(bvm.RECORD)
    assert sched[0] == (cs.num_advice, 1) and sched[-2:] == [(1, 1), (1, 0)] and sched[4] == (lay.n_scalars, 2)
    words = np.ascontiguousarray(sched, dtype=np.uint32)
    assert hc.hc_transcript_schedule_problem(words.ctypes.data_as(u32p), len(sched), lay.slots, 9) is None
    assert b"sum to the proof's slots" in hc.hc_transcript_schedule_problem(words.ctypes.data_as(u32p), len(sched), lay.slots + 1, 9)
    assert b"more challenges" in hc.hc_transcript_schedule_problem(words.ctypes.data_as(u32p), len(sched), lay.slots, 7)


def test_modes_and_python_refusals():
    assert dt.MODES == ("host", "device")
    cs, k = pc.constraint_system("poseidon_k6")
    with pytest.raises(ValueError, match="transcript must be one of"):
        bvm.BatchVerifier(None, None, transcript="gpu")
    with pytest.raises(ValueError, match="16 bytes"):
        dt.blake2b([b"x"], person=b"x" * 17)
    assert dt.blake2b([]) == []
    raw, counts = dt.preamble_rows(5, [[[1, 2], [3]], [[], []]])
    assert raw.shape == (2, 4, 32) and counts.tolist() == [4, 1]
    assert raw[0].tobytes() == b"".join(v.to_bytes(32, "little") for v in (5, 1, 2, 3)) and raw[1, 0].tobytes() == (5).to_bytes(32, "little")
    assert not raw[1, 1:].any()


def test_argument_errors_come_before_the_device():
    lib = _lib.load()
    for name in ("hm_blake2b512_dev", "hm_verify_transcript_dev"):
        assert name in _lib._SIGNATURES
    vp = ctypes.c_void_p
    p16, p4, odd = vp(0x1000), ctypes.cast(vp(0x2000), u32p), ctypes.cast(vp(0x2002), u32p)
    # hm_blake2b512_dev(d_msgs, stride, d_lens, n, personal16, d_out, stream)
    b2_base = dict(msgs=p16, stride=64, lens=p4, n=1, person=None, out=p16, stream=None)
    b2 = lambda **kw: lib.hm_blake2b512_dev(*[dict(b2_base, **kw)[key] for key in ("msgs", "stride", "lens", "n", "person", "out", "stream")])
    for kw, why in ((dict(msgs=None), b"null"), (dict(lens=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n <= 2^24"),
                    (dict(n=(1 << 24) + 1), b"n <= 2^24"), (dict(stride=0), b"stride"), (dict(stride=1 << 32), b"stride"),
                    (dict(lens=odd), b"aligned"), (dict(out=vp(0x1002)), b"aligned")):
        assert b2(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
    # hm_verify_transcript_dev
    sched = np.array([[3, 1], [2, 1]], dtype=np.uint32)
    base = dict(proofs=p16, n=2, table=p4, slots=5, points=2, ybytes=p16, pre=p16, counts=p4, stride=1, sched=sched.ctypes.data_as(u32p),
                pairs=2, bad=p4, records=p16, elems=3, stream=None)
    order = ("proofs", "n", "table", "slots", "points", "ybytes", "pre", "counts", "stride", "sched", "pairs", "bad", "records", "elems", "stream")
    tr = lambda **kw: lib.hm_verify_transcript_dev(*[dict(base, **kw)[key] for key in order])
    short = np.array([[3, 1], [1, 1]], dtype=np.uint32)
    for kw, why in ([(dict([(key, None)]), b"null") for key in ("proofs", "table", "ybytes", "pre", "counts", "sched", "bad", "records")] +
                    [(dict(n=0), b"n_proofs"), (dict(n=(1 << 24) + 1), b"n_proofs"), (dict(slots=0), b"slots"), (dict(slots=(1 << 16) + 1), b"slots"),
                     (dict(points=6), b"points <= slots"), (dict(stride=0), b"preamble_stride"), (dict(elems=0), b"record_elems"),
                     (dict(pairs=0), b"n_schedule_pairs"), (dict(sched=short.ctypes.data_as(u32p)), b"do not sum"),
                     (dict(slots=4), b"do not sum"), (dict(elems=1), b"more challenges"), (dict(proofs=vp(0x1004)), b"16-byte"),
                     (dict(ybytes=vp(0x1008)), b"16-byte"), (dict(pre=vp(0x1001)), b"16-byte"), (dict(records=vp(0x1004)), b"16-byte"),
                     (dict(table=odd), b"4-byte"), (dict(counts=odd), b"4-byte"), (dict(bad=odd), b"4-byte")]):
        assert tr(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
