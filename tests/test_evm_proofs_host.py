"""The EVM encoding without a GPU: ``KeccakWrite`` / ``KeccakRead`` round trips and refusals, the "evm" ``ProofLayout`` and its schedule,
the refusal of an unknown ``encoding`` on every public function, the read and transcript lanes of csrc/keccak.inc (libhm_hostcheck.so,
bound tracking on) against ``read_proof_ints`` / ``transcript_challenges`` and against the compressed read's words on the golden proofs
written in the other encoding, and what the three new entry points refuse before a device is needed."""
import ctypes
import os
import random

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, device_transcript as dt, poseidon as ps, prover, solvency, verifier
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fr_array, g1_words
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.pairing import G1_GEN, g1_mul
from halo2_experiments_amd.transcript import (ENCODINGS, Blake2bWrite, KeccakRead, KeccakWrite, TranscriptError, g1_uncompressed_int,
                                              keccak256)
from halo2_experiments_amd.verifier import _instance_columns, _vk_digest, proof_length

import evm_cases as ec
import prover_cases as pc
from conftest import GOLDEN

u32p = ctypes.POINTER(ctypes.c_uint32)
HM_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_evm_read.restype = ctypes.c_int
    lib.hc_evm_read.argtypes = [u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p]
    lib.hc_verify_read.restype = None
    lib.hc_verify_read.argtypes = [ctypes.c_char_p, u32p, u32p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t]
    lib.hc_verify_transcript_evm.restype = None
    lib.hc_verify_transcript_evm.argtypes = [ctypes.c_size_t, u32p, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p,
                                             ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module", params=[("poseidon_k6", "poseidon_k6"), ("merkle_sum_d5_k9", "merkle_sum_k9")], ids=lambda p: p[1])
def golden(request):
    """a recorded "halo2" proof and the same points and scalars in the "evm" encoding"""
    name, short = request.param
    cs, k = pc.constraint_system(name)
    meta = np.load(os.path.join(GOLDEN, f"proof_{short}.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, f"proof_{short}.bin"), "rb").read()
    lay2, lay = bvm.ProofLayout(cs, k), bvm.ProofLayout(cs, k, "evm")
    return dict(cs=cs, k=k, vk=vk, instance=ps.words_to_ints(meta["instance"]), halo2=proof, evm=ec.to_evm(lay2, proof), lay2=lay2, lay=lay)


# ---- the transcript classes ---------------------------------------------------------------------------------------------------------------------
def some_points(count: int, seed: int):
    rng = random.Random(seed)
    return [g1_mul(rng.randrange(1, R), G1_GEN) for _ in range(count)]


def test_write_then_read_yields_the_same_challenges():
    rng = random.Random(1)
    pts = some_points(5, 2)
    w = KeccakWrite()
    script, challenges = [], []
    w.common_scalar(12345)
    for step in ("p", "p", "c", "c", "s", "c", "p", "s", "s", "c", "p", "p", "c"):
        if step == "p":
            script.append(("p", pts[len(script) % 5]))
            w.write_point(script[-1][1])
        elif step == "s":
            script.append(("s", rng.randrange(R)))
            w.write_scalar(script[-1][1])
        else:
            script.append(("c", None))
            challenges.append(w.squeeze_challenge())
    proof = w.finalize()
    assert len(proof) == 64 * sum(kind == "p" for kind, _ in script) + 32 * sum(kind == "s" for kind, _ in script)
    r = KeccakRead(proof)
    r.common_scalar(12345)
    got = []
    for kind, value in script:
        if kind == "p":
            assert r.read_point() == value
        elif kind == "s":
            assert r.read_scalar() == value
        else:
            got.append(r.squeeze_challenge())
    assert got == challenges and r.remaining() == 0 and len(set(got)) == len(got) and all(c < R for c in got)
    # the bytes: a point is x then y big-endian, a scalar big-endian, as absorbed
    x, y = script[0][1]
    assert proof[:64] == x.to_bytes(32, "big") + y.to_bytes(32, "big")


def test_squeeze_follows_the_stated_buffer_rule():
    t = KeccakWrite()
    t.common_scalar(7)
    first = keccak256((7).to_bytes(32, "big") + b"\x01")                       # exactly 32 bytes: the extra byte
    assert t.squeeze_challenge() == int.from_bytes(first, "big") % R
    second = keccak256(first + b"\x01")                                        # the digest alone: again
    assert t.squeeze_challenge() == int.from_bytes(second, "big") % R
    t.common_scalar(9)
    third = keccak256(second + (9).to_bytes(32, "big"))                        # 64 bytes: none
    assert t.squeeze_challenge() == int.from_bytes(third, "big") % R


def test_each_refusal_fires():
    x, y = some_points(1, 3)[0]
    enc = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")
    assert KeccakRead(enc(x, y)).read_point() == (x, y)
    for bad, why in ((enc(x + P, y), "canonical"), (enc(x, y + P), "canonical"), (enc(x, y ^ 1), "curve"), (bytes(64), "curve"),
                     (enc(x, y)[:63], "ends early")):
        with pytest.raises(TranscriptError, match=why):
            KeccakRead(bad).read_point()
    assert KeccakRead((R - 1).to_bytes(32, "big")).read_scalar() == R - 1
    for bad, why in ((R.to_bytes(32, "big"), "below r"), (bytes(31), "ends early")):
        with pytest.raises(TranscriptError, match=why):
            KeccakRead(bad).read_scalar()
    with pytest.raises(TranscriptError, match="identity"):
        KeccakWrite().common_point(None)
    with pytest.raises(TranscriptError, match="64 bytes"):
        g1_uncompressed_int(bytes(32))


# ---- the layout -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.CASES)
def test_evm_layout_counts_two_slots_per_point(name):
    cs, k = pc.constraint_system(name)
    lay2, lay = bvm.ProofLayout(cs, k), bvm.ProofLayout(cs, k, "evm")
    assert lay.slots == 2 * lay.n_points + lay.n_scalars and 32 * lay.slots == proof_length(cs, 1, "evm") == 32 * lay2.slots + 32 * lay2.n_points
    assert (lay.n_points, lay.own_points, lay.n_scalars, lay.point_keys, lay.eval_keys) == \
           (lay2.n_points, lay2.own_points, lay2.n_scalars, lay2.point_keys, lay2.eval_keys)
    table = [int(e) for e in lay.slot_table]
    assert len(table) == lay.slots and len(lay.point_slots) == lay.n_points and len(lay.scalar_slots) == lay.n_scalars
    assert all(table[s] & bvm.EVM_POINT and table[s + 1] == bvm.EVM_SKIP for s in lay.point_slots)
    assert [table[s] & (bvm.EVM_SKIP - 1) for s in lay.point_slots] == list(range(lay.n_points))
    assert [bool(table[s] & bvm.EVM_TAIL) for s in lay.point_slots] == [False] * lay.own_points + [True]
    assert [table[s] for s in lay.scalar_slots] == list(range(lay.n_scalars))
    sched = lay.transcript_schedule()
    assert sum(a for a, _ in sched) == lay.slots and sum(s for _, s in sched) == 8 == len(bvm.RECORD)
    assert sched[0] == (2 * cs.num_advice, 1) and sched[-2:] == [(2, 1), (2, 0)] and sched[4] == (lay.n_scalars, 2)


@pytest.mark.parametrize("name", ec.CASES)
def test_default_layout_is_what_it_was(name):
    """the fields of ``ProofLayout(cs, k)`` restated from the constraint system: slots, table bits, slot lists and schedule"""
    cs, k = pc.constraint_system(name)
    lay = bvm.ProofLayout(cs, k)
    assert lay.encoding == "halo2" and bvm.ProofLayout(cs, k, "halo2").slot_table.tolist() == lay.slot_table.tolist()
    L, nsets, pieces = len(cs.lookups), cs.permutation_sets(), cs.degree() - 1
    before = cs.num_advice + 2 * L + nsets + L + 1 + pieces
    assert lay.points_before_evals == before and lay.n_points == before + 2 and lay.own_points == before + 1
    assert lay.slots == lay.n_points + lay.n_scalars and 32 * lay.slots == proof_length(cs) == proof_length(cs, 1, "halo2")
    want = [(1 << 31) | i for i in range(before)] + list(range(lay.n_scalars)) + [(1 << 31) | before, (1 << 31) | (1 << 30) | (before + 1)]
    assert lay.slot_table.dtype == np.uint32 and lay.slot_table.tolist() == want
    assert lay.point_slots == list(range(before)) + [lay.slots - 2, lay.slots - 1]
    assert lay.scalar_slots == list(range(before, before + lay.n_scalars))
    assert lay.transcript_schedule() == [(cs.num_advice, 1), (2 * L, 2), (nsets + L + 1, 1), (pieces, 1), (lay.n_scalars, 2), (1, 1), (1, 0)]
    assert (bvm.VR_POINT, bvm.VR_TAIL) == (1 << 31, 1 << 30)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_unknown_encoding_is_refused_everywhere():
    """before anything else is looked at: every argument but the encoding is None"""
    assert ENCODINGS == ("halo2", "evm")
    cs, k = pc.constraint_system("poseidon_k6")
    calls = [lambda e: prover.create_proof(None, None, None, None, 0, encoding=e), lambda e: prover.create_proofs(None, None, None, None, 0, encoding=e),
             lambda e: verifier.verify_proof(None, None, None, b"", encoding=e), lambda e: proof_length(cs, 1, encoding=e),
             lambda e: bvm.ProofLayout(cs, k, encoding=e), lambda e: bvm.BatchVerifier(None, None, encoding=e),
             lambda e: bvm.verify_proofs(None, None, [], [], encoding=e), lambda e: solvency.prove_balances(None, None, None, 0, encoding=e),
             lambda e: solvency.verify_balances(None, None, None, encoding=e), lambda e: dt.preamble_rows(1, [], encoding=e),
             lambda e: h.create_proof(None, None, None, None, 0, encoding=e), lambda e: h.verify_proof(None, None, None, b"", encoding=e)]
    for call in calls:
        for bad in ("keccak", "EVM", "", None, "device"):
            with pytest.raises(ValueError, match="encoding must be one of"):
                call(bad)
    with pytest.raises(TypeError):                                            # the name `transcript` keeps its meaning: host or device
        prover.create_proof(None, None, None, None, 0, transcript="evm")
    with pytest.raises(TypeError):                                            # multi-circuit proofs are out of scope
        prover.create_proof_multi(None, None, None, None, 0, encoding="evm")


def test_a_proof_of_the_other_encoding_is_malformed(golden):
    """wrong length on both sides; and cut or padded to the right length it still does not read or does not verify"""
    g = golden
    params = type("Params", (), {"g2": None, "s_g2": None})()
    assert not verifier.verify_proof(params, g["vk"], g["instance"], g["halo2"], encoding="evm")
    assert not verifier.verify_proof(params, g["vk"], g["instance"], g["evm"])
    for lay, other in ((g["lay"], g["halo2"]), (g["lay2"], g["evm"])):
        with pytest.raises(bvm.MalformedProof, match="length"):
            bvm.read_proof_ints(lay, other)
    with pytest.raises(bvm.MalformedProof):
        bvm.read_proof_ints(g["lay"], g["halo2"].ljust(len(g["evm"]), b"\0"))


# ---- the read lane ------------------------------------------------------------------------------------------------------------------------------------
def read_lane(hc, lay, proof: bytes, table=None, own=None, scalars=None, fill=0):
    raw = np.frombuffer(proof, dtype=np.uint32).copy()
    table = np.ascontiguousarray(lay.slot_table if table is None else table, dtype=np.uint32)
    own = lay.own_points if own is None else own
    scalars = lay.n_scalars if scalars is None else scalars
    pts = np.full((max(own, 1), 16), fill, dtype=np.uint32)
    tail = np.full(16, fill, dtype=np.uint32)
    sc = np.full((max(scalars, 1), 8), fill, dtype=np.uint32)
    ok = hc.hc_evm_read(raw.ctypes.data_as(u32p), table.ctypes.data_as(u32p), len(table), own, scalars, pts.ctypes.data_as(u32p),
                        tail.ctypes.data_as(u32p), sc.ctypes.data_as(u32p))
    return ok, pts, tail, sc


def test_read_lane_gives_the_twins_words_and_the_compressed_reads(hc, golden):
    g = golden
    lay, lay2 = g["lay"], g["lay2"]
    ok, pts, tail, sc = read_lane(hc, lay, g["evm"])
    points, scalars = bvm.read_proof_ints(lay, g["evm"])
    assert ok == 1 and (points, scalars) == bvm.read_proof_ints(lay2, g["halo2"])
    assert np.array_equal(np.concatenate([pts, tail[None]]).view(np.uint64), np.stack([g1_words(p) for p in points])[:, :8])
    assert np.array_equal(sc.view(np.uint64), fr_array(scalars))
    # ... bit for bit what the compressed read leaves for the same points and scalars
    kinds = bytes(1 if int(e) & bvm.VR_POINT else 0 for e in lay2.slot_table)
    raw = np.frombuffer(g["halo2"], dtype=np.uint32).copy()
    out, valid = np.zeros((lay2.slots, 24), dtype=np.uint32), np.zeros(lay2.slots, dtype=np.int32)
    hc.hc_verify_read(kinds, raw.ctypes.data_as(u32p), out.ctypes.data_as(u32p), valid.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), lay2.slots)
    assert valid.all()
    assert np.array_equal(np.concatenate([pts, tail[None]]), out[lay2.point_slots, :16]) and np.array_equal(sc, out[lay2.scalar_slots, :8])


def test_read_lane_refuses_what_the_twin_refuses(hc, golden):
    g = golden
    lay = g["lay"]
    good = read_lane(hc, lay, g["evm"])
    for name, bad in ec.tampers(lay, g["evm"]).items():
        with pytest.raises(bvm.MalformedProof):
            bvm.read_proof_ints(lay, bad)
        ok, pts, tail, sc = read_lane(hc, lay, bad)
        assert ok == 0, name
        # zeros where the slot was refused, the neighbours as in the good proof
        differ = [not np.array_equal(a, b) for a, b in zip(np.concatenate([pts, tail[None]]), np.concatenate([good[1], good[2][None]]))]
        differ_s = [not np.array_equal(a, b) for a, b in zip(sc, good[3])]
        assert sum(differ) + sum(differ_s) == 1, name
        hit = np.concatenate([pts, tail[None]])[differ.index(True)] if any(differ) else sc[differ_s.index(True)]
        assert not hit.any(), name
    # the edges that ARE read: r - 1, and p - 1 as a coordinate is canonical (and off the curve here)
    s0 = lay.scalar_slots[0]
    ok, _, _, sc = read_lane(hc, lay, ec.put(g["evm"], s0, R - 1))
    assert ok == 1 and np.array_equal(sc[0].view(np.uint64), fr_array([R - 1])[0])


def test_read_lane_keeps_inside_its_arrays(hc, golden):
    """a table entry outside its array flags the proof, and nothing is written: the arrays keep their fill"""
    g = golden
    lay = g["lay"]
    FILL = 0xA5A5A5A5
    table = lay.slot_table.copy()
    cases = {"point index": (lay.point_slots[0], bvm.EVM_POINT | lay.own_points), "scalar index": (lay.scalar_slots[0], lay.n_scalars),
             "x slot at the end": (lay.slots - 1, bvm.EVM_POINT | bvm.EVM_TAIL)}
    for name, (slot, entry) in cases.items():
        t = table.copy()
        t[slot] = entry
        ok, pts, tail, sc = read_lane(hc, lay, g["evm"], table=t, fill=FILL)
        assert ok == 0, name
        written_p = [(row != FILL).any() for row in pts]
        written_s = [(row != FILL).any() for row in sc]
        assert sum(written_p) >= lay.own_points - 1 and sum(written_s) >= lay.n_scalars - 1, name
    # smaller arrays than the table names: every index at or past them is refused and nothing lies behind the arrays' ends
    ok, pts, tail, sc = read_lane(hc, lay, g["evm"], own=2, scalars=3, fill=FILL)
    assert ok == 0 and pts.shape == (2, 16) and sc.shape == (3, 8) and (pts != FILL).any(axis=1).all() and (sc != FILL).any(axis=1).all()


# ---- the transcript lane --------------------------------------------------------------------------------------------------------------------------------
def transcript_lane(hc, lay, proofs, preambles, stride=None, bad=None, record_elems=9, fill=0xA5A5A5A5):
    """hc_verify_transcript_evm on every proof of a host batch -> (records (B, record_elems, 8) u32, bad flags)"""
    B = len(proofs)
    raw = np.frombuffer(b"".join(proofs), dtype=np.uint32).copy()
    counts = np.array([len(p) for p in preambles], dtype=np.uint32)
    stride = stride or max(int(counts.max()), 1)
    pre = np.zeros((B, stride, 8), dtype=np.uint32)
    for b, values in enumerate(preambles):
        if len(values) <= stride:
            pre[b, :len(values)] = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in values), dtype=np.uint32).reshape(-1, 8)
    sched = np.ascontiguousarray(lay.transcript_schedule(), dtype=np.uint32)
    flags = np.array(bad if bad is not None else [0] * B, dtype=np.uint32)
    records = np.full((B, record_elems, 8), fill, dtype=np.uint32)
    for b in range(B):
        hc.hc_verify_transcript_evm(b, raw.ctypes.data_as(u32p), lay.slots, pre.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), stride,
                                    sched.ctypes.data_as(u32p), len(sched), flags.ctypes.data_as(u32p), records.ctypes.data_as(u32p), record_elems)
    return records, flags


def boundary_instances(cs) -> int:
    """the instance count that puts the theta squeeze on a 136-byte boundary: 1 + instances + 2 advice points = 0 mod 17 words"""
    return (-(1 + 2 * cs.num_advice)) % 17 or 17


def test_transcript_lane_gives_the_twins_challenges(hc, golden):
    """all 8 challenges word for word: the recorded instance, a preamble that ends the theta block on a rate boundary, none at all --
    differing counts in one batch"""
    g = golden
    cs, lay, proof, digest = g["cs"], g["lay"], g["evm"], _vk_digest(g["vk"])
    rng = random.Random(17)
    count = boundary_instances(cs)
    assert 32 * (1 + count + 2 * cs.num_advice) % 136 == 0
    cases = [_instance_columns(cs, g["instance"]), [[rng.randrange(R) for _ in range(count)]], [[]]]
    preambles = [[digest] + [v for col in cols for v in col] for cols in cases]
    records, flags = transcript_lane(hc, lay, [proof] * 3, preambles)
    assert not flags.any() and len({len(p) for p in preambles}) == 3
    for b, cols in enumerate(cases):
        ch = bvm.transcript_challenges(lay, digest, cols, proof)
        assert np.array_equal(records[b, :8].view(np.uint64), fr_array([ch[name] for name in bvm.RECORD]))
        assert (records[b, 8] == 0xA5A5A5A5).all()                             # the element behind the challenges is the caller's
    assert len({records[b, :8].tobytes() for b in range(3)}) == 3
    # the twin is the reading transcript: KeccakRead over the same bytes squeezes the same theta
    t = KeccakRead(proof)
    t.common_scalar(digest)
    for v in (v for col in cases[0] for v in col):
        t.common_scalar(v)
    for _ in range(cs.num_advice):
        t.read_point()
    assert t.squeeze_challenge() == bvm.transcript_challenges(lay, digest, cases[0], proof)["theta"]


def test_transcript_lane_flags_and_zeroes(hc, golden):
    g = golden
    lay, proof, digest = g["lay"], g["evm"], _vk_digest(g["vk"])
    pre = [digest, 1, 2]
    # proof 1 is flagged on entry, proof 2 counts more preamble words than a row holds; 0 and 3 are their exact neighbours
    records, flags = transcript_lane(hc, lay, [proof] * 4, [pre, pre, pre + [3], pre], stride=3, bad=[0, 1, 0, 0])
    assert flags.tolist() == [0, 1, 1, 0]
    assert not records[1, :8].any() and not records[2, :8].any() and (records[:, 8] == 0xA5A5A5A5).all()
    ch = bvm.transcript_challenges(lay, digest, [[1, 2]], proof)
    want = fr_array([ch[name] for name in bvm.RECORD])
    assert np.array_equal(records[0, :8].view(np.uint64), want) and np.array_equal(records[3, :8].view(np.uint64), want)


def test_the_challenges_of_the_two_encodings_differ(golden):
    g = golden
    digest, cols = _vk_digest(g["vk"]), _instance_columns(g["cs"], g["instance"])
    points, _ = bvm.read_proof_ints(g["lay2"], g["halo2"])
    a = bvm.transcript_challenges(g["lay2"], digest, cols, g["halo2"], [y.to_bytes(32, "little") for _, y in points])
    b = bvm.transcript_challenges(g["lay"], digest, cols, g["evm"])
    assert set(a) == set(b) == set(bvm.RECORD) and all(a[name] != b[name] for name in bvm.RECORD)
    assert ec.to_halo2(g["lay"], g["evm"]) == g["halo2"]


def test_preamble_rows_are_big_endian_for_evm():
    raw, counts = dt.preamble_rows(5, [[[1, 2], [3]], [[], []]], "evm")
    assert raw.shape == (2, 4, 32) and counts.tolist() == [4, 1]
    assert raw[0].tobytes() == b"".join(v.to_bytes(32, "big") for v in (5, 1, 2, 3)) and not raw[1, 1:].any()
    assert dt.preamble_rows(5, [[[1]]])[0].tobytes() == dt.preamble_rows(5, [[[1]]], "halo2")[0].tobytes() == (5).to_bytes(32, "little") + (1).to_bytes(32, "little")
    assert dt.keccak256([]) == []


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    lib = _lib.load()
    for name in ("hm_keccak256_dev", "hm_verify_read_proofs_evm_dev", "hm_verify_transcript_evm_dev"):
        assert name in _lib._SIGNATURES
    vp = ctypes.c_void_p
    p16, p4, odd = vp(0x1000), ctypes.cast(vp(0x2000), u32p), ctypes.cast(vp(0x2002), u32p)
    kc_base = dict(msgs=p16, stride=64, lens=p4, n=1, out=p16, stream=None)
    kc = lambda **kw: lib.hm_keccak256_dev(*[dict(kc_base, **kw)[key] for key in ("msgs", "stride", "lens", "n", "out", "stream")])
    for kw, why in ((dict(msgs=None), b"null"), (dict(lens=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n <= 2^24"),
                    (dict(n=(1 << 24) + 1), b"n <= 2^24"), (dict(stride=0), b"stride"), (dict(stride=1 << 32), b"stride"),
                    (dict(lens=odd), b"aligned"), (dict(out=vp(0x1002)), b"aligned")):
        assert kc(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
    rd_base = dict(proofs=p16, n=2, table=p4, slots=7, own=2, scalars=1, points=p16, tail=p16, out=p16, bad=p4, stream=None)
    rd_order = ("proofs", "n", "table", "slots", "own", "scalars", "points", "tail", "out", "bad", "stream")
    rd = lambda **kw: lib.hm_verify_read_proofs_evm_dev(*[dict(rd_base, **kw)[key] for key in rd_order])
    for kw, why in ([(dict([(key, None)]), b"null") for key in ("proofs", "table", "points", "tail", "out", "bad")] +
                    [(dict(n=0), b"n_proofs"), (dict(n=(1 << 24) + 1), b"n_proofs"), (dict(slots=0), b"slots"), (dict(slots=(1 << 16) + 1), b"slots"),
                     (dict(own=4), b"2 own_points + scalars"), (dict(scalars=4), b"2 own_points + scalars"), (dict(proofs=vp(0x1004)), b"16-byte"),
                     (dict(points=vp(0x1008)), b"16-byte"), (dict(tail=vp(0x1001)), b"16-byte"), (dict(out=vp(0x1004)), b"16-byte"),
                     (dict(table=odd), b"4-byte"), (dict(bad=odd), b"4-byte")]):
        assert rd(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
    sched = np.array([[3, 1], [2, 1]], dtype=np.uint32)
    short = np.array([[3, 1], [1, 1]], dtype=np.uint32)
    base = dict(proofs=p16, n=2, slots=5, pre=p16, counts=p4, stride=1, sched=sched.ctypes.data_as(u32p), pairs=2, bad=p4, records=p16, elems=3,
                stream=None)
    order = ("proofs", "n", "slots", "pre", "counts", "stride", "sched", "pairs", "bad", "records", "elems", "stream")
    tr = lambda **kw: lib.hm_verify_transcript_evm_dev(*[dict(base, **kw)[key] for key in order])
    for kw, why in ([(dict([(key, None)]), b"null") for key in ("proofs", "pre", "counts", "sched", "bad", "records")] +
                    [(dict(n=0), b"n_proofs"), (dict(n=(1 << 24) + 1), b"n_proofs"), (dict(slots=0), b"slots"), (dict(slots=(1 << 16) + 1), b"slots"),
                     (dict(stride=0), b"preamble_stride"), (dict(elems=0), b"record_elems"), (dict(pairs=0), b"n_schedule_pairs"),
                     (dict(sched=short.ctypes.data_as(u32p)), b"do not sum"), (dict(slots=4), b"do not sum"), (dict(elems=1), b"more challenges"),
                     (dict(proofs=vp(0x1004)), b"16-byte"), (dict(pre=vp(0x1001)), b"16-byte"), (dict(records=vp(0x1004)), b"16-byte"),
                     (dict(counts=odd), b"4-byte"), (dict(bad=odd), b"4-byte")]):
        assert tr(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
