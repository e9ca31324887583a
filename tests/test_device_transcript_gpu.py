"""The device transcript on the GPU (csrc/transcript.inc): ``hm_blake2b512_dev`` against ``hashlib`` across two wavefronts,
``hm_verify_transcript_dev`` against ``batch_verifier.transcript_challenges`` bit for bit on proofs made as
tests/test_batch_verifier_gpu.py makes them -- lane-divergent preamble counts, flagged lanes between exact neighbours -- and
``BatchVerifier(transcript="device")`` against host mode: the same scalar arrays, booleans and ``failing()`` lists."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, device_transcript as dt
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fr_array
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.transcript import PERSONAL
from halo2_experiments_amd.verifier import _vk_digest

import prover_cases as pc
from test_batch_verifier_gpu import CASES, flipped, make_case, put, tiled

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 1000)
LANES = 65                                                                     # crosses a wavefront: one block of 64 lanes and one lane more
SENTINEL = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def cases():
    made = {name: make_case(name) for name in CASES}
    yield made
    for c in made.values():
        c["params"].release()


def message(length: int, salt: int) -> bytes:
    return bytes((5 * i + 11 * salt + (i >> 8)) & 0xFF for i in range(length))


# ---- Blake2b -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("person", [b"", PERSONAL], ids=["plain", "personal"])
def test_blake2b_kernel_against_hashlib(person):
    msgs = [message(LENGTHS[(4 * i + i // 11) % len(LENGTHS)], i) for i in range(130)]       # two wavefronts and two lanes more
    assert all(len(a) != len(b) for a, b in zip(msgs, msgs[1:])) and {len(m) for m in msgs} == set(LENGTHS)
    assert dt.blake2b(msgs, person=person) == [hashlib.blake2b(m, digest_size=64, person=person).digest() for m in msgs]


def test_blake2b_kernel_at_odd_strides_and_lengths_past_the_stride():
    """a stride that is no multiple of 4 sends lanes down the byte path; a length above the stride gives zeros and reads nothing"""
    stride, n = 131, 70
    lens = [(37 * i) % (stride + 1) for i in range(n)]
    lens[3], lens[64] = stride + 1, 1 << 31
    raw = np.frombuffer(message(stride * n, 9), dtype=np.uint8).reshape(n, stride)
    d_msgs = torch.from_numpy(raw.copy()).cuda()
    d_lens = torch.from_numpy(np.array(lens, dtype=np.uint32).view(np.int32)).cuda()
    d_out = torch.full((n, 64), 0xEE, dtype=torch.uint8, device="cuda")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _lib.check(_lib.load().hm_blake2b512_dev(ctypes.c_void_p(d_msgs.data_ptr()), stride, ctypes.cast(ctypes.c_void_p(d_lens.data_ptr()), u32p), n,
                                            None, ctypes.c_void_p(d_out.data_ptr()), None))
    torch.cuda.synchronize()
    got = [bytes(row) for row in d_out.cpu().numpy()]
    want = [bytes(64) if lens[i] > stride else hashlib.blake2b(raw[i, :lens[i]].tobytes(), digest_size=64).digest() for i in range(n)]
    assert got == want


# ---- the transcript kernel -----------------------------------------------------------------------------------------------------------------
def uploaded(c, members):
    """the proofs of a batch and the y bytes of their points on the device, as the read kernel takes and leaves them"""
    lay = c["layout"]
    raw = np.stack([np.frombuffer(proof, dtype=np.uint8) for _, proof in members])
    ybytes = []
    for _, proof in members:
        points, _ = bvm.read_proof_ints(lay, proof)
        ybytes.append([y.to_bytes(32, "little") for _, y in points])
    yb = np.frombuffer(b"".join(b"".join(rows) for rows in ybytes), dtype=np.uint8).reshape(len(members), lay.n_points, 32)
    return torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(yb.copy()).cuda(), ybytes


@pytest.mark.parametrize("name", CASES)
def test_transcript_kernel_equals_the_host_transcripts(cases, name):
    c, lay = cases[name], cases[name]["layout"]
    members = tiled(c, LANES)
    digest = _vk_digest(c["vk"])
    real = [bvm._instance_columns(c["cs"], inst) for inst, _ in members]
    # lane-divergent preamble counts in one batch: the digest alone, the digest and one value, the digest and 88 values (for Poseidon
    # k = 6 that puts the theta squeeze on a block boundary), and the proof's own instance
    rng = np.random.default_rng(len(name))
    shapes = [[[]], [[int(rng.integers(1, 1 << 62))]], [[int(v) for v in rng.integers(1, 1 << 62, size=88)]], None]
    instances = [shapes[b % 4] if shapes[b % 4] is not None else real[b] for b in range(LANES)]
    assert {1, 2, 89} <= {1 + sum(len(col) for col in cols) for cols in instances}
    flagged = [5, 63, 64]
    d_proofs, d_ybytes, ybytes = uploaded(c, members)
    d_bad = torch.zeros(LANES, dtype=torch.int32, device="cuda")
    d_bad[flagged] = 1
    records = np.full((LANES, 9, 4), SENTINEL, dtype=np.uint64)
    d_records = torch.from_numpy(records.view(np.int64)).cuda()
    dt.challenges(lay, digest, instances, d_proofs, d_ybytes, d_bad, d_records)
    torch.cuda.synchronize()
    got = d_records.cpu().numpy().view(np.uint64)
    assert d_bad.cpu().tolist() == [int(b in flagged) for b in range(LANES)]
    assert (got[:, 8] == SENTINEL).all()                                        # the r_b element is untouched
    memo = {}
    for b, (cols, (_, proof)) in enumerate(zip(instances, members)):
        if b in flagged:
            assert not got[b, :8].any()
            continue
        key = (b % 4, proof)
        if key not in memo:
            ch = bvm.transcript_challenges(lay, digest, cols, proof, ybytes[b])
            memo[key] = fr_array([ch[k] for k in bvm.RECORD])
        assert np.array_equal(got[b, :8], memo[key]), b


def test_transcript_kernel_flags_a_preamble_count_past_the_stride(cases):
    c, lay = cases["poseidon_k6"], cases["poseidon_k6"]["layout"]
    members = tiled(c, 3)
    digest = _vk_digest(c["vk"])
    d_proofs, d_ybytes, ybytes = uploaded(c, members)
    d_pre, d_counts = dt.upload_preamble(digest, [[[1]], [[1]], [[1]]], d_proofs.device)
    d_counts[1] = 3                                                             # the rows hold two scalars
    d_bad = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_records = torch.from_numpy(np.full((3, 9, 4), SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    dt.challenges(lay, digest, None, d_proofs, d_ybytes, d_bad, d_records, preamble=(d_pre, d_counts))
    torch.cuda.synchronize()
    got = d_records.cpu().numpy().view(np.uint64)
    assert d_bad.cpu().tolist() == [0, 1, 0] and not got[1, :8].any() and (got[:, 8] == SENTINEL).all()
    for b in (0, 2):
        ch = bvm.transcript_challenges(lay, digest, [[1]], members[b][1], ybytes[b])
        assert np.array_equal(got[b, :8], fr_array([ch[k] for k in bvm.RECORD]))


# ---- BatchVerifier(transcript="device") ----------------------------------------------------------------------------------------------------
def batch(c, members, seed=5, **modes):
    bv = h.BatchVerifier(c["params"], c["vk"], seed=seed, **modes)
    for inst, proof in members:
        bv.add_proof(inst, proof)
    return bv


@pytest.mark.parametrize("name", CASES)
def test_device_mode_leaves_the_scalar_arrays_of_host_mode(cases, name):
    c = cases[name]
    members = tiled(c, 5)
    host, dev = batch(c, members), batch(c, members, transcript="device")
    a, b = host._prepare(), dev._prepare()
    assert a["bad"] == b["bad"] == [False] * 5 and host.randomizers == dev.randomizers
    for key in ("d_own", "d_shared", "d_h2_r", "d_h2_l", "d_bases", "d_scalars"):
        assert torch.equal(a[key], b[key]), key
    assert b["ybytes"] is None and torch.equal(b["d_ybytes"].cpu(), torch.from_numpy(a["ybytes"]))
    assert set(host.timings) == set(dev.timings)
    assert dev.finalize(trapdoor=pc.SRS_S) and dev.msm_calls == 4
    assert h.verify_proofs(c["params"], c["vk"], [i for i, _ in members], [p for _, p in members], seed=3, trapdoor=pc.SRS_S, transcript="device")


@pytest.mark.parametrize("count", [1, 64, 65])
def test_device_mode_batches_verify(cases, count):
    c = cases["poseidon_k6"]
    members = tiled(c, count)
    assert batch(c, members, transcript="device").finalize(trapdoor=pc.SRS_S)
    bv = batch(c, members, transcript="device", pairing="device")
    assert bv.finalize() and bv.failing() == []


def test_device_mode_names_the_failing_proofs_of_host_mode(cases):
    c, lay = cases["poseidon_k6"], cases["poseidon_k6"]["layout"]
    members = tiled(c, 65)
    inst, good = members[0]
    members[7] = (members[7][0], flipped(members[7][1], 32 * lay.points_before_evals + 32 * 3 + 1))     # an evaluation byte
    members[64] = (inst, put(good, 0, P.to_bytes(32, "little")))                                        # a malformed point
    members[30] = (inst, good[:-32])                                                                    # a wrong length
    host, dev = batch(c, members), batch(c, members, transcript="device")
    assert not dev.finalize(trapdoor=pc.SRS_S) and not host.finalize(trapdoor=pc.SRS_S)
    assert dev.failing(trapdoor=pc.SRS_S) == host.failing(trapdoor=pc.SRS_S) == [7, 30, 64]
    assert dev.malformed() == host.malformed() == [30, 64]
    a, b = host._prepare(), dev._prepare()
    for key in ("d_own", "d_shared", "d_h2_r", "d_h2_l"):
        assert torch.equal(a[key], b[key]), key


def test_unknown_transcript_value_is_refused(cases):
    c = cases["poseidon_k6"]
    with pytest.raises(ValueError, match="transcript must be one of"):
        h.BatchVerifier(c["params"], c["vk"], transcript="gpu")
    with pytest.raises(ValueError, match="transcript must be one of"):
        h.verify_proofs(c["params"], c["vk"], [], [], transcript="hip")
