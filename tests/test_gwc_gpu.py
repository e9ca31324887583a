"""The GWC multiopen on the GPU (``gwc``, ``create_proof(..., multiopen="gwc")``, ``hm_verify_terms_gwc_dev``,
``BatchVerifier(..., multiopen="gwc")``), on the four systems of tests/gwc_cases.py: round trips in both encodings against the SHPLONK
proof of the same seed, every witness point against the integer quotient, ``create_proofs`` / ``create_proof_multi``, the terms kernel
against ``terms_from_challenges`` on records no transcript produces, and the batch verifier in all four ``pairing`` x ``transcript``
modes with a tampered and a malformed proof in the batch."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, evaluation as ev, gwc, poseidon as ps, proof_layout as pl, synthesis as sy
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.pairing import g1_add
from halo2_experiments_amd.shplonk import g1_words_to_int
from halo2_experiments_amd.verifier import _instance_columns, _vk_digest, proof_length

import gwc_cases as gc
import mutation_cases as mc
from prover_cases import SRS_S, d, ints

pytestmark = pytest.mark.gpu
MODES = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]      # (pairing, transcript)
FILL = -0x5A5A5A5A5A5A5A5B
_u32p = ctypes.POINTER(ctypes.c_uint32)
_KEYS, _PROOFS = {}, {}


@pytest.fixture(scope="module")
def keys():
    def get(name):
        if name not in _KEYS:
            c = mc.case(name)
            params = ParamsKZG.setup(c.k, SRS_S)
            vk = h.keygen_vk(params, c.cs, c.lay)
            advice = torch.from_numpy(sy.columns_to_words(c.advice).view(np.int64)).cuda()
            _KEYS[name] = dict(case=c, params=params, vk=vk, pk=h.keygen_pk(params, vk, c.cs, c.lay, cosets=False), advice=advice,
                               instance=c.proof_instance)
        return _KEYS[name]
    yield get
    for entry in _KEYS.values():
        entry["params"].release()
    _KEYS.clear()
    _PROOFS.clear()


def proof_of(key, name, seed, encoding="halo2", multiopen="gwc"):
    """``create_proof`` once per (system, seed, encoding, scheme)"""
    at = (name, seed, encoding, multiopen)
    if at not in _PROOFS:
        _PROOFS[at] = h.create_proof(key["params"], key["pk"], key["advice"], key["instance"], seed, encoding=encoding, multiopen=multiopen)
    return _PROOFS[at]


# ---- the prover ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", gc.ENCODINGS)
@pytest.mark.parametrize("name", gc.SYSTEMS)
def test_round_trip_and_the_bytes_shared_with_shplonk(keys, name, encoding):
    key = keys(name)
    c, params, vk, inst = key["case"], key["params"], key["vk"], key["instance"]
    proof = proof_of(key, name, 7, encoding)
    lay = gc.layout(name, encoding)
    assert len(proof) == proof_length(c.cs, 1, encoding, "gwc", c.k) == 32 * lay.slots
    assert h.verify_proof(params, vk, inst, proof, trapdoor=SRS_S, encoding=encoding, multiopen="gwc")
    assert h.verify_proof(params, vk, inst, proof, encoding=encoding, multiopen="gwc")                       # by pairing
    other = proof_of(key, name, 7, encoding, "shplonk")
    shared = 32 * ((2 if encoding == "evm" else 1) * lay.points_before_evals + lay.n_scalars)
    assert proof[:shared] == other[:shared] and len(other) == proof_length(c.cs, 1, encoding)
    assert not h.verify_proof(params, vk, inst, other, trapdoor=SRS_S, encoding=encoding, multiopen="gwc")
    assert not h.verify_proof(params, vk, inst, proof, trapdoor=SRS_S, encoding=encoding)


@pytest.mark.parametrize("name", ["poseidon", "overflow_check_v2"])            # k = 6 and k = 5: integer polynomials of 64 and 32 coefficients
def test_every_witness_is_the_commitment_of_the_integer_quotient(keys, name):
    key = keys(name)
    c, params, vk = key["case"], key["params"], key["vk"]
    trace = {}
    proof = h.create_proof(params, key["pk"], key["advice"], key["instance"], 21, _trace=trace, multiopen="gwc")
    assert proof == proof_of(key, name, 21)
    lay = gc.layout(name)
    points, evals = pl.read_proof_ints(lay, proof)
    ch = pl.transcript_challenges(lay, _vk_digest(vk), _instance_columns(c.cs, key["instance"]), proof,
                                  [p[1].to_bytes(32, "little") for p in points])
    assert ch["x"] == trace["challenges"]["x"]
    omega, n = vk.domain.omega, lay.n
    polys = {k_: ints(p) for k_, p in trace["polys"].items()}
    queries = [(k_, ch["x"] * pow(omega, rot, R) % R, None) for k_, rot in lay.queries]
    quotients = gwc.create_opening_ints(queries, polys, ch["v"])
    assert len(quotients) == len(lay.groups) and all(len(q) == n - 1 for q in quotients)
    for i, q in enumerate(quotients):
        assert g1_words_to_int(params.commit(d(q + [0]))) == points[lay.own_index[("w", i)]], i


@pytest.mark.parametrize("name", ["poseidon", "merkle_sum_tree"])
def test_create_proofs_equals_create_proof_byte_for_byte(keys, name):
    key = keys(name)
    seeds = [31, 7, 1000]
    adv = torch.stack([key["advice"]] * 3)
    for encoding in gc.ENCODINGS if name == "poseidon" else ("halo2",):
        proofs = h.create_proofs(key["params"], key["pk"], adv, [key["instance"]] * 3, seeds, encoding=encoding, multiopen="gwc")
        for b, seed in enumerate(seeds):
            assert proofs[b] == proof_of(key, name, seed, encoding), (encoding, b)
        assert len(set(proofs)) == 3


def test_create_proof_multi_verifies_and_fails_with_the_instances_swapped(keys):
    key = keys("poseidon")
    spec, k = ps.default_spec(5), 6
    rng = random.Random(5)
    adv, inst = sy.poseidon_circuit_witness(spec, d([rng.randrange(R) for _ in range(8)]).reshape(2, 4, 4), k)
    instances = [ints(inst[0]), ints(inst[1])]
    assert instances[0] != instances[1]
    proof = h.create_proof_multi(key["params"], key["pk"], adv, instances, 77, multiopen="gwc")
    assert len(proof) == proof_length(key["case"].cs, 2, "halo2", "gwc", k)
    assert h.verify_proof_multi(key["params"], key["vk"], instances, proof, trapdoor=SRS_S, multiopen="gwc")
    assert h.verify_proof_multi(key["params"], key["vk"], instances, proof, multiopen="gwc")
    assert not h.verify_proof_multi(key["params"], key["vk"], instances[::-1], proof, trapdoor=SRS_S, multiopen="gwc")
    assert not h.verify_proof_multi(key["params"], key["vk"], instances, proof, trapdoor=SRS_S)


# ---- the terms kernel against the integer twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poseidon", "merkle_sum_tree"])
def test_the_terms_kernel_equals_the_integer_twin(name):
    """B = 5 records no transcript produces, among them v = 0, u = 0, x^n = 1 and one flagged on entry; a canary row behind every
    output"""
    rows = 2
    lay, plan, omega = gc.plan_of(name, rows)
    rng = random.Random(20260)
    cases = [gc.record(lay, rows, rng), gc.record(lay, rows, rng, v=0), gc.record(lay, rows, rng, u=0),
             gc.record(lay, rows, rng, x=pow(omega, 3, R)), gc.record(lay, rows, rng)]
    B, pre_flagged, q = len(cases), 4, len(lay.groups)
    want = [gc.expected(lay, omega, case)[0] for case in cases]
    assert [w is None for w in want] == [False, False, False, True, False]
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    d_rec = up(np.stack([fr_array([ch[n_] for n_ in pl.GWC_RECORD] + [rb]) for ch, rb, _, _ in cases]))
    d_ev = up(np.stack([fr_array(evals) for _, _, evals, _ in cases]))
    d_inst = up(np.stack([fr_array(plan.instance_row(inst)) for _, _, _, inst in cases]))
    bad_in = np.zeros(B + 1, dtype=np.int32)
    bad_in[pre_flagged], bad_in[B] = 1, 0x5A5A5A5A
    d_bad = torch.from_numpy(bad_in).to(dev)
    full = lambda *shape: torch.full(shape, FILL, dtype=torch.int64, device=dev)
    d_own, d_shared, d_left = full(B + 1, lay.own_points, 4), full(B + 1, len(lay.shared_keys), 4), full(B + 1, q, 4)
    program = ev.CompiledGraph(**plan.lowered)
    try:
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.load().hm_verify_terms_gwc_dev(ctypes.c_uint64(program.handle), plan.words.ctypes.data_as(_u32p), len(plan.words),
                                                       plan.n_columns, 4, B, vp(d_rec), vp(d_ev), vp(d_inst), ctypes.cast(vp(d_bad), _u32p),
                                                       vp(d_own), vp(d_shared), vp(d_left),
                                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
    finally:
        program.destroy()
    host = lambda t: t.cpu().numpy().view(np.uint64)
    own, shared, left, bad = host(d_own), host(d_shared), host(d_left), d_bad.cpu().numpy()
    assert bad.tolist() == [0, 0, 0, 1, 1, 0x5A5A5A5A]
    for b in range(B):
        if want[b] is None or b == pre_flagged:
            assert not own[b].any() and not shared[b].any() and not left[b].any(), b
        else:
            assert np.array_equal(own[b], fr_array(want[b][0])) and np.array_equal(shared[b], fr_array(want[b][1])), b
            assert np.array_equal(left[b], fr_array(want[b][2])), b
    for t in (d_own, d_shared, d_left):
        assert (t[B] == FILL).all()


# ---- the batch verifier ---------------------------------------------------------------------------------------------------------------------
def flip(proof: bytes, at: int) -> bytes:
    return proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:]


def batch_of(key, name, encoding):
    """six proofs, [2] tampered in an evaluation (it reads, and fails) and [4] malformed (a scalar of 2^256 - 1)"""
    lay = gc.layout(name, encoding)
    proofs = [proof_of(key, name, 40 + b, encoding) for b in range(6)]
    s = lay.scalar_slots[3]
    low = 32 * s + (31 if encoding == "evm" else 0)                        # the low byte of the evaluation
    proofs[2] = flip(proofs[2], low)
    proofs[4] = proofs[4][:32 * s] + b"\xff" * 32 + proofs[4][32 * s + 32:]
    return proofs


@pytest.mark.parametrize("pairing,transcript", MODES)
@pytest.mark.parametrize("encoding", gc.ENCODINGS)
def test_batch_verifier_names_the_tampered_and_the_malformed_proof(keys, encoding, pairing, transcript):
    name = "poseidon"
    key = keys(name)
    modes = dict(pairing=pairing, transcript=transcript, encoding=encoding, multiopen="gwc")
    proofs = batch_of(key, name, encoding)
    one = h.BatchVerifier(key["params"], key["vk"], seed=3, **modes)
    one.add_proof(key["instance"], proofs[0])
    assert one.finalize() is True and one.finalize(trapdoor=SRS_S) is True and one.failing(trapdoor=SRS_S) == [] and one.msm_calls % 3 == 0
    one.close()
    bv = h.BatchVerifier(key["params"], key["vk"], seed=3, **modes)
    for proof in proofs:
        bv.add_proof(key["instance"], proof)
    assert len(bv.randomizers) == 6
    assert bv.finalize() is False and bv.finalize(trapdoor=SRS_S) is False
    assert bv.failing(trapdoor=SRS_S) == [2, 4] and bv.malformed() == [4]
    if pairing == "device":
        assert bv.failing() == [2, 4]
    assert set(bv.timings) == {"read", "plan", "transcript", "upload", "terms", "msm", "pairing", "sums", "verdict_pairing"}
    for call in (bv.verdicts, bv.proof_sums, lambda: bv.failing(method="each")):
        with pytest.raises(ValueError, match="gwc"):
            call()
    bv.close()
    clean = [p for b, p in enumerate(proofs) if b not in (2, 4)]
    assert h.verify_proofs(key["params"], key["vk"], [key["instance"]] * 4, clean, seed=9, **modes)
    assert h.verify_proofs(key["params"], key["vk"], [key["instance"]] * 4, clean, seed=9, trapdoor=SRS_S, **modes)


@pytest.mark.parametrize("name", ["merkle_sum_tree", "merkle_v3", "overflow_check_v2"])
def test_batch_verifier_on_the_other_systems(keys, name):
    key = keys(name)
    for encoding in gc.ENCODINGS:
        proofs = [proof_of(key, name, 7, encoding), flip(proof_of(key, name, 8, encoding), len(proof_of(key, name, 8, encoding)) - 1),
                  proof_of(key, name, 9, encoding)]
        bv = h.BatchVerifier(key["params"], key["vk"], seed=1, pairing="device", transcript="device", encoding=encoding, multiopen="gwc")
        for proof in proofs:
            bv.add_proof(key["instance"], proof)
        assert bv.finalize() is False and bv.failing(trapdoor=SRS_S) in ([1], ) and bv.failing() == [1]
        bv.close()
        assert h.verify_proofs(key["params"], key["vk"], [key["instance"]] * 2, [proofs[0], proofs[2]], pairing="device", transcript="device",
                               encoding=encoding, multiopen="gwc")


@pytest.mark.parametrize("encoding", gc.ENCODINGS)
@pytest.mark.parametrize("name", ["poseidon", "merkle_sum_tree"])
def test_device_records_equal_the_host_transcript_and_a_sub_range_sums_to_the_twins(keys, name, encoding):
    key = keys(name)
    c, vk = key["case"], key["vk"]
    proofs = [proof_of(key, name, 40 + b, encoding) for b in range(4)] if name == "poseidon" else [proof_of(key, name, 7 + b, encoding) for b in range(3)]
    bv = h.BatchVerifier(key["params"], vk, seed=11, transcript="device", encoding=encoding, multiopen="gwc")
    for proof in proofs:
        bv.add_proof(key["instance"], proof)
    st = bv._prepare()
    assert st["bad"] == [False] * len(proofs)
    lay = bv.layout
    records = st["d_records"].cpu().numpy().view(np.uint64)
    inst_cols = _instance_columns(c.cs, key["instance"])
    for b, proof in enumerate(proofs):
        points, _ = pl.read_proof_ints(lay, proof)
        ch = pl.transcript_challenges(lay, _vk_digest(vk), inst_cols, proof, [p[1].to_bytes(32, "little") for p in points])
        assert np.array_equal(records[b], fr_array([ch[n_] for n_ in pl.GWC_RECORD] + [bv.randomizers[b]])), b
    lo, hi = 1, len(proofs)
    left, right = bv._with_bases(lambda handle: bv._sums(handle, lo, hi))
    want_l = want_r = None
    for b in range(lo, hi):
        l_b, r_b = pl.proof_sums_ints(vk, key["instance"], proofs[b], lay, weight=bv.randomizers[b])
        want_l, want_r = g1_add(want_l, l_b), g1_add(want_r, r_b)
    assert (left, right) == (want_l, want_r)
    bv.close()


def test_the_keyword_errors_on_the_device_side(keys):
    key = keys("poseidon")
    with pytest.raises(ValueError, match="gwc"):
        h.BatchVerifier(key["params"], key["vk"], circuits=2, multiopen="gwc")
    with pytest.raises(ValueError, match="multiopen must be one of"):
        h.create_proof(key["params"], key["pk"], key["advice"], key["instance"], 1, multiopen="kzg")
