"""The EVM encoding on the GPU (csrc/keccak.inc), on proofs made here as tests/test_batch_verifier_gpu.py makes them, with
``encoding="evm"``: ``hm_keccak256_dev`` against the Python function across two wavefronts; proving and verifying, the batched
prover's bytes, the two verifiers refusing each other's proofs; ``hm_verify_read_proofs_evm_dev`` against ``read_proof_ints`` and
against the compressed read of the same points; ``hm_verify_transcript_evm_dev`` against ``transcript_challenges`` bit for bit;
``BatchVerifier(encoding="evm")`` in the four pairing x transcript modes; the solvency proofs."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, circuits, device_transcript as dt, poseidon as ps, solvency, synthesis as sy
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fr_array, g1_words
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.transcript import keccak256
from halo2_experiments_amd.verifier import _vk_digest, proof_length

import evm_cases as ec
import prover_cases as pc

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 31, 32, 33, 135, 136, 137, 271, 272, 273, 1000)
LANES = 65                                                                     # crosses a wavefront: one block of 64 lanes and one lane more
SENTINEL = 0x0123456789ABCDEF
MODES = list(itertools.product(("host", "device"), ("host", "device")))       # (pairing, transcript)
SEEDS = (7, 8, 9, 10)
u32p = ctypes.POINTER(ctypes.c_uint32)


def make_case(name):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    witnesses = [(advice, instance)]
    if name == "poseidon_k6":                                                  # a second message
        adv, inst = sy.poseidon_circuit_witness(ps.default_spec(5), pc.d([5, 6, 7, R - 1]).reshape(1, 4, 4), lay.k)
        witnesses.append((adv[0].contiguous(), pc.ints(inst[0])))
    proofs = []
    for seed in SEEDS:
        adv, inst = witnesses[seed % len(witnesses)]
        proofs.append((inst, h.create_proof(params, pk, adv, inst, seed, encoding="evm")))
    assert len({p for _, p in proofs}) == 4
    adv, inst = witnesses[SEEDS[0] % len(witnesses)]
    return dict(name=name, cs=cs, params=params, vk=vk, pk=pk, witnesses=witnesses, proofs=proofs, halo2=h.create_proof(params, pk, adv, inst, SEEDS[0]),
                layout=bvm.ProofLayout(cs, lay.k, "evm"), layout2=bvm.ProofLayout(cs, lay.k))


@pytest.fixture(scope="module")
def cases():
    made = {name: make_case(name) for name in ec.CASES}
    yield made
    for c in made.values():
        c["params"].release()


def tiled(c, count):
    return [c["proofs"][i % len(c["proofs"])] for i in range(count)]


def batch(c, members, seed=5, encoding="evm", **modes):
    bv = h.BatchVerifier(c["params"], c["vk"], seed=seed, encoding=encoding, **modes)
    for inst, proof in members:
        bv.add_proof(inst, proof)
    return bv


def message(length: int, salt: int) -> bytes:
    return bytes((5 * i + 11 * salt + (i >> 8)) & 0xFF for i in range(length))


# ---- the hash kernel -------------------------------------------------------------------------------------------------------------------------
def test_keccak_kernel_against_the_python_function():
    msgs = [message(LENGTHS[(5 * i + i // 12) % len(LENGTHS)], i) for i in range(130)]       # two wavefronts and two lanes more
    assert {len(m) for m in msgs} == set(LENGTHS)
    memo = {}
    assert dt.keccak256(msgs) == [memo.setdefault(m, keccak256(m)) for m in msgs]
    assert dt.keccak256([b"", b"abc"])[1].hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_keccak_kernel_at_odd_strides_and_lengths_past_the_stride():
    """a stride that is no multiple of 4 starts most messages off a word boundary and sends their lanes down the byte path; a length
    above the stride gives zeros and reads nothing"""
    stride, n = 139, 70                                                        # above the rate: lengths 135 .. 139 cross a block
    lens = [(37 * i) % (stride + 1) for i in range(n)]
    lens[3], lens[64], lens[5], lens[6], lens[7] = stride + 1, 1 << 31, 135, 136, 137
    raw = np.frombuffer(message(stride * n, 9), dtype=np.uint8).reshape(n, stride)
    d_msgs = torch.from_numpy(raw.copy()).cuda()
    d_lens = torch.from_numpy(np.array(lens, dtype=np.uint32).view(np.int32)).cuda()
    d_out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    assert {(d_msgs.data_ptr() + i * stride) % 4 for i in range(n)} == {0, 1, 2, 3}
    _lib.check(_lib.load().hm_keccak256_dev(ctypes.c_void_p(d_msgs.data_ptr()), stride, ctypes.cast(ctypes.c_void_p(d_lens.data_ptr()), u32p), n,
                                           ctypes.c_void_p(d_out.data_ptr()), None))
    torch.cuda.synchronize()
    got = [bytes(row) for row in d_out.cpu().numpy()]
    assert got == [bytes(32) if lens[i] > stride else keccak256(raw[i, :lens[i]].tobytes()) for i in range(n)]


# ---- prove and verify ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.CASES)
def test_evm_proofs_verify_and_the_encodings_refuse_each_other(cases, name):
    c = cases[name]
    inst, proof = c["proofs"][0]
    assert len(proof) == proof_length(c["cs"], 1, "evm") == 32 * c["layout"].slots
    assert h.verify_proof(c["params"], c["vk"], inst, proof, encoding="evm")                                   # through the pairing
    assert all(h.verify_proof(c["params"], c["vk"], i, p, trapdoor=pc.SRS_S, encoding="evm") for i, p in c["proofs"][1:])
    assert h.verify_proof(c["params"], c["vk"], inst, c["halo2"], trapdoor=pc.SRS_S)
    assert not h.verify_proof(c["params"], c["vk"], inst, c["halo2"], trapdoor=pc.SRS_S, encoding="evm")
    assert not h.verify_proof(c["params"], c["vk"], inst, proof, trapdoor=pc.SRS_S)
    # the same points and scalars in the other encoding read, and do not verify: the challenges are part of the proof
    assert not h.verify_proof(c["params"], c["vk"], inst, ec.to_evm(c["layout2"], c["halo2"]), trapdoor=pc.SRS_S, encoding="evm")
    assert not h.verify_proof(c["params"], c["vk"], inst, ec.to_halo2(c["layout"], proof), trapdoor=pc.SRS_S)
    other = c["proofs"][1][0]
    if other != inst:
        assert not h.verify_proof(c["params"], c["vk"], other, proof, trapdoor=pc.SRS_S, encoding="evm")


@pytest.mark.parametrize("name", ec.CASES)
def test_create_proofs_gives_create_proofs_bytes(cases, name):
    c = cases[name]
    picks = [c["witnesses"][seed % len(c["witnesses"])] for seed in SEEDS[:2]]
    got = h.create_proofs(c["params"], c["pk"], [adv for adv, _ in picks], [inst for _, inst in picks], list(SEEDS[:2]), encoding="evm")
    assert got == [p for _, p in c["proofs"][:2]]


@pytest.mark.parametrize("name", ec.CASES)
def test_the_two_encodings_share_the_advice_commitments_and_nothing_behind_theta(cases, name):
    c, lay, lay2, cs = cases[name], cases[name]["layout"], cases[name]["layout2"], cases[name]["cs"]
    same_seed = ec.to_halo2(lay, c["proofs"][0][1])                            # points compressed, scalars little-endian
    slots = lambda proof: [proof[32 * s:32 * s + 32] for s in range(lay2.slots)]
    a, b = slots(same_seed), slots(c["halo2"])
    A = cs.num_advice
    assert a[:A] == b[:A]                                                      # committed before any challenge
    # (a lookup of ONE input expression permutes columns that theta does not enter, with seed-derived blinding: a' and s' may agree)
    z0 = A + 2 * lay2.L
    assert lay2.nsets >= 1 and lay2.point_keys[z0] == ("perm_z", 0)
    assert all(a[s] != b[s] for s in range(z0, z0 + lay2.nsets + lay2.L))      # the grand products hang on beta and gamma
    h0 = lay2.own_index[("h_piece", 0)]
    assert all(a[s] != b[s] for s in range(h0, h0 + lay2.pieces))              # the quotient on y as well
    adv_q, _, _ = cs.queries()
    first = lay2.scalar_slots[0]
    assert all(a[first + i] != b[first + i] for i in range(len(adv_q)))        # evaluations at another x
    assert a[-2:] != b[-2:] and a[-1] != b[-1]                                 # [h], [h']


# ---- the read kernel ------------------------------------------------------------------------------------------------------------------------------
def rows_of(st, lay, B):
    """(points (B, n_points, 16 u32 as 8 u64), scalars (B, n_scalars, 4 u64)) of a prepared batch"""
    own, n_shared = lay.own_points, len(lay.shared_keys)
    bases = st["d_bases"].cpu().numpy().view(np.uint64)
    tail0 = B * own + n_shared
    points = np.stack([np.concatenate([bases[b * own:(b + 1) * own], bases[tail0 + b:tail0 + b + 1]]) for b in range(B)])
    return points, st["d_scalars"].cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", ec.CASES)
def test_read_kernel_equals_the_twin_and_the_compressed_read(cases, name):
    c, lay, lay2 = cases[name], cases[name]["layout"], cases[name]["layout2"]
    B = len(c["proofs"])
    st = batch(c, c["proofs"])._prepare()
    assert st["bad"] == [False] * B
    points, scalars = rows_of(st, lay, B)
    for b, (_, proof) in enumerate(c["proofs"]):
        pts, evals = bvm.read_proof_ints(lay, proof)
        assert np.array_equal(points[b], np.stack([g1_words(p) for p in pts])[:, :8]) and np.array_equal(scalars[b], fr_array(evals))
    # the compressed read on the same points and scalars leaves the same arrays, shared points included
    st2 = batch(c, [(inst, ec.to_halo2(lay, proof)) for inst, proof in c["proofs"]], encoding="halo2")._prepare()
    assert torch.equal(st["d_bases"], st2["d_bases"]) and torch.equal(st["d_scalars"], st2["d_scalars"])


@pytest.mark.parametrize("name", ec.CASES)
def test_read_kernel_flags_exactly_the_tampered_proofs(cases, name):
    c, lay = cases[name], cases[name]["layout"]
    inst, good = c["proofs"][0]
    bad = dict(zip((1, 2, 3, 5, 6, 7, 9, 10), ec.tampers(lay, good).values()))
    B = 12
    bv = batch(c, [(inst, bad.get(b, good)) for b in range(B)])
    st = bv._prepare()
    assert st["bad"] == [b in bad for b in range(B)] and bv.malformed() == sorted(bad)
    points, scalars = rows_of(st, lay, B)
    for b in bad:                                                              # one row differs from the good proof's, and it is zeros
        dp = [not np.array_equal(x, y) for x, y in zip(points[b], points[0])]
        ds = [not np.array_equal(x, y) for x, y in zip(scalars[b], scalars[0])]
        assert sum(dp) + sum(ds) == 1, b
        assert not (points[b][dp.index(True)] if any(dp) else scalars[b][ds.index(True)]).any(), b
    for b in set(range(B)) - set(bad):
        assert np.array_equal(points[b], points[0]) and np.array_equal(scalars[b], scalars[0])
    assert not bv.finalize(trapdoor=pc.SRS_S) and bv.failing(trapdoor=pc.SRS_S) == sorted(bad)


def test_read_kernel_keeps_inside_its_arrays(cases):
    """table entries outside their arrays, as a caller's mistake would make them: flagged, and the words behind the arrays keep their fill"""
    c, lay = cases["poseidon_k6"], cases["poseidon_k6"]["layout"]
    B, own, ns = 3, lay.own_points, lay.n_scalars
    table = lay.slot_table.copy()
    table[lay.point_slots[1]] = bvm.EVM_POINT | own                            # one past the own points
    table[lay.scalar_slots[2]] = ns                                            # one past the scalars
    raw = np.stack([np.frombuffer(p, dtype=np.uint8) for _, p in tiled(c, B)])
    d_proofs, d_table = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(table.view(np.int32)).cuda()
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device="cuda")
    d_points, d_tail, d_scalars = fill(B * own + 1, 8), fill(B + 1, 8), fill(B * ns + 1, 4)
    d_bad = torch.zeros(B, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().hm_verify_read_proofs_evm_dev(vp(d_proofs), B, ctypes.cast(vp(d_table), u32p), lay.slots, own, ns, vp(d_points), vp(d_tail),
                                                        vp(d_scalars), ctypes.cast(vp(d_bad), u32p), None))
    torch.cuda.synchronize()
    assert d_bad.cpu().tolist() == [1] * B
    for arr in (d_points, d_tail, d_scalars):
        assert (arr[-1] == SENTINEL).all()
    pts, sc = d_points.cpu().numpy().view(np.uint64)[:-1].reshape(B, own, 8), d_scalars.cpu().numpy().view(np.uint64)[:-1].reshape(B, ns, 4)
    untouched_p, untouched_s = (pts == SENTINEL).all(axis=2), (sc == SENTINEL).all(axis=2)
    assert untouched_p.sum(axis=1).tolist() == [1] * B and untouched_p[:, 1].all()     # point 1 was sent elsewhere and refused
    assert untouched_s.sum(axis=1).tolist() == [1] * B and untouched_s[:, 2].all()


# ---- the transcript kernel ----------------------------------------------------------------------------------------------------------------------
def uploaded(members):
    return torch.from_numpy(np.stack([np.frombuffer(proof, dtype=np.uint8) for _, proof in members]).copy()).cuda()


@pytest.mark.parametrize("name", ec.CASES)
def test_transcript_kernel_equals_the_host_transcripts(cases, name):
    c, lay, cs = cases[name], cases[name]["layout"], cases[name]["cs"]
    members = tiled(c, LANES)
    digest = _vk_digest(c["vk"])
    real = [bvm._instance_columns(cs, inst) for inst, _ in members]
    # lane-divergent preamble counts in one batch: the digest alone, the digest and one value, the count that puts the theta squeeze
    # on a 136-byte boundary (1 + instances + 2 advice points = 0 mod 17 words), and the proof's own instance
    count = (-(1 + 2 * cs.num_advice)) % 17 or 17
    assert 32 * (1 + count + 2 * cs.num_advice) % 136 == 0
    rng = np.random.default_rng(len(name))
    shapes = [[[]], [[int(rng.integers(1, 1 << 62))]], [[int(v) for v in rng.integers(1, 1 << 62, size=count)]], None]
    shape_of = lambda b: (b + b // 4) % 4                                       # every shape meets every proof of the tiling
    instances = [shapes[shape_of(b)] if shapes[shape_of(b)] is not None else real[b] for b in range(LANES)]
    flagged = [5, 63, 64]
    d_proofs = uploaded(members)
    d_bad = torch.zeros(LANES, dtype=torch.int32, device="cuda")
    d_bad[flagged] = 1
    d_records = torch.from_numpy(np.full((LANES, 9, 4), SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    dt.challenges(lay, digest, instances, d_proofs, None, d_bad, d_records)
    torch.cuda.synchronize()
    got = d_records.cpu().numpy().view(np.uint64)
    assert d_bad.cpu().tolist() == [int(b in flagged) for b in range(LANES)]
    assert (got[:, 8] == SENTINEL).all()                                        # the r_b element is untouched
    memo = {}
    for b, (cols, (_, proof)) in enumerate(zip(instances, members)):
        if b in flagged:
            assert not got[b, :8].any()
            continue
        key = (shape_of(b), proof)
        if key not in memo:
            ch = bvm.transcript_challenges(lay, digest, cols, proof)
            memo[key] = fr_array([ch[k] for k in bvm.RECORD])
        assert np.array_equal(got[b, :8], memo[key]), b
    assert len(memo) == 16 and len({m.tobytes() for m in memo.values()}) == 16


def test_transcript_kernel_flags_a_preamble_count_past_the_stride(cases):
    c, lay = cases["poseidon_k6"], cases["poseidon_k6"]["layout"]
    members = tiled(c, 3)
    digest = _vk_digest(c["vk"])
    d_proofs = uploaded(members)
    d_pre, d_counts = dt.upload_preamble(digest, [[[1]], [[1]], [[1]]], d_proofs.device, "evm")
    d_counts[1] = 3                                                             # the rows hold two words
    d_bad = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_records = torch.from_numpy(np.full((3, 9, 4), SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    dt.challenges(lay, digest, None, d_proofs, None, d_bad, d_records, preamble=(d_pre, d_counts))
    torch.cuda.synchronize()
    got = d_records.cpu().numpy().view(np.uint64)
    assert d_bad.cpu().tolist() == [0, 1, 0] and not got[1, :8].any() and (got[:, 8] == SENTINEL).all()
    for b in (0, 2):
        ch = bvm.transcript_challenges(lay, digest, [[1]], members[b][1])
        assert np.array_equal(got[b, :8], fr_array([ch[k] for k in bvm.RECORD]))


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 64, 65])
def test_batches_verify_in_every_mode(cases, count):
    c = cases["poseidon_k6"]
    members = tiled(c, count)
    verdicts = []
    for pairing, transcript in MODES:
        bv = batch(c, members, pairing=pairing, transcript=transcript)
        verdicts.append(bv.finalize())
        assert bv.msm_calls == 4
    assert verdicts == [True] * 4
    assert h.verify_proofs(c["params"], c["vk"], [i for i, _ in members], [p for _, p in members], seed=3, pairing="device", transcript="device",
                           encoding="evm")


@pytest.mark.parametrize("name", ec.CASES)
def test_device_mode_leaves_the_scalar_arrays_of_host_mode(cases, name):
    c = cases[name]
    members = tiled(c, 5)
    host, dev = batch(c, members), batch(c, members, transcript="device")
    a, b = host._prepare(), dev._prepare()
    assert a["bad"] == b["bad"] == [False] * 5 and host.randomizers == dev.randomizers
    for key in ("d_own", "d_shared", "d_h2_r", "d_h2_l", "d_bases", "d_scalars"):
        assert torch.equal(a[key], b[key]), key
    assert set(host.timings) == set(dev.timings)
    assert dev.finalize(trapdoor=pc.SRS_S) and host.finalize(trapdoor=pc.SRS_S)
    total = host.column_sum(1, 4)
    assert torch.equal(total, dev.column_sum(1, 4))


def test_failing_names_the_tampered_proofs_in_every_mode(cases):
    c, lay = cases["poseidon_k6"], cases["poseidon_k6"]["layout"]
    members = tiled(c, 65)
    inst, good = members[0]
    s = lay.scalar_slots[3]
    flipped = bytearray(members[7][1])
    flipped[32 * s + 30] ^= 1                                                   # an evaluation byte: reads, and does not verify
    members[7] = (members[7][0], bytes(flipped))
    members[64] = (inst, ec.put(good, lay.point_slots[0], P))                  # a malformed point
    members[30] = (inst, good[:-32])                                            # a wrong length
    lists, arrays = [], []
    for pairing, transcript in MODES:
        bv = batch(c, members, pairing=pairing, transcript=transcript)
        assert not bv.finalize()
        lists.append(bv.failing())
        assert bv.malformed() == [30, 64]
        arrays.append(bv._prepare())
    assert lists == [[7, 30, 64]] * 4
    for key in ("d_own", "d_shared", "d_h2_r", "d_h2_l"):
        assert all(torch.equal(arrays[0][key], other[key]) for other in arrays[1:]), key


# ---- solvency -------------------------------------------------------------------------------------------------------------------------------------
def test_balance_proofs_in_the_evm_encoding():
    """(max_bits, acc_cols) = (4, 4) at k = 5, two assets: the batched prover's proofs, and the commitment read from the first 64 bytes"""
    k, max_bits, acc_cols = 5, 4, 4
    cs = circuits.overflow_check_v2(max_bits, acc_cols, unblinded_value=True)
    lay = sy.RangeCheckLayout(k, max_bits, acc_cols, (1 << k) - 6)
    params = ParamsKZG.setup(k, pc.SRS_S, keep_points=True)
    try:
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        rng = np.random.default_rng(3)
        vals = [[int(v) for v in rng.integers(0, 1 << 16, size=20)] for _ in range(2)]
        proof = solvency.prove_balances(params, pk, pc.d([v for vs in vals for v in vs]).reshape(2, 20, 4), 11, encoding="evm")
        assert proof.totals == [sum(vs) for vs in vals]
        assert all(len(p) == proof_length(cs, 1, "evm") for p in proof.range_proofs)
        for com, rp in zip(proof.commitments, proof.range_proofs):
            assert rp[:64] == com[0].to_bytes(32, "big") + com[1].to_bytes(32, "big")
        assert solvency.verify_balances(params, vk, proof, encoding="evm")
        assert not solvency.verify_balances(params, vk, proof)                                 # the other encoding reads no such proof
        moved = solvency.BalanceProof(proof.commitments, list(reversed(proof.range_proofs)), proof.totals, proof.total_openings, proof.tail_openings,
                                      proof.columns)
        assert not solvency.verify_balances(params, vk, moved, encoding="evm")                 # valid range proofs of the other columns
        one = solvency.prove_balances(params, pk, pc.d(vals[0]).reshape(20, 4), 11, encoding="evm")     # one asset: create_proof
        assert one.range_proofs[0] == proof.range_proofs[0] and solvency.verify_balances(params, vk, one, encoding="evm")
    finally:
        params.release()
