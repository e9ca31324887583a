"""BatchVerifier on the GPU, on proofs made here as tests/test_prover_gpu.py makes them: Poseidon at k = 6 (two messages), MerkleTreeV3
depth 5 at k = 8 (no lookups, two permutation sets) and MerkleSumTree depth 5 at k = 9 (8 lookups, 3 sets, 34 advice queries), about four
distinct proofs each.  The read kernel against ``transcript.g1_decompress_int``, slot by slot, and its flags; the scalar arrays the sums
read against r_b x the integer twin; batches of 1 .. 257 proofs (257 crosses a wavefront and a 256-thread block) through the pairing
and the trapdoor; tampered proofs named by ``failing()``; the column sums over sub-ranges; a batch of malformed proofs only."""
import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import batch_verifier as bvm, poseidon as ps, synthesis as sy
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fq_ints, fr_ints
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG

import prover_cases as pc

pytestmark = pytest.mark.gpu
CASES = ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"]


def make_case(name):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    witnesses = [(advice, instance)]
    if name == "poseidon_k6":                                                  # a second message
        spec = ps.default_spec(5)
        adv, inst = sy.poseidon_circuit_witness(spec, pc.d([5, 6, 7, R - 1]).reshape(1, 4, 4), lay.k)
        witnesses.append((adv[0].contiguous(), pc.ints(inst[0])))
    proofs = []
    for seed in (7, 8, 9, 10):
        adv, inst = witnesses[seed % len(witnesses)]
        proofs.append((inst, h.create_proof(params, pk, adv, inst, seed)))
    assert len({p for _, p in proofs}) == 4
    return dict(name=name, cs=cs, params=params, vk=vk, proofs=proofs, layout=bvm.ProofLayout(cs, lay.k))


@pytest.fixture(scope="module", params=CASES)
def case(request):
    c = make_case(request.param)
    yield c
    c["params"].release()


@pytest.fixture(scope="module")
def poseidon():
    c = make_case("poseidon_k6")
    yield c
    c["params"].release()


def batch(c, proofs, seed=5):
    bv = h.BatchVerifier(c["params"], c["vk"], seed=seed)
    for inst, proof in proofs:
        bv.add_proof(inst, proof)
    return bv


def tiled(c, count):
    return [c["proofs"][i % len(c["proofs"])] for i in range(count)]


def flipped(proof, at):
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


def put(proof, at, data):
    return proof[:at] + data + proof[at + 32:]


# ---- the read kernel -------------------------------------------------------------------------------------------------------------------
def test_read_kernel_equals_the_host_decompression(case):
    c, lay = case, case["layout"]
    bv = batch(c, c["proofs"])
    st = bv._prepare()
    B, own = len(c["proofs"]), lay.own_points
    assert st["bad"] == [False] * B
    bases = st["d_bases"].cpu().numpy().view(np.uint64)
    scalars = st["d_scalars"].cpu().numpy().view(np.uint64)
    tail0 = B * own + len(lay.shared_keys)
    for b, (_, proof) in enumerate(c["proofs"]):
        points, evals = bvm.read_proof_ints(lay, proof)
        rows = np.concatenate([bases[b * own:(b + 1) * own], bases[tail0 + b:tail0 + b + 1]])
        assert [tuple(fq_ints(row.reshape(2, 4))) for row in rows] == points
        assert [int.from_bytes(bytes(y), "little") for y in st["ybytes"][b]] == [y for _, y in points]
        assert fr_ints(scalars[b]) == evals
    shared = bases[B * own:tail0]
    assert [None if not row.any() else tuple(fq_ints(row.reshape(2, 4))) for row in shared] == bvm.shared_points(c["vk"], lay)


def test_read_kernel_flags_the_right_proof_only(case):
    c, lay = case, case["layout"]
    good = c["proofs"][0][1]
    non_residue = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) != 1)
    first_eval, last_eval = 32 * lay.points_before_evals, 32 * (lay.points_before_evals + lay.n_scalars - 1)
    bad = {1: put(good, 0, P.to_bytes(32, "little")), 2: put(good, 32, non_residue.to_bytes(32, "little")),
           3: put(good, len(good) - 32, bytes(32)), 5: put(good, first_eval, R.to_bytes(32, "little")),
           6: put(good, last_eval, (2 ** 256 - 1).to_bytes(32, "little")), 7: put(good, len(good) - 64, bytes(32))}
    inst = c["proofs"][0][0]
    bv = batch(c, [(inst, bad.get(b, good)) for b in range(9)])
    assert bv._prepare()["bad"] == [b in bad for b in range(9)] and bv.malformed() == sorted(bad)
    assert not bv.finalize(trapdoor=pc.SRS_S) and bv.failing(trapdoor=pc.SRS_S) == sorted(bad)


# ---- the scalars the sums read ---------------------------------------------------------------------------------------------------------
def test_scalar_arrays_equal_the_weighted_twin(case):
    c, lay = case, case["layout"]
    proofs = c["proofs"][:3]
    bv = batch(c, proofs)
    st = bv._prepare()
    own = lay.own_points
    got_own = fr_ints(st["d_own"].cpu().numpy().view(np.uint64))
    got_shared = fr_ints(st["d_shared"].cpu().numpy().view(np.uint64))
    got_r, got_l = fr_ints(st["d_h2_r"].cpu().numpy().view(np.uint64)), fr_ints(st["d_h2_l"].cpu().numpy().view(np.uint64))
    for b, (inst, proof) in enumerate(proofs):
        _, o, s, _ = bvm.proof_terms_ints(c["vk"], inst, proof, lay)
        rb = bv.randomizers[b]
        assert got_own[b * own:(b + 1) * own] == [rb * v % R for v in o[:own]]
        assert got_shared[b * len(s):(b + 1) * len(s)] == [rb * v % R for v in s]
        assert (got_r[b], got_l[b]) == (rb * o[own] % R, rb)


def test_both_transcript_modes_prepare_one_state(poseidon):
    """one preparation for both modes: the same keys, every device array equal, ybytes / preamble filled in their own mode only"""
    c = poseidon
    members = tiled(c, 5)
    members[3] = (members[3][0], put(members[3][1], 0, P.to_bytes(32, "little")))            # a malformed point
    states = {}
    for mode in ("host", "device"):
        bv = h.BatchVerifier(c["params"], c["vk"], seed=5, transcript=mode)
        for inst, proof in members:
            bv.add_proof(inst, proof)
        states[mode] = bv._prepare()
    a, b = states["host"], states["device"]
    assert set(a) == set(b) == {"B", "bad", "d_bases", "d_scalars", "d_own", "d_shared", "d_h2_r", "d_h2_l", "d_sum", "d_bad", "d_ybytes",
                                "d_proofs", "d_table", "d_records", "d_inst", "plan", "ybytes", "preamble"}
    assert a["B"] == b["B"] == 5 and a["bad"] == b["bad"] == [False, False, False, True, False]
    for key in a:
        if key.startswith("d_"):
            assert torch.equal(a[key], b[key]), key
    assert a["ybytes"] is not None and b["ybytes"] is None and a["preamble"] is None and b["preamble"] is not None
    assert np.array_equal(a["ybytes"], b["d_ybytes"].cpu().numpy())


# ---- whole batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 257])
def test_valid_batches(poseidon, count):
    c = poseidon
    bv = batch(c, tiled(c, count))
    assert bv.finalize(trapdoor=pc.SRS_S) and bv.failing(trapdoor=pc.SRS_S) == []
    if count in (1, 3, 65):
        assert bv.finalize()                                                    # the pairing agrees with the trapdoor
    assert len(bv.randomizers) == count


def test_valid_batch_of_each_circuit_and_verify_proofs(case):
    c = case
    insts, proofs = [i for i, _ in c["proofs"]], [p for _, p in c["proofs"]]
    assert h.verify_proofs(c["params"], c["vk"], insts, proofs, seed=3, trapdoor=pc.SRS_S)
    assert h.verify_proofs(c["params"], c["vk"], insts, proofs)                 # unseeded, through the pairing


def test_one_check_agrees_with_verify_proof_per_proof(case):
    c = case
    (i0, p0), (i1, p1), (i2, p2), (i3, p3) = c["proofs"]
    lay = c["layout"]
    wrong = list(i1)
    wrong[-1] = (wrong[-1] + 1) % R
    members = [(i0, p0), (wrong, p1), (i2, flipped(p2, 32 * lay.points_before_evals + 32 * 3 + 1)), (i3, p3), (i0, p1), (i1, p1),
               (i2, p2[:-32]), (i3, flipped(p3, len(p3) - 32))]
    each = [h.verify_proof(c["params"], c["vk"], inst, proof, trapdoor=pc.SRS_S) for inst, proof in members]
    assert each[0] and each[3] and each[5] and not each[1] and not each[2] and not each[6]
    bv = batch(c, members)
    assert bv.finalize(trapdoor=pc.SRS_S) == all(each)
    assert bv.failing(trapdoor=pc.SRS_S) == [b for b, ok in enumerate(each) if not ok]
    good = [m for m, ok in zip(members, each) if ok]
    assert batch(c, good).finalize(trapdoor=pc.SRS_S) and batch(c, good).finalize()


TAMPERINGS = ["an evaluation", "first commitment", "last point", "instance", "truncated", "one byte more"]


def tamper(c, member, what):
    inst, proof = member
    lay = c["layout"]
    if what == "an evaluation":
        return inst, flipped(proof, 32 * lay.points_before_evals + 32 * 3 + 1)
    if what == "first commitment":
        return inst, flipped(proof, 0)
    if what == "last point":
        return inst, flipped(proof, len(proof) - 32)
    if what == "instance":
        return [(inst[0] + 1) % R] + list(inst[1:]), proof
    if what == "truncated":
        return inst, proof[:-32]
    return inst, proof + b"\0"


TAMPER_CASES = [(257, (0,), "an evaluation"), (257, (63, 64), "first commitment"), (257, (256,), "last point"), (257, (64, 256), "instance"),
                (65, (0, 64), "truncated"), (65, (63,), "one byte more"), (65, (63, 64), "an evaluation"), (64, (63,), "instance"),
                (65, (0,), "last point"), (257, (0, 63), "truncated"), (257, (64,), "one byte more"), (65, (64,), "first commitment")]
assert {what for _, _, what in TAMPER_CASES} == set(TAMPERINGS)


@pytest.mark.parametrize("count,where,what", TAMPER_CASES)
def test_tampered_proofs_are_named(poseidon, count, where, what):
    c = poseidon
    members = tiled(c, count)
    for b in where:
        members[b] = tamper(c, members[b], what)
    bv = batch(c, members)
    assert not bv.finalize(trapdoor=pc.SRS_S)
    before = bv.msm_calls
    assert bv.failing(trapdoor=pc.SRS_S) == list(where)
    assert (bv.msm_calls - before) // 4 <= 2 * len(where) * (count.bit_length() + 1) + 1      # O(f log B) checks, not B


@pytest.mark.parametrize("what", ["an evaluation", "instance"])
def test_tampered_proof_through_the_pairing(case, what):
    c = case
    members = list(c["proofs"][:3])
    members[1] = tamper(c, members[1], what)
    bv = batch(c, members, seed=None)
    assert not bv.finalize() and bv.failing() == [1]


# ---- the column sums -------------------------------------------------------------------------------------------------------------------
def test_column_sums_over_sub_ranges(poseidon):
    c, lay = poseidon, poseidon["layout"]
    members = tiled(c, 257)
    members[70] = tamper(c, members[70], "truncated")                          # a malformed proof holds a zero row
    bv = batch(c, members)
    st = bv._prepare()
    n_shared = len(lay.shared_keys)
    rows = np.array(fr_ints(st["d_shared"].cpu().numpy().view(np.uint64)), dtype=object).reshape(257, n_shared)
    assert not rows[70].any() and rows[69].any()
    for lo, hi in [(0, 1), (1, 65), (64, 257), (0, 257), (5, 5)]:
        got = fr_ints(bv.column_sum(lo, hi).cpu().numpy().view(np.uint64))
        assert got == [int(sum(rows[lo:hi, col])) % R for col in range(n_shared)], (lo, hi)


def test_a_batch_of_malformed_proofs_launches_no_msm(poseidon):
    c = poseidon
    inst, proof = c["proofs"][0]
    bv = batch(c, [(inst, proof[:-32]), (inst, put(proof, 0, bytes(32))), (inst, b"")])
    assert not bv.finalize(trapdoor=pc.SRS_S) and not bv.finalize()
    assert bv.failing(trapdoor=pc.SRS_S) == [0, 1, 2] and bv.msm_calls == 0


def test_terms_entry_refuses_an_unknown_program_and_foreign_counts(poseidon):
    import ctypes
    from halo2_experiments_amd import _lib
    c = poseidon
    bv = batch(c, c["proofs"][:1])
    assert bv.finalize(trapdoor=pc.SRS_S)
    plan = next(iter(bv._plans.values()))
    lib, u32p = _lib.load(), ctypes.POINTER(ctypes.c_uint32)
    t = torch.zeros((4096, 4), dtype=torch.int64, device="cuda")              # never written: every call below is refused
    vp = ctypes.c_void_p(t.data_ptr())
    call = lambda handle, cols, dyn: lib.hm_verify_terms_dev(ctypes.c_uint64(handle), plan.words.ctypes.data_as(u32p), len(plan.words), cols, dyn, 1,
                                                             vp, vp, vp, ctypes.cast(vp, u32p), vp, vp, vp, vp, None)
    assert call(0xDEAD, plan.n_columns, 4) == -1 and b"unknown program handle" in lib.hm_last_error()
    assert call(bv._program.handle, plan.n_columns, 3) == -1 and call(bv._program.handle, plan.n_columns + 1, 4) == -1
    torch.cuda.synchronize()
    assert not t.any()
    bv.close()
    assert bv._program is None
