"""Per-proof verdicts on the GPU.  The sums kernel through ``hm_verify_proof_sums_dev`` against the oracle of
tests/proof_sums_cases.py, bit for bit: every term count around the workgroup's 128 lanes (T = 1, no point at all, is a call the entry
refuses, so that refusal is what is checked for it), every own / shared split, one to 257 proofs, the rows that meet a doubling, a
cancellation, a zero scalar and a (0, 0) base, rows where the fold itself doubles, flagged proofs between good ones.  On the
proofs tests/test_batch_verifier_gpu.py makes -- Poseidon k = 6, MerkleTreeV3 depth 5 / k = 8, MerkleSumTree depth 5 / k = 9, whose terms cross a wavefront --:
``proof_sums()`` against the four-MSM ``_sums`` of every single proof; ``verdicts()`` against ``verify_proof`` member by member on
batches of 1, 3 and 65 with tampered members first, in the middle and last; a malformed proof beside valid ones; the four pairing x
transcript modes in both encodings; ``failing(method="each")``, ``finalize`` and ``verify_each`` against each other; and how many
launches a batch of 65 costs."""
import ctypes

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, device_pairing, poseidon as ps, synthesis as sy
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, g1_ints
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.pairing import g1_neg

import proof_sums_cases as sc
import prover_cases as pc

pytestmark = pytest.mark.gpu
CASES = ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"]
HM_ERR_BAD_ARG = -1
u32p = ctypes.POINTER(ctypes.c_uint32)


# ---- the kernel against the oracle ------------------------------------------------------------------------------------------------------
def device_rows(case):
    """the batch through the C entry -> ((B, 2, 8) uint64 rows, the words behind them, which the kernel must leave alone)"""
    dev = torch.device("cuda")
    up = lambda a, dt=np.int64: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1)).to(dev) if a.size else torch.zeros(2, dtype=torch.int64, device=dev)
    d = {key: up(case[key]) for key in ("bases", "own_s", "shared_s", "h2r", "h2l")}
    d_bad = up(case["bad"], np.int32)
    B = case["B"]
    d_out = torch.full((B * 16 + 16,), -1, dtype=torch.int64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.load().hm_verify_proof_sums_dev(vp(d["bases"]), B, case["own"], case["shared"], vp(d["own_s"]), vp(d["shared_s"]), vp(d["h2r"]),
                                             vp(d["h2l"]), ctypes.cast(vp(d_bad), u32p), vp(d_out),
                                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, _lib.load().hm_last_error()
    out = d_out.cpu().numpy()
    assert np.array_equal(d_bad.cpu().numpy().view(np.uint32), case["bad"])                  # read only
    return out[:B * 16].view(np.uint64).reshape(B, 2, 8), out[B * 16:]


def check(case, what):
    rows, behind = device_rows(case)
    assert (behind == -1).all(), what
    wrong = [b for b in range(case["B"]) if not np.array_equal(rows[b], case["expect"][b])]
    assert not wrong, (what, wrong)


@pytest.mark.parametrize("T", sc.T_LIST)
def test_kernel_equals_the_oracle_at_every_term_count(T):
    if T == 1:                                                                # no own and no shared point: not a call the entry takes
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        vp = ctypes.c_void_p(t.data_ptr())
        lib = _lib.load()
        assert lib.hm_verify_proof_sums_dev(vp, 3, 0, 0, vp, vp, vp, vp, ctypes.cast(vp, u32p), vp, None) == HM_ERR_BAD_ARG
        assert b"own_points + shared_points" in lib.hm_last_error()
        torch.cuda.synchronize()
        assert not t.any()
        return
    for own, shared in sc.splits(T):
        check(sc.build(3, own, shared, seed=T), (T, own, shared))
    own, shared = sc.splits(T)[-1]
    check(sc.build(3, own, shared, seed=(T, "bad"), bad=(1,)), (T, "a flagged proof in the middle"))


@pytest.mark.parametrize("B", [1, 65, 257])
def test_kernel_equals_the_oracle_at_every_batch_size(B):
    specials = {b: sc.SPECIALS[b % len(sc.SPECIALS)] for b in range(0, B, 3) if abs(b - B // 2) > 1}   # plain rows beside the flagged one
    case = sc.build(B, 2, 2, seed=B, specials=specials, bad=(B // 2,) if B > 1 else ())
    check(case, B)
    if B > 1:
        assert not case["expect"][B // 2].any() and case["expect"][B // 2 - 1].any() and case["expect"][B // 2 + 1].any()


@pytest.mark.parametrize("own,shared", [(2, 0), (5, 3), (130, 2)])
def test_kernel_on_rows_with_special_terms(own, shared):
    specials = {0: "double", 1: "cancel", 3: "zero scalar", 4: "zero base", 5: "all zero", 6: "double"}
    case = sc.build(7, own, shared, seed="special", specials=specials, bad=(2,))
    check(case, (own, shared))
    expect = case["expect"]
    assert not expect[2].any() and not expect[5].any() and all(expect[b, 1].any() for b in (0, 1, 3, 4, 6))


@pytest.mark.parametrize("special", sorted(sc.FOLD_DOUBLINGS))
def test_kernel_where_the_fold_meets_a_doubling(special):
    """equal partial sums in lanes t and t + off when step off runs (tests/test_proof_sums_host.py counts that these rows take
    g1_add's doubling branch in the fold, once each): same base and scalar at the first and at the last step, and one point in two
    Jacobian forms"""
    own, shared = sc.FOLD_DOUBLINGS[special]
    case = sc.build(3, own, shared, seed=special, specials={0: special, 2: special})
    check(case, special)
    assert case["expect"][0, 1].any() and case["expect"][2, 1].any()


# ---- on real proofs ----------------------------------------------------------------------------------------------------------------------
def make_case(name):
    """the proofs of tests/test_batch_verifier_gpu.py's ``make_case``, four distinct ones per circuit (for Poseidon also in the "evm"
    encoding), and a cache of what ``verify_proof`` says to a member"""
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    witnesses = [(advice, instance)]
    if name == "poseidon_k6":                                                  # a second message
        adv, inst = sy.poseidon_circuit_witness(ps.default_spec(5), pc.d([5, 6, 7, R - 1]).reshape(1, 4, 4), lay.k)
        witnesses.append((adv[0].contiguous(), pc.ints(inst[0])))
    proofs, evm = [], []
    for seed in (7, 8, 9, 10):
        adv, inst = witnesses[seed % len(witnesses)]
        proofs.append((inst, h.create_proof(params, pk, adv, inst, seed)))
        if name == "poseidon_k6" and seed < 10:
            evm.append((inst, h.create_proof(params, pk, adv, inst, seed, encoding="evm")))
    assert len({p for _, p in proofs}) == 4
    return dict(name=name, cs=cs, params=params, vk=vk, proofs=proofs, evm=evm, layout=bvm.ProofLayout(cs, lay.k), expected={})


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


def batch(c, members, seed=5, **modes):
    bv = h.BatchVerifier(c["params"], c["vk"], seed=seed, **modes)
    for inst, proof in members:
        bv.add_proof(inst, proof)
    return bv


def tiled(c, count):
    return [c["proofs"][i % len(c["proofs"])] for i in range(count)]


def expected(c, member, encoding="halo2"):
    """``verify_proof`` of one member, computed once per distinct (instance, proof) pair"""
    inst, proof = member
    key = (tuple(inst), proof, encoding)
    if key not in c["expected"]:
        c["expected"][key] = bool(h.verify_proof(c["params"], c["vk"], inst, proof, trapdoor=pc.SRS_S, encoding=encoding))
    return c["expected"][key]


TAMPERINGS = ["an evaluation", "instance", "off the curve", "scalar >= r", "length"]


def tamper(c, member, what):
    inst, proof = member
    lay = c["layout"]
    first_eval = 32 * lay.points_before_evals
    put = lambda at, data: proof[:at] + data + proof[at + 32:]
    if what == "an evaluation":
        at = first_eval + 32 * 3 + 1
        return inst, proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:]
    if what == "instance":
        return list(inst[:-1]) + [(inst[-1] + 1) % R], proof
    if what == "off the curve":
        non_residue = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) != 1)
        return inst, put(32, non_residue.to_bytes(32, "little"))
    if what == "scalar >= r":
        return inst, put(first_eval, R.to_bytes(32, "little"))
    assert what == "length"
    return inst, proof[:-32]


def test_proof_sums_equal_the_msm_route_proof_by_proof(case):
    c = case
    bv = batch(c, tiled(c, 5))
    rows = bv.proof_sums().cpu().numpy().view(np.uint64)
    assert rows.shape == (5, 2, 8) and bv.msm_calls == 0
    by_msm = bv._with_bases(lambda handle: [bv._sums(handle, b, b + 1) for b in range(5)])
    for b, (left, right) in enumerate(by_msm):
        assert left is not None and right is not None
        assert (g1_ints(rows[b, 0]), g1_neg(g1_ints(rows[b, 1]))) == (left, right), b
    bv.close()


# batch size, {position: tampering}: every kind, and first / middle / last of every size that has them
SCENARIOS = [(1, {0: "an evaluation"}), (1, {0: "length"}), (3, {0: "off the curve", 1: "scalar >= r", 2: "length"}),
             (3, {1: "an evaluation", 2: "instance"}), (65, {0: "instance", 32: "off the curve", 64: "an evaluation"}),
             (65, {0: "scalar >= r", 32: "an evaluation", 64: "length"})]
assert {what for _, where in SCENARIOS for what in where.values()} == set(TAMPERINGS)


@pytest.mark.parametrize("count,where", SCENARIOS, ids=lambda v: str(v) if isinstance(v, int) else "+".join(f"{k}:{w}" for k, w in v.items()))
def test_verdicts_equal_verify_proof_member_by_member(case, count, where):
    c = case
    members = tiled(c, count)
    for b, what in where.items():
        members[b] = tamper(c, members[b], what)
    want = [expected(c, m) for m in members]
    assert len(want) == count and all(want[b] is False for b in where) and all(want[b] for b in range(count) if b not in where)
    bv = batch(c, members)
    assert bv.verdicts(trapdoor=pc.SRS_S) == want
    bv.close()
    if count == 65:
        dev = batch(c, members, pairing="device")
        assert dev.verdicts() == want
        dev.close()


@pytest.mark.parametrize("pairing", ["host", "device"])
def test_a_malformed_proof_beside_valid_ones(poseidon, pairing):
    """the rows of a malformed proof are identities, whose pairing product is 1: its verdict must come from the flag"""
    c = poseidon
    members = tiled(c, 3)
    members[1] = tamper(c, members[1], "length")
    bv = batch(c, members, pairing=pairing)
    assert bv.verdicts() == [True, False, True] and bv.verdicts(trapdoor=pc.SRS_S) == [True, False, True]
    assert not bv.proof_sums()[1].any().item() and bv.proof_sums()[0].any().item()
    bv.close()


@pytest.mark.parametrize("encoding", ["halo2", "evm"])
@pytest.mark.parametrize("transcript", ["host", "device"])
@pytest.mark.parametrize("pairing", ["host", "device"])
def test_verdicts_in_every_mode(poseidon, pairing, transcript, encoding):
    c = poseidon
    members = list(c["evm" if encoding == "evm" else "proofs"][:3])
    inst, proof = members[1]
    members[1] = (list(inst[:-1]) + [(inst[-1] + 1) % R], proof)
    want = [expected(c, m, encoding) for m in members]
    assert want == [True, False, True]
    bv = batch(c, members, pairing=pairing, transcript=transcript, encoding=encoding)
    assert bv.verdicts() == want and bv.verdicts(trapdoor=pc.SRS_S) == want
    assert {"sums", "verdict_pairing"} <= set(bv.timings) and bv.timings["verdict_pairing"] > 0
    bv.close()


def test_each_bisect_finalize_and_verify_each_agree(case):
    c = case
    members = tiled(c, 6)
    members[1] = tamper(c, members[1], "an evaluation")
    members[4] = tamper(c, members[4], "length")
    for group in (members, tiled(c, 3), []):
        bv = batch(c, group)
        verdicts = bv.verdicts(trapdoor=pc.SRS_S)
        assert bv.failing(trapdoor=pc.SRS_S, method="each") == bv.failing(trapdoor=pc.SRS_S) == [b for b, ok in enumerate(verdicts) if not ok]
        assert all(verdicts) == bv.finalize(trapdoor=pc.SRS_S)
        each = h.verify_each(c["params"], c["vk"], [i for i, _ in group], [p for _, p in group], seed=9, trapdoor=pc.SRS_S)
        assert each == verdicts                                               # another seed, other weights: the same verdicts
        bv.close()
    dev = batch(c, members, pairing="device")
    assert dev.failing(method="each") == dev.failing() == [1, 4] and not dev.finalize()
    assert h.verify_each(c["params"], c["vk"], [i for i, _ in members], [p for _, p in members], pairing="device", transcript="device") \
        == [b not in (1, 4) for b in range(6)]
    with pytest.raises(ValueError):
        dev.failing(method="all")
    with pytest.raises(ValueError):
        h.verify_each(c["params"], c["vk"], [members[0][0]], [])
    dev.close()


def test_launches_of_a_batch_of_65(poseidon, monkeypatch):
    c = poseidon
    members = tiled(c, 65)
    members[7] = tamper(c, members[7], "an evaluation")
    members[40] = tamper(c, members[40], "length")
    calls = []
    real = device_pairing.run_device
    monkeypatch.setattr(device_pairing, "run_device", lambda *a, **kw: calls.append(int(a[3])) or real(*a, **kw))
    bv = batch(c, members, pairing="device")
    before = bv.msm_calls
    first = bv.verdicts()
    assert first == [b not in (7, 40) for b in range(65)]
    assert calls == [64] and bv.sums_calls == 1 and bv.msm_calls == before     # one pairing call over the well-formed proofs, no MSM
    assert bv.verdicts() == first and bv.sums_calls == 1 and calls == [64, 64]  # the sums are kept with the prepared state
    bv.add_proof(*c["proofs"][0])                                             # a new member: a new state, new sums
    assert bv.verdicts() == first + [True] and bv.sums_calls == 2
    bv.close()


def test_a_batch_of_malformed_proofs_launches_nothing(poseidon, monkeypatch):
    c = poseidon
    inst, proof = c["proofs"][0]
    calls = []
    monkeypatch.setattr(device_pairing, "run_device", lambda *a, **kw: calls.append(a))
    bv = batch(c, [(inst, proof[:-32]), (inst, proof[:32] + bytes(32) + proof[64:]), (inst, b"")], pairing="device")
    assert bv.verdicts() == [False] * 3 and bv.verdicts(trapdoor=pc.SRS_S) == [False] * 3 and bv.failing(method="each") == [0, 1, 2]
    assert not bv.proof_sums().any().item() and bv.sums_calls == 0 and bv.msm_calls == 0 and calls == []
    bv.close()


def test_run_device_refuses_tensors_it_cannot_hand_to_the_library(poseidon):
    c = poseidon
    bv = batch(c, tiled(c, 4), pairing="device")
    rows = bv.proof_sums()
    n = 4
    d_g1 = rows.reshape(2 * n, 8)
    d_g2 = torch.from_numpy(np.frombuffer(bytes(c["params"].s_g2) + bytes(c["params"].g2), dtype=np.int64).reshape(2, 16).copy()).to(rows.device).repeat(n, 1)
    d_off = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=rows.device)
    assert device_pairing.run_device(d_g1, d_g2, d_off, n).cpu().tolist() == [1] * n
    wide = torch.zeros((2 * n, 16), dtype=torch.int64, device=rows.device)
    for g1, g2, off, checks in [(wide[:, :8], d_g2, d_off, n),                   # a strided view
                                (d_g1, d_g2[::2], d_off[:n // 2 + 1], n // 2),      # likewise, and one G2 point per two G1 points
                                (d_g1.to(torch.int32), d_g2, d_off, n), (d_g1, d_g2, d_off.to(torch.int64), n),
                                (d_g1.cpu(), d_g2, d_off, n), (d_g1, d_g2.cpu(), d_off, n), (d_g1.reshape(-1), d_g2, d_off, n),
                                (d_g1, d_g2[:, :8].contiguous(), d_off, n), (d_g1, d_g2, d_off[:-1], n), (d_g1[:0], d_g2[:0], d_off[:1], 0)]:
        with pytest.raises(ValueError):
            device_pairing.run_device(g1, g2, off, checks)
    empty = batch(c, [])
    assert tuple(empty.proof_sums().shape) == (0, 2, 8) and empty.sums_calls == 0
    bv.close()
