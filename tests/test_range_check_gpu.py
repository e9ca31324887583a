"""The range-check circuit on the GPU: synthesis.range_witness word for word against RangeCheckLayout.assign_ints (limbs inside and
across 64-bit words, every usable row, the counter of the values that do not fit), the device MockProver on a batch, keygen /
create_proof / verify_proof / verify_proofs with and without the unblinded value column, and the solvency statement of
halo2_experiments_amd.solvency with its rejections.  Keys, parameters and proofs are made once per shape and shared, never changed."""
import ctypes

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, circuits, poseidon as ps, solvency, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.transcript import g1_decompress_int

from range_check_cases import values as case_values

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
RC = sy.RangeCheckLayout
GATE = "equality check between decomposed value and value"


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def words(columns):
    return sy.columns_to_words(columns)


def in_range(max_bits, acc_cols, rows, seed):
    """`rows` values that fit: the case list with what does not fit masked down"""
    mask = (1 << (max_bits * acc_cols)) - 1
    return [v & mask for v in case_values(max_bits, acc_cols, rows, seed)]


# ---- the witness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, max_bits, acc_cols, rows", [(5, 4, 4, 3), (5, 4, 4, 26), (13, 12, 6, 100), (9, 8, 31, 100)])
def test_witness_equals_assign_ints(k, max_bits, acc_cols, rows):
    m, lay = 3, RC(k, max_bits, acc_cols, rows)
    vals = [case_values(max_bits, acc_cols, rows, seed=10 * k + c) for c in range(m)]
    if rows == 3:
        vals[0] = [65534, 1, 65535]                          # the reference's two cases
        vals[1] = [65534, 3, 65537]
    dv = d([v for vs in vals for v in vs]).reshape(m, rows, 4)
    out = torch.full((m, 1 + acc_cols, 1 << k, 4), -1, dtype=torch.int64, device="cuda")       # every word must be written
    adv, over = sy.range_witness(dv, k, max_bits, acc_cols, out=out)
    assert adv.data_ptr() == out.data_ptr()
    got = adv.cpu().numpy().view(np.uint64)
    for c in range(m):
        assert np.array_equal(got[c], words(lay.assign_ints(vals[c]))), c
    assert not got[:, :, rows:].any()
    assert over.cpu().tolist() == [sum(v >> (max_bits * acc_cols) != 0 for v in vs) for vs in vals]
    assert rows == 3 or min(over.cpu().tolist()) >= 2        # 2^bits and r - 1 are among the values
    host_adv, host_over = sy.range_witness_host(dv.cpu().numpy().view(np.uint64), k, max_bits, acc_cols)
    assert np.array_equal(host_adv, got) and host_over.tolist() == over.cpu().tolist()
    one, over1 = sy.range_witness(dv[1], k, max_bits, acc_cols)                                 # (rows, 4): one circuit
    assert np.array_equal(one.cpu().numpy().view(np.uint64)[0], got[1]) and over1.cpu().tolist() == over.cpu().tolist()[1:2]


def test_witness_of_every_usable_row_at_k17():
    """(16, 4) at k = 17, rows = 2^17 - 6, m = 3: the limbs by numpy from the plain values (assign_ints would take a minute); the
    value column is the input, the tail rows are zero, the counter counts"""
    k, max_bits, acc_cols, m = 17, 16, 4, 3
    n, rows = 1 << k, (1 << k) - 6
    rng = np.random.default_rng(17)
    plain = rng.integers(0, 1 << 63, size=(m, rows), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(m, rows), dtype=np.uint64)
    special = case_values(max_bits, acc_cols, 16, seed=1)
    too_big = [i for i, v in enumerate(special) if v >> 64]
    vals = ps.ints_to_words([int(v) for v in plain.reshape(-1)]).reshape(m, rows, 4)
    vals[1, :16] = ps.ints_to_words(special)                 # circuit 1 starts with the case list: r - 1, single bits above 2^64 ...
    dv = torch.from_numpy(vals.view(np.int64)).cuda()
    adv, over = sy.range_witness(dv, k, max_bits, acc_cols)
    got = adv.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:, 0, :rows], vals) and not got[:, :, rows:].any()
    assert over.cpu().tolist() == [0, len(too_big), 0]
    small = np.array([ps.ints_to_words(list(range(1 << 16)))])[0]                               # Montgomery words of every limb
    low = plain.copy()
    low[1, :16] = np.array([v & ((1 << 64) - 1) for v in special], dtype=np.uint64)
    for i in range(acc_cols):
        limb = (low >> np.uint64(16 * (acc_cols - 1 - i))) & np.uint64(0xFFFF)
        assert np.array_equal(got[:, 1 + i, :rows], small[limb.astype(np.int64)]), i


def test_witness_bad_arguments_leave_the_output_untouched():
    lib = _lib.load()
    dv = d([1, 2, 3]).reshape(1, 3, 4)
    out = torch.full((1, 5, 32, 4), -1, dtype=torch.int64, device="cuda")
    over = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    O = ctypes.cast(ctypes.c_void_p(over.data_ptr()), ctypes.POINTER(ctypes.c_uint32))
    call = lambda max_bits=4, acc_cols=4, log_n=5, m=1, rows=3, v=P(dv), a=P(out), o=O: lib.hm_range_witness_bn256_fr_dev(
        max_bits, acc_cols, log_n, m, rows, v, a, o, None)
    bad = [call(max_bits=0), call(max_bits=17), call(acc_cols=0), call(max_bits=16, acc_cols=16), call(log_n=25), call(rows=0), call(rows=27),
           call(max_bits=5, log_n=5), call(m=0), call(v=None), call(a=None), call(v=P(dv, 8)), call(a=P(out, 8)),
           call(o=ctypes.cast(ctypes.c_void_p(over.data_ptr() + 2), ctypes.POINTER(ctypes.c_uint32))), call(v=P(out, 64))]
    assert bad == [-1] * len(bad)
    hv = dv.cpu().numpy().view(np.uint64)
    hadv = np.full((1, 5, 32, 4), 9, dtype=np.uint64)
    u64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.hm_range_witness_bn256_fr(4, 4, 5, 1, 27, u64(hv), u64(hadv), None) == -1
    assert lib.hm_range_witness_bn256_fr(4, 4, 24, 1, 3, u64(hv), u64(hadv), None) == -1       # more than 256 MiB of columns
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and over.cpu().tolist() == [77] and (hadv == 9).all()
    assert call() == 0 and call(o=None) == 0
    torch.cuda.synchronize()
    assert over.cpu().tolist() == [0] and not bool((out == -1).any())
    with pytest.raises(ValueError):
        sy.range_witness(dv.cpu(), 5)
    with pytest.raises(ValueError):
        sy.range_witness(dv, 5, out=torch.zeros((1, 5, 16, 4), dtype=torch.int64, device="cuda"))


# ---- the device MockProver ----------------------------------------------------------------------------------------------------------
def test_device_mock_prover_names_what_fails():
    k, rows, m = 5, 26, 3
    lay, cs = RC(k, 4, 4, rows), circuits.overflow_check_v2(4, 4)
    vals = [in_range(4, 4, rows, seed=c) for c in range(m)]
    adv, over = sy.range_witness(d([v for vs in vals for v in vs]).reshape(m, rows, 4), k, 4, 4)
    assert over.cpu().tolist() == [0, 0, 0]
    mp = h.MockProver(cs, lay)
    mp.assert_satisfied(adv)                                 # the instance column holds nothing: None
    assert mp.verify(adv, [[]]).ok and mp.verify(adv, [torch.zeros((m, 0, 4), dtype=torch.int64, device="cuda")]).ok
    bad = adv.clone()
    bad[1, 3, 7] = d([16])[0]                                # limb column 3 (lookup 2) of circuit 1, row 7 ...
    bad[1, 0, 7] = d([(sum(ps.words_to_ints(adv[1, 1 + i, 7:8].cpu().numpy().view(np.uint64))[0] << (4 * (3 - i)) for i in (0, 1, 3))
                       + (16 << 4)) % R])[0]                 # ... with the value adjusted: the gate holds
    res = mp.verify(bad)
    assert not res.ok and res.failures == [("lookup", 1, 2, 7)] and res.users_failed == [1]
    big = list(vals[2])
    big[5] = (1 << 16) + 5
    adv2, over2 = sy.range_witness(d(vals[0] + vals[1] + big).reshape(m, rows, 4), k, 4, 4)
    assert over2.cpu().tolist() == [0, 0, 1]
    res = mp.verify(adv2)
    assert res.failures == [("gate", 2, GATE, 0, 5)] and res.total == {"gate": 1, "copy": 0, "lookup": 0}
    with pytest.raises(h.NotSatisfied):
        mp.assert_satisfied(adv2)


# ---- proving at (4, 4, k = 5), every usable row ----------------------------------------------------------------------------------------
K5, ROWS5 = 5, 26


@pytest.fixture(scope="module")
def k5():
    params = ParamsKZG.setup(K5, SRS_S, keep_points=True)
    lay = RC(K5, 4, 4, ROWS5)
    keys = {}
    for unblinded in (False, True):
        cs = circuits.overflow_check_v2(4, 4, unblinded_value=unblinded)
        vk = h.keygen_vk(params, cs, lay)
        keys[unblinded] = (cs, vk, h.keygen_pk(params, vk, cs, lay, cosets=False))
    vals = [in_range(4, 4, ROWS5, seed=50 + c) for c in range(3)]
    adv, _ = sy.range_witness(d([v for vs in vals for v in vs]).reshape(3, ROWS5, 4), K5, 4, 4)
    proofs = {u: [h.create_proof(params, keys[u][2], adv[c], [[]], 20 + c) for c in range(3)] for u in (False, True)}
    return dict(params=params, lay=lay, keys=keys, vals=vals, adv=adv, proofs=proofs)


def test_proofs_verify(k5):
    p = k5["params"]
    for u in (False, True):
        cs, vk, pk = k5["keys"][u]
        assert len(k5["proofs"][u][0]) == h.verifier.proof_length(cs)
        assert h.verify_proof(p, vk, [[]], k5["proofs"][u][0]) and h.verify_proof(p, vk, [[]], k5["proofs"][u][1], trapdoor=SRS_S)
        assert h.verify_proofs(p, vk, [[[]]] * 3, k5["proofs"][u], seed=5)
        assert h.create_proofs(p, pk, k5["adv"], [[[]]] * 3, [20, 21, 22]) == k5["proofs"][u]
        flipped = bytearray(k5["proofs"][u][2])
        flipped[-1] ^= 1
        assert not h.verify_proof(p, vk, [[]], bytes(flipped), trapdoor=SRS_S)
        assert not h.verify_proofs(p, vk, [[[]]] * 3, k5["proofs"][u][:2] + [bytes(flipped)], seed=5)


def test_unblinded_value_commitment_is_commit_lagrange(k5):
    p, col = k5["params"], k5["adv"][0, 0].contiguous()
    assert not bool(col[ROWS5:].any())
    expected = h.bn256.g1_ints(p.commit_lagrange(col))
    assert g1_decompress_int(k5["proofs"][True][0][:32]) == expected
    assert g1_decompress_int(k5["proofs"][False][0][:32]) != expected
    # the other columns are blinded as before: the limb commitments of the two proofs agree, slot for slot
    assert k5["proofs"][True][0][32:5 * 32] == k5["proofs"][False][0][32:5 * 32]


def test_too_large_a_value_is_rejected(k5):
    p = k5["params"]
    vals = list(k5["vals"][0])
    vals[3] = 1 << 16
    adv, over = sy.range_witness(d(vals).reshape(1, ROWS5, 4), K5, 4, 4)
    assert over.cpu().tolist() == [1]
    for u in (False, True):
        cs, vk, pk = k5["keys"][u]
        assert not h.verify_proof(p, vk, [[]], h.create_proof(p, pk, adv[0], [[]], 9), trapdoor=SRS_S)


# ---- the solvency statement ------------------------------------------------------------------------------------------------------------
def _solvency_case(k, max_bits, acc_cols, users, assets, params=None, keys=None):
    if params is None:
        params = ParamsKZG.setup(k, SRS_S, keep_points=True)
        cs = circuits.overflow_check_v2(max_bits, acc_cols, unblinded_value=True)
        lay = RC(k, max_bits, acc_cols, (1 << k) - 6)        # every usable row is under the selector
        vk = h.keygen_vk(params, cs, lay)
        keys = (cs, vk, h.keygen_pk(params, vk, cs, lay, cosets=False))
    vals = [in_range(max_bits, acc_cols, users, seed=900 + a) for a in range(assets)]
    bal = d([v for vs in vals for v in vs]).reshape(assets, users, 4)
    proof = h.prove_balances(params, keys[2], bal[0] if assets == 1 else bal, seed=33)
    return dict(params=params, keys=keys, vals=vals, bal=bal, proof=proof, openings=h.user_openings(params, proof), k=k, users=users)


@pytest.fixture(scope="module")
def sol5(k5):
    return _solvency_case(K5, 4, 4, 26, 1, k5["params"], k5["keys"][True])


@pytest.fixture(scope="module")
def sol13():
    return _solvency_case(13, 12, 6, 100, 2)


def _check_statement(c):
    params, (cs, vk, pk), proof = c["params"], c["keys"], c["proof"]
    n, assets = 1 << c["k"], len(c["vals"])
    assert proof.totals == [sum(vs) for vs in c["vals"]]
    assert len(proof.commitments) == len(proof.range_proofs) == len(proof.total_openings) == assets
    assert h.verify_balances(params, vk, proof) and h.verify_balances(params, vk, proof, pairing="device", tail=True)
    assert tuple(c["openings"].shape) == (assets, n, 8)
    for a in range(assets):
        padded = c["vals"][a] + [0] * (n - c["users"])
        rows = sorted(set(range(c["users"])) | {c["users"], n - 7} | set(range(n - 6, n)))     # every user, two zero rows, the 6 tail rows
        every = h.verify_users(params, proof.commitments[a], rows, [padded[i] for i in rows], c["openings"][a][rows], pairing="device")
        assert every == [True] * len(rows)                   # every user's own check, in one launch chain
        for i in (0, c["users"] - 1, n - 1):
            assert h.verify_user(params, proof.commitments[a], i, padded[i], c["openings"][a, i])
    return True


def test_solvency_26_users(sol5):
    assert _check_statement(sol5)
    # user_openings from the balances alone gives the same openings
    assert torch.equal(h.user_openings(sol5["params"], sol5["bal"][0]), sol5["openings"][0])


def test_solvency_two_assets_100_users(sol13):
    assert _check_statement(sol13)


def test_solvency_rejections(sol5):
    c = sol5
    params, (cs, vk, pk), proof = c["params"], c["keys"], c["proof"]
    replace = lambda **kw: solvency.BalanceProof(**{**{f: getattr(proof, f) for f in ("commitments", "range_proofs", "totals", "total_openings",
                                                                                    "tail_openings", "columns")}, **kw})
    assert h.verify_balances(params, vk, replace())
    assert not h.verify_balances(params, vk, replace(totals=[proof.totals[0] + 1]))
    assert not h.verify_balances(params, vk, replace(totals=[proof.totals[0] - 1]))
    other = h.prove_balances(params, pk, d([v ^ 1 for v in c["vals"][0]]).reshape(26, 4), seed=34)
    assert h.verify_balances(params, vk, other) and other.commitments != proof.commitments
    assert not h.verify_balances(params, vk, replace(commitments=other.commitments))
    assert not h.verify_balances(params, vk, replace(range_proofs=other.range_proofs))
    assert not h.verify_balances(params, vk, replace(total_openings=other.total_openings))
    for i in (0, 25):
        assert not h.verify_user(params, proof.commitments[0], i, c["vals"][0][i] + 1, c["openings"][0, i])
        assert not h.verify_user(params, proof.commitments[0], i, c["vals"][0][i], c["openings"][0, (i + 1) % 26])
    assert h.verify_users(params, proof.commitments[0], [3, 4], [c["vals"][0][3], c["vals"][0][4] + 1], c["openings"][0, 3:5], pairing="device") == [True, False]
    # a balance of 2^bits
    vals = list(c["vals"][0])
    vals[7] = 1 << 16
    with pytest.raises(ValueError, match=r"asset 0: 1 balance"):
        h.prove_balances(params, pk, d(vals).reshape(26, 4), seed=35)
    forced = h.prove_balances(params, pk, d(vals).reshape(26, 4), seed=35, check=False)
    assert forced.totals == [sum(vals)] and not h.verify_balances(params, vk, forced)
    two = torch.stack([c["bal"][0], d(vals).reshape(26, 4)])
    with pytest.raises(ValueError, match=r"asset 1: 1 balance"):
        h.prove_balances(params, pk, two, seed=36)
    # a key whose value column is blinded has another first commitment: refused
    blinded_cs = circuits.overflow_check_v2(4, 4)
    with pytest.raises(ValueError, match="unblinded_value"):
        solvency._range_parameters(blinded_cs, "prove_balances")
    # a negative balance: r - 10^9 lowers the total, and is what the range proof refuses
    vals[7] = R - 10 ** 9
    neg = h.prove_balances(params, pk, d(vals).reshape(26, 4), seed=37, check=False)
    assert neg.totals == [sum(vals) % R] and not h.verify_balances(params, vk, neg)
