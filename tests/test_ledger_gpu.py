"""The ledger openings on the GPU (halo2_experiments_amd/ledger.py, csrc/ledger.hip): prove_ledger -> verify_ledger with its rejections,
ledger_openings against the single columns' openings and against open_at, and verify_ledger_users -- one kernel for every user's pairing
operands, one pairing call -- against the host function, the host twin of the kernel, the edges of a wavefront, tampered and malformed
users, and a ledger of constant columns, whose openings are all the identity.

Shapes: k = 5 with overflow_check_v2(4, 4) -- the reference's own range-check shape -- and k = 4.  A table of 2^4 entries does not fit
the 10 usable rows of k = 4 (RangeCheckLayout refuses it), so k = 4 runs overflow_check_v2(3, 4), the widest limb that fits; every check
is the same at both sizes.  Keys, parameters and proofs are made once per shape and shared, never changed."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import circuits, device_pairing, ledger as lg, poseidon as ps, synthesis as sy
from halo2_experiments_amd.bn256 import FQ_MODULUS as P_MOD, FR_MODULUS as R, fr_array, g1_ints, g1_words
from halo2_experiments_amd.domain import EvaluationDomain
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.openings import domain_omega, open_all, open_at
from halo2_experiments_amd.pairing import g1_add, g1_mul

import ledger_cases as lc

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
SHAPES = {4: (3, 4), 5: (4, 4)}                              # k -> (max_bits, acc_cols)


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def keys():
    out = {}
    for k, (max_bits, acc_cols) in SHAPES.items():
        params = ParamsKZG.setup(k, SRS_S, keep_points=True)
        cs = circuits.overflow_check_v2(max_bits, acc_cols, unblinded_value=True)
        lay = sy.RangeCheckLayout(k, max_bits, acc_cols, rows=(1 << k) - 6)
        vk = h.keygen_vk(params, cs, lay)
        out[k] = (params, vk, h.keygen_pk(params, vk, cs, lay, cosets=False))
    return out


@pytest.fixture(scope="module")
def cases(keys):
    """(k, P) -> the ledger: integers, words, the proof and every user's opening"""
    out = {}
    for k in SHAPES:
        for assets in (1, 3):
            params, vk, pk = keys[k]
            n, rows, bits = 1 << k, (1 << k) - 6, SHAPES[k][0] * SHAPES[k][1]
            rng = random.Random(f"ledger gpu {k} {assets}")
            ids = rng.sample(range(1, 1 << 62), rows - 1) + [R - 1]               # pairwise distinct
            vals = [[rng.randrange(1 << bits) for _ in range(rows - 2)] + [0, (1 << bits) - 1] for _ in range(assets)]
            bal = d([v for vs in vals for v in vs]).reshape(assets, rows, 4)
            proof = lg.prove_ledger(params, pk, d(ids).reshape(rows, 4), bal[0] if assets == 1 else bal, seed=50 + k)
            ids_p, vals_p = ids + [0] * 6, [vs + [0] * 6 for vs in vals]
            out[k, assets] = dict(k=k, n=n, P=assets, params=params, vk=vk, pk=pk, ids=ids_p, vals=vals_p, proof=proof,
                                  openings=lg.ledger_openings(params, proof), id_words=fr_array(ids_p),
                                  bal_words=np.ascontiguousarray(fr_array(vals_p).transpose(1, 0, 2)))
    return out


def users(c, rows, on_device=True):
    """the arguments of verify_ledger_users for these rows (with repetition)"""
    rows = list(rows)
    idw, bw = c["id_words"][rows], c["bal_words"][rows]
    return (rows, dev(idw), dev(bw), c["openings"][rows].contiguous()) if on_device else \
        (rows, idw, bw, c["openings"][rows].cpu().numpy().view(np.uint64))


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, assets", [(4, 1), (4, 3), (5, 1), (5, 3)])
def test_round_trip_and_rejections(cases, k, assets):
    c = cases[k, assets]
    params, vk, proof, n = c["params"], c["vk"], c["proof"], c["n"]
    assert proof.id_total == sum(c["ids"]) % R and proof.totals == [sum(vs) for vs in c["vals"]]
    assert len(proof.commitments) == len(proof.range_proofs) == assets and tuple(proof.columns.shape) == (assets + 1, n, 4)
    tail = c["openings"][n - 6:].cpu().numpy().view(np.uint64)
    assert lg.verify_ledger(params, vk, proof)
    assert lg.verify_ledger(params, vk, proof, pairing="device", tail=list(tail))
    fields = ("id_commitment", "commitments", "range_proofs", "id_total", "totals", "zero_opening")
    replace = lambda **kw: lg.LedgerProof(**{**{f: getattr(proof, f) for f in fields}, **kw})
    dv = dict(pairing="device")
    assert lg.verify_ledger(params, vk, replace(), **dv)
    assert not lg.verify_ledger(params, vk, replace(totals=[proof.totals[0] + 1] + proof.totals[1:]), **dv)            # a changed total
    assert not lg.verify_ledger(params, vk, replace(totals=proof.totals[:-1] + [proof.totals[-1] - 1]), **dv)
    assert not lg.verify_ledger(params, vk, replace(id_total=(proof.id_total + 1) % R), **dv)
    # sums that compensate each other under a challenge the prover knows: T_0 understated by d, S_id raised by challenge * d
    d_, gamma = 1000, lg.ledger_gamma(k, proof.id_commitment, proof.commitments)
    for ch in (gamma, lg.ledger_eta(k, proof.id_commitment, proof.commitments, proof.id_total, proof.totals)):
        forged = replace(totals=[proof.totals[0] - d_] + proof.totals[1:], id_total=(proof.id_total + ch * d_) % R)
        assert not lg.verify_ledger(params, vk, forged, **dv)
        if assets == 3:
            moved = [proof.totals[0] - d_, (proof.totals[1] + pow(ch, -1, R) * d_) % R, proof.totals[2]]
            assert not lg.verify_ledger(params, vk, replace(totals=moved), **dv)
    assert lg.verify_ledger_totals(params, proof, proof.id_total, proof.totals, proof.zero_opening, pairing="device")
    other = cases[k, 4 - assets]["proof"]                                                                               # the other ledger of this key
    if assets == 3:
        swapped = [proof.commitments[1], proof.commitments[0], proof.commitments[2]]
        assert not lg.verify_ledger(params, vk, replace(commitments=swapped), **dv)                                     # a swapped commitment
        assert not lg.verify_ledger(params, vk, replace(range_proofs=[proof.range_proofs[1], proof.range_proofs[0], proof.range_proofs[2]]), **dv)
        assert not lg.verify_ledger(params, vk, replace(commitments=swapped, range_proofs=[proof.range_proofs[j] for j in (1, 0, 2)]), **dv)
    else:
        assert not lg.verify_ledger(params, vk, replace(commitments=other.commitments[:1]), **dv)
        assert not lg.verify_ledger(params, vk, replace(range_proofs=other.range_proofs[:1]), **dv)                     # a range proof of another asset
    assert not lg.verify_ledger(params, vk, replace(id_commitment=other.id_commitment), **dv)
    assert not lg.verify_ledger(params, vk, replace(zero_opening=other.zero_opening), **dv)
    assert not lg.verify_ledger(params, vk, replace(), tail=list(tail[:5]), **dv)
    assert not lg.verify_ledger(params, vk, replace(), tail=[tail[j] for j in (1, 0, 2, 3, 4, 5)], **dv)                # tail rows in another order


def test_prove_ledger_checks_its_arguments(cases):
    c = cases[5, 1]
    params, pk = c["params"], c["pk"]
    ids, bal = d(c["ids"][:26]).reshape(26, 4), d(c["vals"][0][:26]).reshape(26, 4)
    with pytest.raises(ValueError, match="ids"):
        lg.prove_ledger(params, pk, ids[:25], bal, seed=1)
    with pytest.raises(ValueError, match="ids"):
        lg.prove_ledger(params, pk, ids.cpu(), bal, seed=1)
    big = ids.clone()
    big[3] = dev(lc.raw_words(R))
    with pytest.raises(ValueError, match="canonical"):
        lg.prove_ledger(params, pk, big, bal, seed=1)
    over = list(c["vals"][0][:26])
    over[7] = 1 << 16
    with pytest.raises(ValueError, match=r"asset 0: 1 balance"):
        lg.prove_ledger(params, pk, ids, d(over).reshape(26, 4), seed=1)
    with pytest.raises(ValueError, match="balances"):
        lg.prove_ledger(params, pk, ids, bal.cpu(), seed=1)


# ---- the openings -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, assets", [(4, 1), (5, 3)])
def test_openings_are_the_combination_of_the_columns_openings(cases, k, assets):
    c = cases[k, assets]
    params, proof, n = c["params"], c["proof"], c["n"]
    gamma = lg.ledger_gamma(k, proof.id_commitment, proof.commitments)
    single = open_all(params, proof.columns, form="lagrange").cpu().numpy().view(np.uint64)                              # (P + 1, n, 8)
    got = c["openings"].cpu().numpy().view(np.uint64)
    assert got.shape == (n, 8)
    for i in range(n):
        acc = None
        for j in range(assets + 1):
            acc = g1_add(acc, g1_mul(pow(gamma, j, R), g1_ints(single[j, i])))
        assert np.array_equal(got[i], g1_words(acc)), i
    # open_at of the combined polynomial, on three rows
    combined = h.linear_combination([proof.columns[j] for j in range(assets + 1)], fr_array([pow(gamma, j, R) for j in range(assets + 1)]))
    coeffs = EvaluationDomain(2, k).lagrange_to_coeff(combined.clone())
    for i in (0, 7, n - 1):
        value, pi = open_at(params, coeffs, pow(domain_omega(k), i, R))
        assert value == lg.combined_value(gamma, c["ids"][i], [vs[i] for vs in c["vals"]])
        assert np.array_equal(pi, got[i]), i
    # from the bare columns: the same openings
    assert torch.equal(lg.ledger_openings(params, proof.columns), c["openings"])


# ---- many users, a verdict each --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, assets", [(4, 1), (4, 3), (5, 1), (5, 3)])
def test_every_row_passes_and_equals_the_host_function(cases, k, assets):
    c = cases[k, assets]
    params, proof, n = c["params"], c["proof"], c["n"]
    rows = list(range(n))                                                                   # the six zero tail rows among them
    assert lg.verify_ledger_users(params, proof, *users(c, rows)) == [True] * n
    assert lg.verify_ledger_users(params, (proof.id_commitment, proof.commitments), *users(c, rows, on_device=False)) == [True] * n
    assert lg.verify_ledger_users(params, lg.ledger_statement(params, proof), *users(c, rows)) == [True] * n        # gamma and C_gamma made once
    pis = c["openings"].cpu().numpy().view(np.uint64)
    host = lambda i, **kw: lg.verify_ledger_user(params, proof, i, c["ids"][i], [vs[i] for vs in c["vals"]], pis[i], **kw)
    assert [host(i, pairing="device") for i in rows] == [True] * n
    assert all(host(i) for i in (0, n - 7, n - 1))                                          # ... and through pairing.py itself
    # the rows the kernel wrote against its host twin, user for user
    _, made = lg.ledger_pairs(params, proof, *users(c, rows))
    d_g1, d_flags, d_g2 = made
    assert not bool(d_flags.any()) and tuple(d_g1.shape) == (2 * n, 8) and tuple(d_g2.shape) == (2 * n, 16)
    got = d_g1.cpu().numpy().view(np.uint64).reshape(n, 2, 8)
    hc = lc.load_twin()
    gamma = lg.ledger_gamma(k, proof.id_commitment, proof.commitments)
    c_gamma = lg.combined_commitment(gamma, proof.id_commitment, proof.commitments)
    for i in rows:
        flag, rows_i = lc.twin_rows(hc, k, gamma, c_gamma, i, c["id_words"][i], c["bal_words"][i], pis[i])
        assert flag == 0 and np.array_equal(got[i], rows_i), i
        assert np.array_equal(got[i], lc.expected_rows(k, gamma, c_gamma, i, c["ids"][i], [vs[i] for vs in c["vals"]], g1_ints(pis[i]))), i


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_batch_sizes_around_a_wavefront(cases, B):
    c = cases[5, 3]
    rows = [(7 * j + 3) % c["n"] for j in range(B)]                                         # gathered with repetition
    args = users(c, rows)
    assert lg.verify_ledger_users(c["params"], c["proof"], *args) == [True] * B
    ids = args[1].clone()
    ids[B - 1, 0] ^= 1                                                                      # the last lane of the last wavefront
    assert lg.verify_ledger_users(c["params"], c["proof"], rows, ids, args[2], args[3]) == [True] * (B - 1) + [False]


@pytest.mark.parametrize("k, assets", [(4, 1), (5, 3)])
def test_tampering_fails_exactly_the_tampered_users(cases, k, assets):
    c = cases[k, assets]
    n = c["n"]
    rows, ids, bal, pis = users(c, range(n))
    ids, bal, pis = ids.clone(), bal.clone(), pis.clone()
    ids[1] = dev(fr_array([c["ids"][1] + 1]))[0]                                            # one id
    bal[3, assets - 1] = dev(fr_array([c["vals"][assets - 1][3] + 1]))[0]                   # one balance of the last asset
    pis[[5, 6]] = pis[[6, 5]]                                                               # one opening swapped with its neighbour
    rows[8] = 9                                                                             # one index off by one
    bad = {1, 3, 5, 6, 8}
    assert lg.verify_ledger_users(c["params"], c["proof"], rows, ids, bal, pis) == [i not in bad for i in range(n)]


def test_malformed_users_are_flagged_and_nothing_else_changes(cases):
    c = cases[5, 3]
    params, proof, n = c["params"], c["proof"], c["n"]
    rows, ids, bal, pis = users(c, range(n), on_device=False)
    ids, bal, pis = ids.copy(), bal.copy(), pis.copy()
    pis[2, 4] ^= np.uint64(1)                                                               # off the curve
    pis[4, :4] = lc.raw_words(P_MOD)                                                        # x = p
    pis[6, 4:] = lc.raw_words((1 << 256) - 1)                                               # y >= p
    ids[9] = lc.raw_words(R)                                                                # a scalar pattern >= r
    bal[11, 2] = lc.raw_words(R + 5)
    pis[13] = 0                                                                             # the identity where the opening is not: valid, and wrong
    flagged = {2, 4, 6, 9, 11}
    assert lg.verify_ledger_users(params, proof, rows, ids, bal, pis) == [i not in flagged | {13} for i in range(n)]
    _, (d_g1, d_flags, d_g2) = lg.ledger_pairs(params, proof, rows, ids, bal, pis)
    assert d_flags.cpu().tolist() == [int(i in flagged) for i in range(n)]
    got = d_g1.cpu().numpy().view(np.uint64).reshape(n, 2, 8)
    assert all(not got[i].any() for i in flagged) and all(got[i, 1].any() for i in range(n) if i not in flagged)
    status = device_pairing.run_device(d_g1, d_g2, torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device="cuda"), n).cpu().tolist()
    # a flagged user's identity rows pass the pairing -- status 1 --: the flag is what fails it; row 13 fails in the pairing
    assert status == [0 if i == 13 else 1 for i in range(n)]


@pytest.mark.parametrize("k, assets", [(4, 1), (5, 3)])
def test_constant_columns_open_to_the_identity(cases, k, assets):
    """every column constant over the WHOLE domain: each opening is the identity, and R = C_gamma - [y]G has to come out as one"""
    c = cases[k, assets]
    params, n = c["params"], c["n"]
    consts = [R - 3] + [11 * (p + 1) for p in range(assets)]
    columns = dev(fr_array([[v] * n for v in consts]))
    public = (g1_ints(params.commit_lagrange(columns[0])), [g1_ints(params.commit_lagrange(columns[1 + p])) for p in range(assets)])
    openings = lg.ledger_openings(params, columns)
    assert tuple(openings.shape) == (n, 8) and not bool(openings.any())
    rows = list(range(n))
    ids, bal = dev(fr_array([consts[0]] * n)), dev(fr_array([consts[1:]] * n))
    assert lg.verify_ledger_users(params, public, rows, ids, bal, openings) == [True] * n
    _, (d_g1, d_flags, _) = lg.ledger_pairs(params, public, rows, ids, bal, openings)
    assert not bool(d_g1.any()) and not bool(d_flags.any())
    wrong = ids.clone()
    wrong[2] = dev(fr_array([5]))[0]
    assert lg.verify_ledger_users(params, public, rows, wrong, bal, openings) == [i != 2 for i in range(n)]


def test_errors_come_before_any_launch(cases):
    c = cases[5, 3]
    params, proof, n = c["params"], c["proof"], c["n"]
    rows, ids, bal, pis = users(c, range(4))
    assert lg.verify_ledger_users(params, proof, [], ids[:0], bal[:0], pis[:0]) == []
    for bad_rows in ([0, 1, 2, n], [0, 1, 2, -1], [0, 1, 2, 1 << 20]):
        with pytest.raises(ValueError, match="outside the domain"):
            lg.verify_ledger_users(params, proof, bad_rows, ids, bal, pis)
    assert lg.verify_ledger_users(params, proof, [0, 1, 2, 3], ids, bal, pis, k=5) == [True] * 4
    with pytest.raises(ValueError, match="outside the domain"):
        lg.verify_ledger_users(params, proof, [0, 1, 2, 16], ids, bal, pis, k=4)
    for args in ((rows, ids[:3], bal, pis), (rows, ids, bal[:, :2].contiguous(), pis), (rows, ids, bal, pis[:, :4].contiguous()),
                 (rows, ids, bal.reshape(4, 12), pis), (rows[:3], ids, bal, pis), (rows, ids.to(torch.int32), bal, pis),
                 (rows, ids.cpu(), bal, pis), (rows, ids, bal, pis.cpu().numpy()), (rows, ids, bal.cpu().numpy().view(np.uint64).astype(np.float64), pis),
                 ([0.5, 1, 2, 3], ids, bal, pis)):
        with pytest.raises(ValueError):
            lg.verify_ledger_users(params, proof, *args)
    with pytest.raises(ValueError):
        lg.verify_ledger_users(params, (proof.id_commitment, []), rows, ids, bal[:, :0].contiguous(), pis)
    with pytest.raises(ValueError):
        lg.ledger_openings(params, proof.columns[0])
    with pytest.raises(ValueError):
        lg.ledger_openings(params, lg.LedgerProof(None, [None], [], 0, [0], None))
    # a commitment off the curve: every answer False, nothing launched
    assert lg.verify_ledger_users(params, ((1, 1), proof.commitments), rows, ids, bal, pis) == [False] * 4
