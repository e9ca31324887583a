"""The ledger's id proof on the GPU (ledger.py with ``id_pk`` / ``id_vk``): a shuffled ledger is refused until
``ledger_order`` has sorted it, the sorted one verifies and every user's check passes with ``rows`` while an index behind the live rows
does not; a duplicated id is refused by ``check`` and, forced through, rejected under the id key -- and accepted without it, which is
the behaviour before this key existed, pinned here; an id proof over another column fails the commitment comparison; and without
``id_pk`` the proof is what the unchanged path computes.  k = 5 with overflow_check_v2(4, 4) and sorted_column(4, 4), every usable row
live.  Keys, parameters and proofs are made once and shared, never changed."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import circuits, ledger as lg, poseidon as ps, synthesis as sy
from halo2_experiments_amd.bn256 import FR_MODULUS as R, g1_ints
from halo2_experiments_amd.kzg import ParamsKZG

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
K, ROWS, N, ASSETS = 5, 26, 32, 2


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def case():
    params = ParamsKZG.setup(K, SRS_S, keep_points=True)
    cs, lay = circuits.overflow_check_v2(4, 4, unblinded_value=True), sy.RangeCheckLayout(K, 4, 4, rows=ROWS)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    id_cs, id_lay = circuits.sorted_column(4, 4), sy.SortedColumnLayout(K, 4, 4, rows=ROWS)
    id_vk = h.keygen_vk(params, id_cs, id_lay)
    id_pk = h.keygen_pk(params, id_vk, id_cs, id_lay, cosets=False)
    rng = random.Random("ledger distinct")
    ids = [rng.randrange(1 << 250)]
    for _ in range(ROWS - 1):
        ids.append(ids[-1] + rng.randrange(1, 1 << 16))          # distinct, neighbours less than 2^16 apart once sorted
    rng.shuffle(ids)
    vals = [[rng.randrange(1 << 16) for _ in range(ROWS)] for _ in range(ASSETS)]
    d_ids, d_bal = d(ids).reshape(ROWS, 4), d([v for vs in vals for v in vs]).reshape(ASSETS, ROWS, 4)
    perm = lg.ledger_order(d_ids)
    s_ids, s_bal = d_ids[perm].contiguous(), d_bal[:, perm].contiguous()
    proof = lg.prove_ledger(params, pk, s_ids, s_bal, seed=90, id_pk=id_pk)
    return dict(params=params, vk=vk, pk=pk, id_vk=id_vk, id_pk=id_pk, ids=ids, vals=vals, d_ids=d_ids, d_bal=d_bal, perm=perm.cpu().tolist(),
                s_ids=s_ids, s_bal=s_bal, proof=proof)


def test_shuffled_ids_are_refused_and_sorted_ones_verify(case):
    c = case
    params, vk, id_vk, proof = c["params"], c["vk"], c["id_vk"], c["proof"]
    assert c["perm"] == sorted(range(ROWS), key=lambda i: (c["ids"][i], i)) and c["perm"] != list(range(ROWS))
    with pytest.raises(ValueError, match=r"gap\(s\).*ledger_order"):
        lg.prove_ledger(params, c["pk"], c["d_ids"], c["d_bal"], seed=90, id_pk=c["id_pk"])
    assert isinstance(proof.id_proof, bytes) and proof.rows == ROWS
    assert lg.verify_ledger(params, vk, proof, id_vk=id_vk) and lg.verify_ledger(params, vk, proof, pairing="device", id_vk=id_vk)
    assert lg.verify_ledger(params, vk, proof)                   # the id proof is an addition: the rest verifies as before
    assert h.verify_proof(params, id_vk, [[]], proof.id_proof)
    # every user, and the rows behind them
    openings = lg.ledger_openings(params, proof)
    rows = list(range(N))
    ids_w = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    ids_w[:ROWS] = c["s_ids"]
    bal_w = torch.zeros((N, ASSETS, 4), dtype=torch.int64, device="cuda")
    bal_w[:ROWS] = c["s_bal"].transpose(0, 1)
    assert lg.verify_ledger_users(params, proof, rows, ids_w, bal_w, openings) == [True] * N
    assert lg.verify_ledger_users(params, proof, rows, ids_w, bal_w, openings, rows=ROWS) == [True] * ROWS + [False] * (N - ROWS)
    assert lg.verify_ledger_users(params, proof, [3, ROWS, 0], ids_w[[3, ROWS, 0]], bal_w[[3, ROWS, 0]], openings[[3, ROWS, 0]],
                                  rows=ROWS) == [True, False, True]
    sorted_ids = sorted(c["ids"])
    pis = openings.cpu().numpy().view(np.uint64)
    user = lambda i, **kw: lg.verify_ledger_user(params, proof, i, (sorted_ids + [0] * 6)[i],
                                                 [(vs + [0] * 6)[i] for vs in _sorted_vals(c)], pis[i], **kw)
    assert user(4, rows=ROWS) and user(ROWS - 1, rows=ROWS) and user(ROWS) and not user(ROWS, rows=ROWS) and not user(N - 1, rows=ROWS)


def _sorted_vals(c):
    return [[vs[i] for i in c["perm"]] for vs in c["vals"]]


def test_a_duplicated_id_is_rejected_under_the_id_key_only(case):
    c = case
    params, vk, pk, id_vk, id_pk = c["params"], c["vk"], c["pk"], c["id_vk"], c["id_pk"]
    ids = c["s_ids"].clone()
    ids[8] = ids[7]                                              # one row, id included, handed out twice
    host = sorted(c["ids"])
    host[8] = host[7]
    count = sy.SortedColumnLayout(K, 4, 4, ROWS).over(host)      # the pair itself, and the gap from the copy to row 9 when it is too wide
    assert count in (1, 2)
    with pytest.raises(ValueError, match=rf"{count} gap\(s\)"):
        lg.prove_ledger(params, pk, ids, c["s_bal"], seed=91, id_pk=id_pk)
    forced = lg.prove_ledger(params, pk, ids, c["s_bal"], seed=91, id_pk=id_pk, check=False)
    assert forced.id_proof is not None and forced.rows == ROWS
    assert not lg.verify_ledger(params, vk, forced, id_vk=id_vk)
    assert lg.verify_ledger(params, vk, forced)                  # without the id key nothing about ids is checked: as before
    # sorting does not help a duplicate
    perm = lg.ledger_order(ids)
    with pytest.raises(ValueError, match=r"gap\(s\)"):
        lg.prove_ledger(params, pk, ids[perm].contiguous(), c["s_bal"][:, perm].contiguous(), seed=91, id_pk=id_pk)


def test_an_id_proof_of_another_column_fails_the_commitment_comparison(case):
    c = case
    params, vk, id_vk, id_pk, proof = c["params"], c["vk"], c["id_vk"], c["id_pk"], c["proof"]
    other_ids = d(sorted(v + 1 for v in c["ids"])).reshape(ROWS, 4)
    other = lg.prove_ledger(params, c["pk"], other_ids, c["s_bal"], seed=92, id_pk=id_pk)
    assert lg.verify_ledger(params, vk, other, id_vk=id_vk) and other.id_commitment != proof.id_commitment
    fields = ("id_commitment", "commitments", "range_proofs", "id_total", "totals", "zero_opening", "columns", "id_proof", "rows")
    replace = lambda **kw: lg.LedgerProof(**{**{f: getattr(proof, f) for f in fields}, **kw})
    assert lg.verify_ledger(params, vk, replace(), id_vk=id_vk)
    assert h.verify_proof(params, id_vk, [[]], other.id_proof)   # a valid proof -- of another column
    assert not lg.verify_ledger(params, vk, replace(id_proof=other.id_proof), id_vk=id_vk)
    assert not lg.verify_ledger(params, vk, replace(id_proof=None), id_vk=id_vk)
    assert not lg.verify_ledger(params, vk, replace(id_proof=proof.id_proof[:-1]), id_vk=id_vk)
    assert not lg.verify_ledger(params, vk, replace(id_proof=proof.range_proofs[0]), id_vk=id_vk)
    # the keys are told apart
    with pytest.raises(ValueError, match="sorted_column"):
        lg.verify_ledger(params, vk, proof, id_vk=vk)
    with pytest.raises(ValueError, match="sorted_column"):
        lg.verify_ledger(params, id_vk, proof)
    with pytest.raises(ValueError, match="sorted_column"):
        lg.prove_ledger(params, c["pk"], c["s_ids"], c["s_bal"], seed=90, id_pk=c["pk"])
    with pytest.raises(ValueError, match="sorted_column"):
        lg.prove_ledger(params, id_pk, c["s_ids"], c["s_bal"], seed=90)


def test_without_the_id_key_the_proof_is_the_unchanged_one(case):
    c = case
    params, pk, proof = c["params"], c["pk"], c["proof"]
    plain = lg.prove_ledger(params, pk, c["s_ids"], c["s_bal"], seed=90)
    assert plain.id_proof is None and plain.rows is None
    for f in ("id_commitment", "commitments", "range_proofs", "id_total", "totals"):
        assert getattr(plain, f) == getattr(proof, f), f
    assert np.array_equal(plain.zero_opening, proof.zero_opening) and torch.equal(plain.columns, proof.columns)
    # ... and what the steps of the path give when made here: the witness, the proofs of seed + p, the commitments, the sums
    advice, _ = sy.range_witness(c["s_bal"], K, 4, 4)
    assert plain.range_proofs == h.create_proofs(params, pk, advice, [[[]]] * ASSETS, 90)
    columns = torch.zeros((ASSETS + 1, N, 4), dtype=torch.int64, device="cuda")
    columns[0, :ROWS] = c["s_ids"]
    columns[1:, :ROWS] = c["s_bal"]
    assert torch.equal(plain.columns, columns)
    assert [plain.id_commitment] + plain.commitments == [g1_ints(params.commit_lagrange(columns[j])) for j in range(ASSETS + 1)]
    assert plain.id_total == sum(c["ids"]) % R and plain.totals == [sum(vs) for vs in c["vals"]]
    assert lg.verify_ledger(params, c["vk"], plain) and not lg.verify_ledger(params, c["vk"], plain, id_vk=c["id_vk"])
