"""The sorted-column circuit on the GPU: synthesis.sorted_witness word for word against SortedColumnLayout.assign_ints (one id, two, every
usable row, limbs of 16 bits at k = 17, the counters of m circuits side by side, the zeros behind the live rows), ledger.ledger_order
against Python's sort by (id, row) at the sizes around its tile, the device MockProver on a batch mixing good and bad columns against
the CPU verdicts of tests/sorted_column_cases.py, and keygen / create_proof / verify_proof with both multiopens, the first commitment
being commit_lagrange of the id column.  Keys, parameters and proofs are made once per shape and shared, never changed."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import circuits, ledger as lg, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.transcript import g1_decompress_int

import sorted_column_cases as sc

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
SL = sy.SortedColumnLayout
TILE = lg.ARGSORT_TILE


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def words(columns):
    return sy.columns_to_words(columns)


# ---- the witness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, max_bits, acc_cols, rows", [(5, 4, 4, 1), (5, 4, 4, 2), (5, 4, 4, 26), (17, 16, 8, 1000), (3, 1, 1, 2)])
def test_witness_equals_assign_ints(k, max_bits, acc_cols, rows):
    """m = 3 circuits: a satisfied column between two columns with bad gaps -- the counters must not leak from one to the next; the
    output starts as all ones, so every word must be written, zeros behind the live rows and in the limbs of the last live row"""
    m, lay, B = 3, SL(k, max_bits, acc_cols, rows), max_bits * acc_cols
    ids = [sc.host_ids(max_bits, acc_cols, rows, seed=1), sc.ascending(rows, B, seed=2), sc.host_ids(max_bits, acc_cols, rows, seed=3)]
    dv = d([v for vs in ids for v in vs]).reshape(m, rows, 4)
    out = torch.full((m, 1 + acc_cols, 1 << k, 4), -1, dtype=torch.int64, device="cuda")
    adv, over = sy.sorted_witness(dv, k, max_bits, acc_cols, out=out)
    assert adv.data_ptr() == out.data_ptr()
    got = adv.cpu().numpy().view(np.uint64)
    for c in range(m):                                           # the live rows word for word; behind them every word must be zero
        assert np.array_equal(got[c][:, :rows], words([col[:rows] for col in lay.assign_ints(ids[c])])), c
    assert not got[:, :, rows:].any() and not got[:, 1:, rows - 1].any()
    expected = [lay.over(vs) for vs in ids]
    assert over.cpu().tolist() == expected and expected[1] == 0 and (rows < 4 or min(expected[0], expected[2]) >= 2)
    host_adv, host_over = sy.sorted_witness_host(dv.cpu().numpy().view(np.uint64), k, max_bits, acc_cols)
    assert np.array_equal(host_adv, got) and host_over.tolist() == expected
    one, over1 = sy.sorted_witness(dv[2], k, max_bits, acc_cols)                                # (rows, 4): one circuit
    assert np.array_equal(one.cpu().numpy().view(np.uint64)[0], got[2]) and over1.cpu().tolist() == expected[2:]


def test_witness_refuses_what_the_layout_refuses():
    dv = d([1, 2, 3]).reshape(1, 3, 4)
    out = torch.full((1, 16, 1 << 17, 4), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(h._lib.Halo2Mi355xError, match="253"):
        sy.sorted_witness(dv, 17, 16, 15, out=out)                # B + k = 257
    with pytest.raises(h._lib.Halo2Mi355xError):
        sy.sorted_witness(d(list(range(27))).reshape(1, 27, 4), 5, 4, 4)
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    with pytest.raises(ValueError):
        sy.sorted_witness(dv.cpu(), 5)
    with pytest.raises(ValueError):
        sy.sorted_witness(dv, 5, out=torch.zeros((1, 5, 16, 4), dtype=torch.int64, device="cuda"))


# ---- the order ------------------------------------------------------------------------------------------------------------------------
def _order(ids):
    return sorted(range(len(ids)), key=lambda i: (ids[i], i))


@pytest.fixture(scope="module")
def random_ids():
    """2 * tile + 5 random 254-bit ids with 0 and r - 1 among them, and repeats: shared by the sizes, never changed"""
    rnd = random.Random(0xA45)
    ids = [rnd.randrange(R) for _ in range(2 * TILE + 5)]
    ids[5], ids[17], ids[40], ids[41] = R - 1, 0, ids[3], ids[3]
    return ids


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 5])
def test_order_of_random_ids(random_ids, n):
    ids = random_ids[:n]
    perm = lg.ledger_order(d(ids).reshape(n, 4))
    assert perm.dtype == torch.int64 and perm.is_cuda and tuple(perm.shape) == (n,)
    assert perm.cpu().tolist() == _order(ids)


@pytest.mark.parametrize("name", ["top word", "low word", "sorted", "reversed", "equal", "few values"])
def test_order_of_patterns(name):
    n, rnd = TILE + 70, random.Random(name)
    base = rnd.randrange(1 << 180)
    ids = {"top word": lambda: [(rnd.randrange(1 << 61) << 192) + base for _ in range(n)],       # differing only in the top 64-bit word
           "low word": lambda: [(base << 64) + rnd.randrange(1 << 64) for _ in range(n)],       # ... only in the low word
           "sorted": lambda: sorted(rnd.randrange(R) for _ in range(n)),
           "reversed": lambda: sorted((rnd.randrange(R) for _ in range(n)), reverse=True),
           "equal": lambda: [base] * n,
           "few values": lambda: [rnd.choice((0, 1, R - 1, base)) for _ in range(n)]}[name]()
    perm = lg.ledger_order(d(ids).reshape(n, 4)).cpu().tolist()
    assert perm == _order(ids)
    if name == "equal":
        assert perm == list(range(n))                            # ties by row: the identity


def test_order_refuses_bad_arguments():
    ids = d([3, 1, 2]).reshape(3, 4)
    for bad in (ids.cpu(), ids[:0], ids.reshape(12), ids.to(torch.int32)):
        with pytest.raises(ValueError):
            lg.ledger_order(bad)
    assert lg.ledger_order(ids.repeat(1, 2)[:, :4]).cpu().tolist() == [1, 2, 0]                 # a strided view is made contiguous


# ---- the device MockProver ----------------------------------------------------------------------------------------------------------
def test_device_mock_prover_agrees_with_the_cpu_verdicts():
    k, rows = 5, 26
    lay, cs = SL(k, 4, 4, rows), circuits.sorted_column(4, 4)
    cases = sc.columns_at_4_4(rows)
    m = len(cases)
    adv, over = sy.sorted_witness(d([v for _, ids, _, _ in cases for v in ids]).reshape(m, rows, 4), k, 4, 4)
    assert over.cpu().tolist() == [o for *_, o in cases]
    mp = h.MockProver(cs, lay)
    res = mp.verify(adv)
    assert res.users_failed == [u for u, (_, _, satisfied, _) in enumerate(cases) if not satisfied] == [1, 2, 3]
    expected = []
    for u, (name, ids, satisfied, _) in enumerate(cases):
        fails = sc.verify(lay, cs, lay.assign_ints(ids))
        assert (fails == []) == satisfied, name
        expected += [("gate", u, gate, poly, row) for _, gate, poly, row in fails]
    assert sorted(res.failures) == sorted(expected) and res.total == {"gate": len(expected), "copy": 0, "lookup": 0}
    good = adv[[0, 4, 5]].contiguous()
    mp.assert_satisfied(good)
    with pytest.raises(h.NotSatisfied):
        mp.assert_satisfied(adv)
    bad = good.clone()
    bad[1, 3, 7] = d([16])[0]                                    # a limb outside the table, no id adjusted: the gate and the lookup
    res = mp.verify(bad)
    assert sorted(res.failures) == [("gate", 1, sc.GATE, 0, 7), ("lookup", 1, 2, 7)] and res.users_failed == [1]


# ---- proving ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proved():
    """(k, max_bits, acc_cols, rows) -> params, keys, ids, witness: (4, 4) at k = 5 with every usable row, (8, 2) at k = 9"""
    out = {}
    for k, max_bits, acc_cols, rows in ((5, 4, 4, 26), (9, 8, 2, 300)):
        params = ParamsKZG.setup(k, SRS_S, keep_points=True)
        cs, lay = circuits.sorted_column(max_bits, acc_cols), SL(k, max_bits, acc_cols, rows)
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        ids = sc.ascending(rows, max_bits * acc_cols, seed=k)
        adv, over = sy.sorted_witness(d(ids).reshape(1, rows, 4), k, max_bits, acc_cols)
        assert over.cpu().tolist() == [0]
        out[k] = dict(params=params, cs=cs, lay=lay, vk=vk, pk=pk, ids=ids, adv=adv, rows=rows, shape=(max_bits, acc_cols))
    return out


@pytest.mark.parametrize("k, multiopen", [(5, "shplonk"), (5, "gwc"), (9, "shplonk")])
def test_proofs_verify_and_open_the_id_commitment(proved, k, multiopen):
    c = proved[k]
    p, vk, pk = c["params"], c["vk"], c["pk"]
    proof = h.create_proof(p, pk, c["adv"][0], [[]], 70 + k, multiopen=multiopen)
    assert h.verify_proof(p, vk, [[]], proof, multiopen=multiopen)
    other = "gwc" if multiopen == "shplonk" else "shplonk"
    assert not h.verify_proof(p, vk, [[]], proof, multiopen=other)
    column = c["adv"][0, 0].contiguous()
    assert not bool(column[c["rows"]:].any())
    assert g1_decompress_int(proof[:32]) == h.bn256.g1_ints(p.commit_lagrange(column))
    assert h.create_proofs(p, pk, c["adv"], [[[]]], [70 + k], multiopen=multiopen) == [proof]
    flipped = bytearray(proof)
    flipped[-1] ^= 1
    assert not h.verify_proof(p, vk, [[]], bytes(flipped), multiopen=multiopen)


@pytest.mark.parametrize("k", [5, 9])
def test_unsorted_ids_are_rejected(proved, k):
    c = proved[k]
    p, vk, pk, rows = c["params"], c["vk"], c["pk"], c["rows"]
    for name, change in (("duplicate", lambda v: v[:7] + [v[6]] + v[8:]), ("swapped", lambda v: v[:3] + [v[4], v[3]] + v[5:])):
        ids = change(list(c["ids"]))
        adv, over = sy.sorted_witness(d(ids).reshape(1, rows, 4), k, *c["shape"])
        assert over.cpu().tolist() == [c["lay"].over(ids)] and over.cpu().tolist()[0] >= 1, name
        assert not h.verify_proof(p, vk, [[]], h.create_proof(p, pk, adv[0], [[]], 9), trapdoor=SRS_S), name
