"""``MockProver`` on the GPU against the tests' own Python-integer checker (tests/mock_prover.py, the yardstick): the failure SETS of
every user must be the yardstick's -- on a synthetic constraint system that has every feature (rotations -1 / +1 that wrap inside a
user, a gate of two polynomials, a fixed-table and an advice-table lookup, copies between advice, fixed and instance cells, an
instance column shorter than the domain) and on the three circuits' own witnesses."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.circuits import ConstraintSystem
from halo2_experiments_amd.evaluation import Advice, Fixed, Instance
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.mock_prover import KINDS, MockProver, NotSatisfied, decode_records

import mock_prover as yardstick
import prover_cases as pc

pytestmark = pytest.mark.gpu
R = yardstick.R
FILL = 0x5A5A5A5A5A5A5A5A
INST_ROWS = 3
TOP_WORD = 5 + (7 << 224)          # the table holds 5: equal in the seven low words
FOURTH_WORD = 5 + (1 << 96)        # ... equal in the three low words


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merkle_sum_tree_case.json")) as f:
        g = json.load(f)
    return (g["leaf"]["hash"], g["leaf"]["balance"]), [(e["hash"], e["balance"]) for e in g["path_elements"]], list(g["path_indices"])


def _path_tensors(leaf, sib, bits):
    leaves = d(list(leaf)).reshape(1, 2, 4)
    sibs = d([v for p in sib for v in p]).reshape(1, len(sib), 2, 4)
    return leaves, sibs, torch.tensor([sum(int(b) << l for l, b in enumerate(bits))], dtype=torch.int64, device="cuda")


# ---- the synthetic constraint system ----------------------------------------------------------------------------------
def synthetic_cs():
    q, a0, a1, a2 = Fixed(0), Advice(0), Advice(1), Advice(2)
    neighbours = Advice(0, -1) + Advice(0, 1)
    gates = [("neighbours", [q * (neighbours - a1)]),
             ("pair", [q * a2 * (a1 - neighbours), q * Instance(0) * (Instance(0) - a0)])]
    lookups = [([a2], [Fixed(1)]), ([a2], [Advice(2, 1)])]
    equality = [("advice", 0), ("advice", 2), ("fixed", 1), ("instance", 0)]
    return ConstraintSystem("synthetic", "tests", 2, 3, 1, gates, lookups, equality, blinding_factors=5)


COPIES = [(("advice", 0, 1), ("advice", 0, 3)), (("advice", 2, 0), ("fixed", 1, 0)), (("advice", 0, 2), ("instance", 0, 2))]


def synthetic_fixed(k):
    n, usable = 1 << k, (1 << k) - 6
    table = list(range(usable - 2)) + [3 * (1 << 224) + 5, R - 1]
    return [[1] * usable + [0] * 6, table + [0] * 6], table


def synthetic_witness(k, m, seed=1):
    """-> (advice integers [user][column][row], instance integers [user][row]); satisfied, every user's cells distinct"""
    rng = random.Random(seed * 1000 + k * 100 + m)
    n, usable = 1 << k, (1 << k) - 6
    _, table = synthetic_fixed(k)
    adv, inst = [], []
    for u in range(m):
        a0 = [rng.randrange(1, R) for _ in range(n)]
        a0[3] = a0[1]
        a1 = [(a0[(r - 1) % n] + a0[(r + 1) % n]) % R for r in range(n)]
        a2 = [table[0]] + [table[(3 * r + u) % usable] for r in range(1, n)]
        adv.append([a0, a1, a2])
        inst.append(a0[:INST_ROWS])
    return adv, inst


def to_device(adv, inst):
    m, n = len(adv), len(adv[0][0])
    a = d([v for user in adv for col in user for v in col]).reshape(m, 3, n, 4)
    i = d([v for user in inst for v in user]).reshape(m, INST_ROWS, 4)
    return a, i


def expected(cs, fixed, adv_t, inst_t, copies, users, k, rows=None):
    """the yardstick on the users named: sorted failures with the user in second place, as MockProver lists them"""
    n = 1 << k
    out = []
    for u in users:
        inst_cols = []
        for t in inst_t:
            col = ints(t[u])
            inst_cols.append(col + [0] * (n - len(col)))
        fails = yardstick.verify(cs, fixed, [ints(c) for c in adv_t[u]], inst_cols, copies, n, n - 6, rows=rows)
        out += [(f[0], u) + tuple(f[1:]) for f in fails]
    return sorted(out)


def corrupt(t, *index):
    t[index + (0,)] ^= 1


@pytest.fixture(scope="module")
def synthetic():
    cs = synthetic_cs()
    return {k: dict(cs=cs, k=k, fixed=synthetic_fixed(k)[0], mp=MockProver(cs, k=k, fixed=synthetic_fixed(k)[0], copies=COPIES)) for k in (4, 6)}


@pytest.mark.parametrize("m", [1, 3, 65])
@pytest.mark.parametrize("k", [4, 6])
def test_synthetic_satisfied_and_corrupted(synthetic, k, m):
    s = synthetic[k]
    cs, mp, fixed, n, usable = s["cs"], s["mp"], s["fixed"], 1 << k, (1 << k) - 6
    adv, inst = to_device(*synthetic_witness(k, m))
    assert expected(cs, fixed, adv, [inst], COPIES, [0, m - 1], k) == []            # the witness is what it is meant to be
    res = mp.verify(adv, inst)
    assert res.ok and res.total == {"gate": 0, "copy": 0, "lookup": 0} and res.failures == [] and res.users_failed == []
    mp.assert_satisfied(adv, [inst])
    last, mid = m - 1, m // 2

    def check(a, i, touched, must_fail=True):
        got = mp.verify(a, i)
        want = expected(cs, fixed, a, [i], COPIES, sorted(set(touched)), k)
        assert got.failures == want                                                  # nothing for any user that was not touched
        assert got.total == {kind: sum(f[0] == kind for f in want) for kind in KINDS}
        assert got.users_failed == sorted({f[1] for f in want}) and got.ok == (not want)
        assert bool(want) == must_fail
        return want

    # the first and the last usable row of the first and the last user; the rotations wrap inside the user
    a = adv.clone()
    corrupt(a, 0, 1, 0)
    corrupt(a, last, 1, usable - 1)
    want = check(a, inst, [0, last])
    assert ("gate", 0, "neighbours", 0, 0) in want and ("gate", last, "neighbours", 0, usable - 1) in want
    a = adv.clone()
    corrupt(a, 0, 0, n - 1)                  # read by row 0 of the SAME user at rotation -1 (and by no other usable row)
    assert [f for f in check(a, inst, [0]) if f[0] == "gate"] == [("gate", 0, "neighbours", 0, 0)]      # (a2 is 0 on row 0: "pair" holds)
    a = adv.clone()
    corrupt(a, last, 0, n - 6)               # the first blinding row, read by the last usable row of the same user at rotation +1
    assert ("gate", last, "neighbours", 0, usable - 1) in check(a, inst, [last])
    # a cell of the first blinding row that no usable row reaches is not checked
    a = adv.clone()
    corrupt(a, mid, 1, n - 6)
    check(a, inst, [mid], must_fail=False)
    # a copy cell, an instance cell, the advice cell copied from the fixed column
    a, i = adv.clone(), inst.clone()
    corrupt(a, 0, 0, 3)
    corrupt(i, last, 2)
    a[mid, 2, 0] = d([1])[0]
    want = check(a, i, [0, mid, last])
    assert ("copy", 0) + COPIES[0] in want and ("copy", mid) + COPIES[1] in want and ("copy", last) + COPIES[2] in want
    assert m > 1 or len([f for f in want if f[0] == "copy"]) == 3
    # lookup inputs: a value absent from the table, values that differ from a table entry in one high word only
    a = adv.clone()
    a[0, 2, 4] = d([1000])[0]
    a[mid, 2, 0] = d([TOP_WORD])[0]
    a[last, 2, 2] = d([FOURTH_WORD])[0]
    want = check(a, inst, [0, mid, last])
    assert ("lookup", 0, 0, 4) in want and ("lookup", mid, 0, 0) in want and ("lookup", mid, 1, 0) in want and ("lookup", last, 0, 2) in want


def test_an_advice_table_is_each_users_own(synthetic):
    """lookup 1's table is a rotated advice column: a value that only user 0's table holds does not serve user 1"""
    s = synthetic[4]
    adv, inst = to_device(*synthetic_witness(4, 2))
    adv[0, 2, 5] = d([2000])[0]
    adv[1, 2, 0] = d([2000])[0]
    res = s["mp"].verify(adv, inst)
    want = expected(s["cs"], s["fixed"], adv, [inst], COPIES, [0, 1], 4)
    assert res.failures == want and ("lookup", 1, 1, 0) in want and ("lookup", 0, 1, 5) not in want and ("lookup", 0, 0, 5) in want


def test_cap_totals_flags_and_determinism(synthetic):
    s = synthetic[4]
    k, m, cs, mp = 4, 65, s["cs"], s["mp"]
    adv, inst = to_device(*synthetic_witness(k, m))
    adv[:, 1, :, 0] ^= 1                     # every row of a1 of every user: 650 rows fail "neighbours"
    adv[:, 0, 3, 0] ^= 2                     # ... one copy per user
    adv[:, 2, 4] = d([1000])[0]              # ... and both lookups on row 4
    want = expected(cs, s["fixed"], adv, [inst], COPIES, range(m), k)
    totals = {kind: sum(f[0] == kind for f in want) for kind in KINDS}
    assert totals["gate"] > 100 and totals["copy"] == m and totals["lookup"] >= m
    res = mp.verify(adv, inst, max_failures=4)
    assert res.total == totals and not res.ok and res.users_failed == list(range(m))
    assert [sum(f[0] == kind for f in res.failures) for kind in KINDS] == [4, 4, 4]
    assert res.failures == sorted(sum(([f for f in want if f[0] == kind][:4] for kind in KINDS), []))      # the smallest of each kind
    assert mp.verify(adv, inst, max_failures=4) == res
    full = mp.verify(adv, inst, max_failures=10 ** 6)
    assert full.failures == want and mp.verify(adv, inst, max_failures=10 ** 6) == full
    with pytest.raises(NotSatisfied, match=r"\('neighbours'\) is not satisfied outside any region, on row 0") as e:
        mp.assert_satisfied(adv, inst)
    assert e.value.result.total == totals
    # a chunk of the batch, and a batch written into a larger buffer
    part = mp.verify(adv[10:13], inst[10:13], max_failures=10 ** 6)
    assert part.failures == sorted((f[0], f[1] - 10) + f[2:] for f in want if 10 <= f[1] < 13) and part.users_failed == [0, 1, 2]
    one = mp.verify(adv[64], inst[64], max_failures=10 ** 6)
    assert one.failures == sorted((f[0], 0) + f[2:] for f in want if f[1] == 64)


def _entry_args(mp, adv, inst):
    adv, insts, m = mp._batch(adv, inst)
    return mp._state(), mp._table(adv, insts), m


def test_the_record_buffer_ends_at_its_capacity(synthetic):
    """the gates' entry with room for 4 records and 650 failing lanes: the counter is exact, the words behind the buffer keep their
    pattern, every user is flagged"""
    s = synthetic[4]
    mp, m = s["mp"], 65
    adv, inst = to_device(*synthetic_witness(4, m))
    adv[:, 1, :, 0] ^= 1
    dev, (bases, strides, rows, count), _ = _entry_args(mp, adv, inst)
    rec = torch.full((4 + 60,), FILL, dtype=torch.int64, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    flags = torch.zeros(m + 8, dtype=torch.uint8, device="cuda")
    dyn = np.ascontiguousarray(ps.ints_to_words([0, 0, 0, 12345]).reshape(4, 4))
    out = ctypes.c_uint64(0)
    vp = ctypes.c_void_p
    u64 = lambda addr: ctypes.cast(vp(addr), ctypes.POINTER(ctypes.c_uint64))       # lanes, records and counter are uint64_t*
    lib = _lib.load()
    for cap, lanes in ((4, None), (4, torch.tensor([(64 << 32) | 9, (3 << 32) | 0, (65 << 32) | 0, (1 << 32) | 10], dtype=torch.int64, device="cuda"))):
        rec.fill_(FILL)
        counter.zero_()
        flags.zero_()
        _lib.check(lib.hm_mock_gates_dev(ctypes.c_uint64(dev.combined.handle), bases, strides, rows, count, dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                         4, 4, 10, m, u64(lanes.data_ptr()) if lanes is not None else None, 0 if lanes is None else lanes.numel(),
                                         u64(rec.data_ptr()), cap, u64(counter.data_ptr()), vp(flags.data_ptr()), ctypes.byref(out), None))
        assert bool((rec[4:] == FILL).all()) and not bool(flags[m:].any())
        if lanes is None:
            assert out.value == counter.item() == m * 10 and bool(flags[:m].all())
            got = decode_records(rec[:4].cpu().numpy())
            assert len(set(got)) == 4 and all(u < m and r < 10 for u, r in got)
        else:                                  # a list: only the lanes inside the batch run -- user 65 and row 10 are none
            assert out.value == 2 and decode_records(rec[:2].cpu().numpy()) == [(3, 0), (64, 9)] and flags.nonzero().flatten().tolist() == [3, 64]


def test_rejected_arguments_leave_everything_untouched(synthetic):
    s = synthetic[4]
    mp, m = s["mp"], 3
    adv, inst = to_device(*synthetic_witness(4, m))
    adv[:, 1, :, 0] ^= 1                                                   # failures that WOULD be written
    dev, (bases, strides, rows, count), _ = _entry_args(mp, adv, inst)
    rec = torch.full((16,), FILL, dtype=torch.int64, device="cuda")
    counter = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    flags = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
    dyn = np.ascontiguousarray(ps.ints_to_words([0, 0, 0, 12345]).reshape(4, 4))
    dynp, vp, lib = dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.c_void_p, _lib.load()
    u64 = lambda addr: ctypes.cast(vp(addr), ctypes.POINTER(ctypes.c_uint64))       # records and counter are uint64_t*
    pairs = dev.pairs
    perm = mp._perm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    table = dev.lookups[0].shared

    def call(which, bases=bases, rows=rows, m=m, cap=8, rec_ptr=rec.data_ptr()):
        out = ctypes.c_uint64(99)
        tail = (u64(rec_ptr), cap, u64(counter.data_ptr()), vp(flags.data_ptr()), ctypes.byref(out), None)
        if which == "gates":
            rc = lib.hm_mock_gates_dev(ctypes.c_uint64(dev.combined.handle), bases, strides, rows, count, dynp, 4, 4, 10, m, None, 0, *tail)
        elif which == "copies":
            rc = lib.hm_mock_copies_dev(bases, strides, rows, count, perm, len(mp._perm), ctypes.cast(vp(pairs.data_ptr()), ctypes.POINTER(ctypes.c_uint32)),
                                        len(mp._pairs), 4, m, *tail)
        else:
            rc = lib.hm_mock_lookup_dev(ctypes.c_uint64(dev.lookups[0].input.handle), bases, strides, rows, count, dynp, 4, 4, 10, m, 0,
                                        vp(table.data_ptr()), *tail)
        return rc, out.value

    misaligned = (ctypes.c_void_p * count)(*[b + (8 if j == 2 else 0) for j, b in enumerate(bases)])
    long_instance = (ctypes.c_uint32 * count)(*[17 if j == count - 1 else r for j, r in enumerate(rows)])
    for which in ("gates", "copies", "lookup"):
        for kw in (dict(bases=misaligned), dict(m=0), dict(cap=0), dict(rows=long_instance), dict(rec_ptr=rec.data_ptr() + 4)):
            assert call(which, **kw) == (-1, 99), (which, kw)
            assert which.encode() in lib.hm_last_error()
    assert lib.hm_mock_gates_dev(ctypes.c_uint64(1 << 40), bases, strides, rows, count, dynp, 4, 4, 10, m, None, 0, u64(rec.data_ptr()), 8,
                                 u64(counter.data_ptr()), vp(flags.data_ptr()), ctypes.byref(ctypes.c_uint64(0)), None) == -4      # unknown handle
    torch.cuda.synchronize()
    assert bool((rec == FILL).all()) and counter.item() == 41 and bool((flags == 7).all())
    assert call("gates")[0] == 0 and counter.item() == 41 + 30               # and the same arguments, not refused, do write


def test_python_refuses_what_is_not_a_batch(synthetic):
    mp = synthetic[4]["mp"]
    adv, inst = to_device(*synthetic_witness(4, 3))
    for bad_adv, bad_inst in ((adv[:, :2], inst), (adv.cpu(), inst), (adv, inst[:2]), (adv, [inst, inst]), (adv[:, :, ::2], inst),
                              (adv, torch.zeros((3, 17, 4), dtype=torch.int64, device="cuda")), (adv.to(torch.int32), inst)):
        with pytest.raises(ValueError):
            mp.verify(bad_adv, bad_inst)
    with pytest.raises(ValueError):
        mp.verify(adv, inst, max_failures=0)


# ---- the circuits' own witnesses -----------------------------------------------------------------------------------------
def around(*rows):
    return sorted({r + dr for r in rows for dr in (-1, 0, 1) if r + dr >= 0})


@pytest.mark.parametrize("depth", [1, 5])
def test_merkle_sum_tree_witnesses(depth):
    k, m, spec = 9, 5, ps.default_spec(5)
    rng = random.Random(depth)
    cs, lay = circuits.merkle_sum_tree(spec), sy.MerkleSumTreeLayout(depth, k, spec)
    mp = MockProver(cs, lay)
    leaves = [(rng.randrange(R), rng.randrange(1 << 40)) for _ in range(1 << depth)]
    tree = ps.MerkleSumTree.build(d([v for leaf in leaves for v in leaf]).reshape(1 << depth, 2, 4), spec)
    idx = [0, (1 << depth) - 1] + [rng.randrange(1 << depth) for _ in range(m - 2)]
    out = torch.full((m + 2, sy.N_ADVICE, 1 << k, 4), FILL, dtype=torch.int64, device="cuda")
    adv, inst = tree.witness(idx, 1 << 60, k, out=out[1:m + 1])              # a chunk of a larger buffer, filled in place
    assert mp.verify(adv, inst).ok and mp.verify(out[1:m + 1], [inst]).ok
    fixed, copies = lay.fixed_columns(), lay.copies()

    def check(a, i, touched, rows):
        got = mp.verify(a, i)
        want = expected(cs, fixed, a, [i], copies, touched, k, rows=rows)
        assert got.failures == want and got.users_failed == sorted({f[1] for f in want}) and want
        return want

    # assets below the root's balance: every user fails "check == is_lt" on the less-than row, nothing else
    low, low_inst = tree.witness(idx, 1 << 30, k)
    want = check(low, low_inst, list(range(m)), [lay.lt_row])
    assert want == [("gate", u, "check == is_lt", 0, lay.lt_row) for u in range(m)]
    # one flipped state word of one user
    a = adv.clone()
    row = lay.perm_row(depth - 1) + 10
    corrupt(a, 3, sy.STATE[1], row)
    want = check(a, inst, [3], around(row))
    assert {f[2] for f in want} == {"partial rounds"} and {f[1] for f in want} == {3}
    # a DIFF byte of 256 is not a byte
    a = adv.clone()
    a[1, sy.DIFF[0], lay.lt_row] = d([256])[0]
    want = check(a, inst, [1], [lay.lt_row])
    assert ("lookup", 1, 0, lay.lt_row) in want and {f[2] for f in want if f[0] == "gate"} == {"lt gate"}
    # the digest of level 0 no longer equals the next level's input (or the instance, at depth 1)
    a = adv.clone()
    _, col, row = lay.digest_cell(0)
    corrupt(a, 4, col, row)
    want = check(a, inst, [4], around(row))
    assert [f for f in want if f[0] == "copy"] and all(lay.digest_cell(0) in f[2:] for f in want if f[0] == "copy")


def test_merkle_sum_tree_unsatisfiable_inputs():
    """the two inputs of tests/test_witness_gpu.py that no witness can satisfy, as one call each"""
    spec = ps.default_spec(5)
    cs, lay = circuits.merkle_sum_tree(spec), sy.MerkleSumTreeLayout(5, 9, spec)
    mp = MockProver(cs, lay)
    leaf, sib, bits = golden()
    for sibs, assets, must in ((sib, 200, {"check == is_lt"}), ([(1, 1 << 65)] + sib[1:], 500, {"lt gate", "check == is_lt"})):
        adv, inst = sy.merkle_sum_witness(spec, *_path_tensors(leaf, sibs, bits), assets, 9)
        res = mp.verify(adv, inst)
        assert res.failures == expected(cs, lay.fixed_columns(), adv, [inst], lay.copies(), [0], 9, rows=around(lay.lt_row))
        assert {f[2] for f in res.failures} == must and {f[4] for f in res.failures} == {lay.lt_row} and res.total["gate"] == len(res.failures)


@pytest.mark.parametrize("depth", [1, 5])
def test_merkle_v3_witnesses(depth):
    k, m, spec = 9, 5, ps.default_spec(3)
    rng = random.Random(30 + depth)
    cs, lay = circuits.merkle_v3(spec), sy.MerkleTreeV3Layout(depth, k, spec)
    mp = MockProver(cs, lay)
    tree = ps.MerkleTree.build(d([rng.randrange(R) for _ in range(1 << depth)]), spec)
    adv, inst = tree.witness([0, (1 << depth) - 1] + [rng.randrange(1 << depth) for _ in range(m - 2)], k)
    assert mp.verify(adv, inst).ok
    a = adv.clone()
    row = lay.perm_row(depth - 1) + 10
    corrupt(a, 2, lay.STATE[1], row)
    got = mp.verify(a, inst)
    assert got.failures == expected(cs, lay.fixed_columns(), a, [inst], lay.copies(), [2], k, rows=around(row))
    assert {f[2] for f in got.failures} == {"partial rounds"} and got.users_failed == [2]
    i = inst.clone()
    corrupt(i, 0, 1)                                                          # the root this user claims
    got = mp.verify(adv, i)
    assert got.failures == expected(cs, lay.fixed_columns(), adv, [i], lay.copies(), [0], k, rows=[0]) and got.total == {"gate": 0, "copy": 1, "lookup": 0}


def test_poseidon_circuit_witnesses():
    k, m, spec = 9, 5, ps.default_spec(5)
    rng = random.Random(77)
    cs, lay = circuits.poseidon(spec), sy.PoseidonCircuitLayout(k, spec)
    mp = MockProver(cs, lay)
    adv, inst = sy.poseidon_circuit_witness(spec, d([rng.randrange(R) for _ in range(4 * m)]).reshape(m, 4, 4), k)
    assert mp.verify(adv, inst).ok
    a = adv.clone()
    row = lay.perm_row(0) + 20
    corrupt(a, 4, lay.STATE[3], row)
    got = mp.verify(a, inst)
    assert got.failures and got.failures == expected(cs, lay.fixed_columns(), a, [inst], lay.copies(), [4], k, rows=around(row))


def test_what_the_checker_rejects_does_not_verify():
    """depth 5 / k = 9: the witness MockProver accepts proves and verifies; the one it rejects gives a proof that does not"""
    cs, lay, advice, instance, cells = pc.build("merkle_sum_d5_k9")
    mp = MockProver(cs, lay)
    inst = pc.d(instance).reshape(1, 4, 4)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    try:
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        bad = pc.tampered(advice, cells["sum"])
        assert mp.verify(advice, inst).ok
        res = mp.verify(bad, inst)
        assert not res.ok and "sum constraint" in {f[2] for f in res.failures if f[0] == "gate"}
        assert h.verify_proof(params, vk, instance, h.create_proof(params, pk, advice, instance, 7), trapdoor=pc.SRS_S)
        assert not h.verify_proof(params, vk, instance, h.create_proof(params, pk, bad, instance, 7), trapdoor=pc.SRS_S)
    finally:
        params.release()
