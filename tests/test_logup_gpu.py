"""The logUp lookup argument on the GPU: the two kernels against the pure-integer twin (tests/logup_twin.py), bit
for bit, at the shapes the host twins are held to in tests/test_logup_host.py; then ``lookup="logup"`` through the prover, the host
verifier, the solvency and ledger statements, on the mutation sweep's shapes.  Keys, parameters and witnesses are made once per
module and never changed."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, arithmetic, circuits, ledger as lg, poseidon as ps, prover, synthesis as sy
from halo2_experiments_amd.batch_verifier import BatchVerifier, verify_each, verify_proofs
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.proof_layout import ProofLayout
from halo2_experiments_amd.verifier import proof_length

import logup_twin as tw
import mutation_cases as mc
import safe_accumulator_cases as sc
from prover_cases import SRS_S

pytestmark = pytest.mark.gpu


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64).reshape(-1, 4))


# ---- the running sums ----------------------------------------------------------------------------------------------------------------------
def test_the_shapes_are_the_kernels_own():
    assert arithmetic.LOGUP_COUNT_BITS == tw.COUNT_BITS


@pytest.mark.parametrize("values", tw.GRAND_SUM_VALUES)
@pytest.mark.parametrize("n", tw.GRAND_SUM_LENGTHS)
def test_grand_sum_equals_the_twin(n, values):
    for count in (1, 3):
        columns = tw.grand_sum_columns(n, values, count)
        want = [tw.prefix_sums(col) for col in columns]
        terms = [d(col) for col in columns]
        keep = [t.clone() for t in terms]
        outs = h.grand_sum_batch(terms)
        assert [ints(o) for o in outs] == want and all(torch.equal(t, k) for t, k in zip(terms, keep))      # out of place
        guard = torch.full((count, n + 2, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        for j, t in enumerate(terms):
            guard[j, 1:n + 1] = t
        views = [guard[j, 1:n + 1] for j in range(count)]
        assert h.grand_sum_batch(views, outs=views)[0].data_ptr() == views[0].data_ptr()                      # in place
        assert [ints(v) for v in views] == want
        assert bool((guard[:, 0] == 0x5A5A5A5A5A5A5A5A).all()) and bool((guard[:, n + 1] == 0x5A5A5A5A5A5A5A5A).all())


# ---- the multiplicities --------------------------------------------------------------------------------------------------------------------
def run_multiplicities(cases, usable=None):
    """cases: [(table, inputs)] of one length -> ([m per argument as integers on the live rows], the tensors)"""
    rows = len(cases[0][0])
    n = rows + 3                                                                        # rows behind the live ones: left zero
    pad = lambda col: d(list(col) + [7] * (n - rows))
    tabs = [pad(table) for table, _ in cases]
    ins = [[pad(f) for f in inputs] for _, inputs in cases]
    outs = h.logup_multiplicities(tabs, ins, rows)
    assert all(not bool(o[rows:].any()) for o in outs)
    return [ints(o[:rows]) for o in outs]


@pytest.mark.parametrize("kind", tw.MULTIPLICITY_TABLES)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("rows", tw.MULTIPLICITY_ROWS)
def test_multiplicities_equal_the_twin(rows, c, kind):
    table, inputs = tw.multiplicity_case(rows, c, kind)
    want, missing = tw.multiplicities(table, inputs)
    assert not missing and (max(table) >= 1 << tw.COUNT_BITS) == (kind in ("at_switch", "wide"))      # the sorted records / the value bins
    assert run_multiplicities([(table, inputs)]) == [want]


@pytest.mark.parametrize("kinds", [["range", "hot", "below_switch", "range"], ["range", "wide", "at_switch", "hot"]])
def test_a_batch_of_arguments_and_a_missing_input(kinds):
    """four arguments with 3, 1, 2 and 3 inputs in ONE call, on the value bins and on the sorted records; then an input of argument 2
    leaves its table: NOT_FOUND naming that argument, the other arguments' columns complete"""
    rows = 65
    cases = []
    for a, (kind, c) in enumerate(zip(kinds, (3, 1, 2, 3))):
        cases.append(tw.multiplicity_case(rows, c, kind, seed=a))
    want = [tw.multiplicities(table, inputs)[0] for table, inputs in cases]
    assert run_multiplicities(cases) == want
    table, inputs = cases[2]
    inputs[1][64] = (max(table) + 1) % R if kinds[2] != "wide" else 5
    assert tw.multiplicities(table, inputs)[1]
    n = rows
    tabs = [d(t) for t, _ in cases]
    ins = [[d(f) for f in fs] for _, fs in cases]
    outs = list(torch.zeros((4, n, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.Halo2Mi355xError) as e:
        h.logup_multiplicities(tabs, ins, rows, outs=outs)
    assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.missing == [2]
    assert [ints(o) for a, o in enumerate(outs) if a != 2] == [w for a, w in enumerate(want) if a != 2]
    assert ints(outs[2]) == tw.multiplicities(table, inputs)[0]                          # the inputs that are in the table are counted


def test_the_c_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    rows = 8
    table, inputs = tw.multiplicity_case(rows, 2, "range")
    t, f0, f1 = d(table), d(inputs[0]), d(inputs[1])
    out = torch.full((rows + 1, 4), 0x33, dtype=torch.int64, device="cuda")
    arr = lambda ps_: (ctypes.c_void_p * len(ps_))(*ps_)
    cnt = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    call = lambda tabs, ins, counts, count, r, outs: lib.hm_logup_multiplicities_bn256_fr_dev(arr(tabs), arr(ins), cnt(*counts), count, r,
                                                                                            arr(outs), None, None)
    tp, ip, op = t.data_ptr(), [f0.data_ptr(), f1.data_ptr()], out.data_ptr()
    assert lib.hm_logup_multiplicities_bn256_fr_dev(None, None, None, 1, rows, None, None, None) == _lib.HM_ERR_BAD_ARG
    bad = [([tp], ip, [2], 1, 0, [op]),                      # rows = 0
           ([tp], ip, [2], 1, 1 << 31, [op]),                # rows out of range
           ([tp], ip, [0], 1, rows, [op]),                   # no input column
           ([tp], [ip[0]] * 2, [1 << 30, 1], 1, rows, [op]), # c * rows = 2^33
           ([None], ip, [2], 1, rows, [op]),                 # null table
           ([tp], [ip[0], None], [2], 1, rows, [op]),        # null input
           ([tp], ip, [2], 1, rows, [None]),                 # null output
           ([tp + 8], ip, [2], 1, rows, [op]),               # misaligned
           ([tp], ip, [2], 1, rows, [op + 8]),
           ([tp], ip, [2], 1, rows, [tp]),                   # the output is the table
           ([tp], ip, [2], 1, rows, [ip[1] + 32]),           # the output overlaps an input
           ([tp, tp], ip, [1, 1], 2, rows, [op, op + 32])]   # two outputs overlap
    for args in bad:
        assert call(*args) == _lib.HM_ERR_BAD_ARG, args
    assert lib.hm_logup_multiplicities_bn256_fr_dev(None, None, None, 0, rows, None, None, None) == _lib.HM_OK      # nothing to do
    gs = lambda terms, n, outs, count: lib.hm_fr_grand_sum_batch_dev(arr(terms), n, arr(outs), count, None)
    assert lib.hm_fr_grand_sum_batch_dev(None, rows, None, 1, None) == _lib.HM_ERR_BAD_ARG
    for args in [([tp], 0, [op], 1), ([tp], 1 << 32, [op], 1), ([None], rows, [op], 1), ([tp], rows, [None], 1), ([tp + 4], rows, [op], 1),
                 ([tp], rows, [tp + 32], 1), ([tp, ip[0]], rows, [op, tp], 2), ([tp, ip[0]], rows, [op, op + 32], 2)]:
        assert gs(*args) == _lib.HM_ERR_BAD_ARG, args
    assert lib.hm_fr_grand_sum_batch_dev(arr([tp]), rows, arr([op]), 70000, None) == _lib.HM_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x33).all()) and ints(t) == table and ints(f1) == inputs[1]
    with pytest.raises(ValueError):
        h.logup_multiplicities([t], [[]], rows)
    with pytest.raises(ValueError):
        h.logup_multiplicities([t], [[f0]], rows + 1)


# ---- proving and verifying -----------------------------------------------------------------------------------------------------------------
NAMES = ["merkle_sum_tree", "overflow_check_v2", "safe_accumulator", "sorted_column", "poseidon"]


def build(name):
    """-> cs, lay, k, the witness on the device, the instance as create_proof takes it, and the integer columns the twin reads"""
    if name in mc.NAMES:
        c = mc.case(name)
        adv = d([v for col in c.advice for v in col]).reshape(c.cs.num_advice, c.n, 4)
        return dict(cs=c.cs, lay=c.lay, k=c.k, adv=adv, instance=c.proof_instance, advice=c.advice, fixed=c.fixed)
    if name == "sorted_column":
        k, rows = 5, 26
        cs, lay = circuits.sorted_column(4, 4), sy.SortedColumnLayout(k, 4, 4, rows)
        rng = random.Random("logup sorted")
        ids = [rng.randrange(1 << 200)]
        for _ in range(rows - 1):
            ids.append(ids[-1] + rng.randrange(1, 1 << 16))
        adv, over = sy.sorted_witness(d(ids).reshape(1, rows, 4), k, 4, 4)
        assert over.cpu().tolist() == [0]
        return dict(cs=cs, lay=lay, k=k, adv=adv[0], instance=[[]], advice=lay.assign_ints(ids), fixed=lay.fixed_columns())
    k, b, A, rows = 5, 4, 4, 8
    cs, lay = circuits.safe_accumulator(b, A), sy.SafeAccumulatorLayout(k, b, A, rows)
    ini, vs = [0, 0, 1, 2], [(7 * r) % 16 for r in range(rows)]
    assert sc.satisfied(b, A, ini, vs)
    adv, finals, over = sy.accumulator_witness(d(vs).reshape(1, rows, 4), torch.tensor([ini], dtype=torch.int64, device="cuda"), k, b, A)
    assert over.cpu().tolist() == [0]
    return dict(cs=cs, lay=lay, k=k, adv=adv[0], instance=finals.cpu().tolist()[0], advice=None, fixed=None)


_MADE = {}


@pytest.fixture(scope="module")
def made():
    """name -> the case with its parameters and keys, a logUp proof with its trace and a halo2 proof of the same witness and seed"""
    def get(name):
        if name not in _MADE:
            c = build(name)
            params = ParamsKZG.setup(c["k"], SRS_S, keep_points=True)
            vk = h.keygen_vk(params, c["cs"], c["lay"])
            pk = h.keygen_pk(params, vk, c["cs"], c["lay"], cosets=False)
            digest = prover.vk_digest(vk)
            trace = {}
            logup = h.create_proof(params, pk, c["adv"], c["instance"], 77, _trace=trace, lookup="logup")
            halo2 = h.create_proof(params, pk, c["adv"], c["instance"], 77)
            assert prover.vk_digest(vk) == digest                                       # one key pair, either argument
            _MADE[name] = dict(c, params=params, vk=vk, pk=pk, logup=logup, halo2=halo2, trace=trace)
        return _MADE[name]
    yield get
    for entry in _MADE.values():
        entry["params"].release()
    _MADE.clear()


@pytest.mark.parametrize("name", NAMES)
def test_a_logup_proof_verifies_under_its_own_argument_only(made, name):
    c = made(name)
    p, vk, cs, inst = c["params"], c["vk"], c["cs"], c["instance"]
    assert h.verify_proof(p, vk, inst, c["logup"], lookup="logup") and h.verify_proof(p, vk, inst, c["logup"], trapdoor=SRS_S, lookup="logup")
    assert h.verify_proof(p, vk, inst, c["halo2"])
    assert len(c["logup"]) == proof_length(cs, lookup="logup") and len(c["halo2"]) == proof_length(cs)
    if cs.lookups:
        assert len(c["logup"]) < len(c["halo2"])
        assert not h.verify_proof(p, vk, inst, c["logup"]) and not h.verify_proof(p, vk, inst, c["halo2"], lookup="logup")
        assert not h.verify_proof(p, vk, inst, c["logup"][:len(c["halo2"])] + bytes(max(0, len(c["halo2"]) - len(c["logup"]))))
    else:
        assert cs.logup_arguments() == [] and c["logup"] == c["halo2"]                  # no lookups: the same bytes
    assert c["logup"][:32 * cs.num_advice] == c["halo2"][:32 * cs.num_advice]            # the advice commitments come first, unchanged
    print(name, "bytes", len(c["halo2"]), "->", len(c["logup"]))


@pytest.mark.parametrize("name", ["merkle_sum_tree", "overflow_check_v2", "sorted_column"])
def test_the_provers_columns_equal_the_twin(made, name):
    """m and phi of every argument (the prover's debug return) on the usable rows, against the integers: every lookup here reads one
    advice column and one fixed table column, so the compressed columns are the columns themselves"""
    c = made(name)
    cs, n = c["cs"], 1 << c["k"]
    u = n - cs.blinding_factors - 1
    lag, beta = c["trace"]["lagrange"], c["trace"]["challenges"]["beta"]
    groups = cs.logup_arguments()
    assert len(lag["logup_m"]) == len(lag["logup_phi"]) == len(groups) and lag["lookup_z"] == [] and lag["permuted"] == []
    for g, (tabs, ins_list) in enumerate(groups):
        table = c["fixed"][tabs[0].column][:u]
        inputs = [c["advice"][ins[0].column][:u] for ins in ins_list]
        m, missing = tw.multiplicities(table, inputs)
        assert not missing and ints(lag["logup_m"][g][:u]) == m and sum(m) == len(inputs) * u
        phi = tw.running_sum(table, inputs, m, beta)
        assert ints(lag["logup_phi"][g][:u + 1]) == phi and phi[u] == 0
    assert ("logup_m", 0) in c["trace"]["polys"] and ("logup_phi", 0) in c["trace"]["commits"]


def test_multi_circuit_and_batched_proofs():
    c = mc.case("overflow_check_v2")
    params = ParamsKZG.setup(c.k, SRS_S)
    try:
        vk = h.keygen_vk(params, c.cs, c.lay)
        pk = h.keygen_pk(params, vk, c.cs, c.lay, cosets=False)
        rng = random.Random(3)
        advs = torch.stack([d([v for col in c.lay.assign_ints([rng.randrange(1 << 16) for _ in range(26)]) for v in col])
                            .reshape(c.cs.num_advice, c.n, 4) for _ in range(3)])
        inst = [[[]]] * 3
        multi = h.create_proof_multi(params, pk, advs, inst, 5, lookup="logup")
        assert len(multi) == proof_length(c.cs, 3, lookup="logup")
        assert h.verify_proof_multi(params, vk, inst, multi, trapdoor=SRS_S, lookup="logup") and not h.verify_proof_multi(params, vk, inst, multi)
        assert h.verify_proof_multi(params, vk, inst, multi, lookup="logup")           # and with the pairing
        assert h.create_proof_multi(params, pk, advs[:1], inst[:1], 5, lookup="logup") == h.create_proof(params, pk, advs[0], [[]], 5, lookup="logup")
        proofs = h.create_proofs(params, pk, advs, inst, [11, 12, 13], lookup="logup")
        for b in range(3):
            assert proofs[b] == h.create_proof(params, pk, advs[b], [[]], 11 + b, lookup="logup"), b
            assert h.verify_proof(params, vk, [[]], proofs[b], trapdoor=SRS_S, lookup="logup")
        # an out-of-table limb: the error of today, naming proof and argument
        bad = advs.clone()
        bad[1, 3, 7] = d([16])[0]
        with pytest.raises(_lib.Halo2Mi355xError) as e:
            h.create_proofs(params, pk, bad, inst, [11, 12, 13], lookup="logup")
        assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.proofs == [1] and e.value.missing == [2] and "proof 1 (argument 2)" in str(e.value)
        with pytest.raises(_lib.Halo2Mi355xError) as e:
            h.create_proof(params, pk, bad[1], [[]], 5, lookup="logup")
        assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.missing == [2]
        with pytest.raises(_lib.Halo2Mi355xError) as e:
            h.create_proof(params, pk, bad[1], [[]], 5)
        assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.missing == [2]      # lookup 2 = argument 2 here: one input each
        for call in (lambda: h.create_proof(params, pk, advs[0], [[]], 5, lookup="mv"), lambda: h.verify_proof(params, vk, [[]], multi, lookup="mv"),
                     lambda: h.create_proofs(params, pk, advs, inst, 5, lookup="mv"), lambda: h.create_proof_multi(params, pk, advs, inst, 5, lookup="mv")):
            with pytest.raises(ValueError, match="lookup must be"):
                call()
    finally:
        params.release()


@pytest.mark.parametrize("name, encoding, multiopen", [("overflow_check_v2", "halo2", "gwc"), ("overflow_check_v2", "evm", "shplonk"),
                                                       ("overflow_check_v2", "evm", "gwc"), ("merkle_sum_tree", "evm", "gwc")])
def test_logup_composes_with_the_encoding_and_the_multiopen(made, name, encoding, multiopen):
    c = made(name)
    p, vk, inst = c["params"], c["vk"], c["instance"]
    proof = h.create_proof(p, c["pk"], c["adv"], inst, 78, encoding=encoding, multiopen=multiopen, lookup="logup")
    assert len(proof) == proof_length(c["cs"], 1, encoding, multiopen, c["k"], "logup")
    assert h.verify_proof(p, vk, inst, proof, trapdoor=SRS_S, encoding=encoding, multiopen=multiopen, lookup="logup")
    assert not h.verify_proof(p, vk, inst, proof, trapdoor=SRS_S, encoding=encoding, multiopen=multiopen)
    assert h.create_proofs(p, c["pk"], c["adv"].unsqueeze(0), [inst], [78], encoding=encoding, multiopen=multiopen, lookup="logup") == [proof]


@pytest.mark.parametrize("name", ["overflow_check_v2", "merkle_sum_tree"])
def test_a_flipped_byte_in_any_logup_element_is_rejected(made, name):
    """one byte in each m commitment, each phi commitment and each of the three evaluations per argument: False, never True (a byte
    that makes a point undecodable or a scalar too large is a TranscriptError inside verify_proof, which is False too)"""
    c = made(name)
    lay = ProofLayout(c["cs"], c["k"], lookup="logup")
    G = len(c["cs"].logup_arguments())
    slots = [lay.point_slots[i] for i, key in enumerate(lay.point_keys) if key[0] in ("logup_m", "logup_phi")]
    slots += [lay.scalar_slots[i] for i, (key, _) in enumerate(lay.eval_keys) if key[0] in ("logup_m", "logup_phi")]
    assert len(slots) == 5 * G and len(set(slots)) == 5 * G
    rng = random.Random(name)
    for s in slots:
        forged = bytearray(c["logup"])
        forged[32 * s + rng.randrange(31)] ^= 1 << rng.randrange(8)
        assert not h.verify_proof(c["params"], c["vk"], c["instance"], bytes(forged), trapdoor=SRS_S, lookup="logup"), s


def test_solvency_and_ledger_round_trip_under_logup():
    k, rows = 5, 26
    params = ParamsKZG.setup(k, SRS_S, keep_points=True)
    try:
        cs, lay = circuits.overflow_check_v2(4, 4, unblinded_value=True), sy.RangeCheckLayout(k, 4, 4, rows=rows)
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        id_cs, id_lay = circuits.sorted_column(4, 4), sy.SortedColumnLayout(k, 4, 4, rows=rows)
        id_vk = h.keygen_vk(params, id_cs, id_lay)
        id_pk = h.keygen_pk(params, id_vk, id_cs, id_lay, cosets=False)
        rng = random.Random("logup ledger")
        vals = [[rng.randrange(1 << 16) for _ in range(rows)] for _ in range(2)]
        bal = d([v for vs in vals for v in vs]).reshape(2, rows, 4)
        proof = h.prove_balances(params, pk, bal, seed=33, lookup="logup")
        assert h.verify_balances(params, vk, proof, lookup="logup") and not h.verify_balances(params, vk, proof)
        assert proof.commitments == h.prove_balances(params, pk, bal, seed=33).commitments                 # C_p is where it was
        openings = h.user_openings(params, proof)
        for i in (0, 25):
            assert h.verify_user(params, proof.commitments[1], i, vals[1][i], openings[1, i])
        ids = [rng.randrange(1 << 250)]
        for _ in range(rows - 1):
            ids.append(ids[-1] + rng.randrange(1, 1 << 16))
        led = lg.prove_ledger(params, pk, d(ids).reshape(rows, 4), bal, seed=90, id_pk=id_pk, lookup="logup")
        assert lg.verify_ledger(params, vk, led, id_vk=id_vk, lookup="logup") and not lg.verify_ledger(params, vk, led, id_vk=id_vk)
        assert h.verify_proof(params, id_vk, [[]], led.id_proof, lookup="logup")
        pis = lg.ledger_openings(params, led).cpu().numpy().view(np.uint64)
        for i in (0, 25):
            assert lg.verify_ledger_user(params, led, i, ids[i], [vs[i] for vs in vals], pis[i], rows=rows)
        for call in (lambda: h.prove_balances(params, pk, bal, seed=33, lookup="mv"), lambda: h.verify_balances(params, vk, proof, lookup="mv"),
                     lambda: lg.prove_ledger(params, pk, d(ids).reshape(rows, 4), bal, seed=90, lookup="mv"),
                     lambda: lg.verify_ledger(params, vk, led, lookup="mv")):
            with pytest.raises(ValueError, match="lookup must be"):
                call()
    finally:
        params.release()


def test_the_batch_verifier_refuses_logup(made):
    c = made("overflow_check_v2")
    with pytest.raises(ValueError, match="not batch-verified"):
        BatchVerifier(c["params"], c["vk"], seed=1, lookup="logup")
    with pytest.raises(ValueError, match="not batch-verified"):
        verify_proofs(c["params"], c["vk"], [c["instance"]], [c["logup"]], seed=1, lookup="logup")
    with pytest.raises(ValueError, match="not batch-verified"):
        verify_each(c["params"], c["vk"], [c["instance"]], [c["logup"]], seed=1, lookup="logup")
    with pytest.raises(ValueError, match="lookup must be"):
        BatchVerifier(c["params"], c["vk"], seed=1, lookup="mv")
    assert verify_proofs(c["params"], c["vk"], [c["instance"]], [c["halo2"]], seed=1, trapdoor=SRS_S)
