"""The mutation sweep on the GPU (tests/mutation_cases.py; the host half is tests/test_mutation_sweep.py): one satisfied witness per
circuit, replicated m times on the device with ONE cell changed in copy b, so that a single ``MockProver.verify`` call judges every
mutant and ``users_failed`` is the verdict per cell.  The device checker, ``create_proofs`` and the batch verifier must each give the
yardstick's verdict for every single cell: the failing users, the exact totals per kind, the proofs that do not verify.

The ``whole`` path of ``MockProver.verify`` (every polynomial over the whole batch) is taken when the first pass flags more lanes than
``max_records``; the checker for those calls is built with ``max_records = 4096`` and the batch tiled until more than 4096 lanes fail."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, poseidon as ps
from halo2_experiments_amd.batch_verifier import BatchVerifier
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.mock_prover import KINDS, MockProver

import mutation_cases as mc
from prover_cases import SRS_S

pytestmark = pytest.mark.gpu
ADVICE_BYTES = 1 << 30                    # at most this much advice in one verify call
FILL = 0x5A5A5A5A5A5A5A5A


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


_BASE = {}


def base(c):
    """the case's witness on the device, uploaded once: advice (num_advice, n, 4), instance (rows, 4) or None"""
    if c.name not in _BASE:
        adv = d([v for col in c.advice for v in col]).reshape(c.cs.num_advice, c.n, 4)
        inst = d(c.instance[0][:c.inst_rows]) if c.inst_rows else None
        _BASE[c.name] = (adv, inst)
    return _BASE[c.name]


def batch(c, cells, delta, kind="advice", out=None):
    """-> (advice (m, num_advice, n, 4), instance (m, rows, 4) or None): copy b is the witness with cells[b] plus delta mod r"""
    m = len(cells)
    adv0, inst0 = base(c)
    assert m * adv0.numel() * 8 <= ADVICE_BYTES
    adv = torch.empty((m,) + tuple(adv0.shape), dtype=torch.int64, device="cuda") if out is None else out
    adv.copy_(adv0)
    inst = inst0.unsqueeze(0).repeat(m, 1, 1) if inst0 is not None else None
    source = c.advice if kind == "advice" else c.instance
    new = d([(source[col][row] + delta) % R for col, row in cells])
    users = torch.arange(m, device="cuda")
    cols = torch.tensor([col for col, _ in cells], device="cuda")
    rows = torch.tensor([row for _, row in cells], device="cuda")
    if kind == "advice":
        adv[users, cols, rows] = new
    else:
        inst[users, rows] = new
    return adv, inst


def totals(verdicts):
    return {kind: sum(v[i] for v in verdicts) for i, kind in enumerate(KINDS)}


def failing(verdicts):
    return [b for b, v in enumerate(verdicts) if any(v[:3])]


_CHECKERS = {}


def checker(c, **kw):
    key = (c.name, tuple(sorted(kw.items())))
    if key not in _CHECKERS:
        _CHECKERS[key] = MockProver(c.cs, c.lay, **kw)
    return _CHECKERS[key]


# ---- a. the device checker against the yardstick, every mutant -------------------------------------------------------------------------
@pytest.mark.parametrize("delta_name", list(mc.DELTAS))
@pytest.mark.parametrize("name", mc.NAMES)
def test_the_device_checker_judges_every_mutant_as_the_yardstick_does(name, delta_name):
    c, delta = mc.case(name), mc.DELTAS[delta_name]
    cells, verdicts = mc.verdicts(name, delta_name)
    m, mp = len(cells), checker(c)
    want_total, want_failed = totals(verdicts), failing(verdicts)
    assert want_failed and len(want_failed) < m                                # both classes are there
    assert (want_total["lookup"] > 0) == (bool(c.cs.lookups) and (delta_name == "random" or name == "overflow_check_v2"))
    adv, inst = batch(c, cells, delta)
    assert mp.verify(base(c)[0], None if inst is None else inst[:1]).ok        # the witness itself is satisfied
    res = mp.verify(adv, inst)
    print(name, delta_name, "mutants", m, "failing", len(want_failed), "totals", res.total)
    assert res.users_failed == want_failed and res.total == want_total and not res.ok
    few = mp.verify(adv, inst, max_failures=8)
    assert few.users_failed == want_failed and few.total == want_total
    assert all(sum(f[0] == kind for f in few.failures) <= 8 for kind in KINDS)
    assert few.failures == sorted(sum(([f for f in res.failures if f[0] == kind][:8] for kind in KINDS), []))
    # every record names a user the yardstick fails with a failure of that kind
    index = {kind: i for i, kind in enumerate(KINDS)}
    assert all(verdicts[f[1]][index[f[0]]] for f in res.failures)
    del adv
    # the same batch as a chunk of a larger buffer
    out = torch.full((m + 2,) + tuple(base(c)[0].shape), FILL, dtype=torch.int64, device="cuda")
    chunk, inst = batch(c, cells, delta, out=out[1:m + 1])
    assert chunk.data_ptr() == out[1].data_ptr()
    part = mp.verify(chunk, inst)
    assert part.users_failed == want_failed and part.total == want_total and part.failures == res.failures
    assert bool((out[0] == FILL).all()) and bool((out[m + 1] == FILL).all())


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_whole_path_gives_the_same_verdicts(name):
    """more flagged lanes than records are kept (max_records = 4096): every polynomial runs over the whole batch; totals and flags stay exact"""
    c = mc.case(name)
    cells, verdicts = mc.verdicts(name, "one")
    order = sorted(range(len(cells)), key=lambda b: -verdicts[b][3])
    caught = [b for b in order if verdicts[b][0]]
    unit = caught + [b for b in order if not any(verdicts[b][:3])][:16]        # every cell a gate catches, and 16 free ones
    m = min(8192, ADVICE_BYTES // (c.cs.num_advice * c.n * 32))
    picked = [unit[i % len(unit)] for i in range(m)]
    tiled_cells, tiled = [cells[b] for b in picked], [verdicts[b] for b in picked]
    lanes = sum(v[3] for v in tiled)
    mp = checker(c, max_records=4096)
    assert lanes > 4096 == mp.max_records and m <= 8192                        # the precondition of the whole path
    adv, inst = batch(c, tiled_cells, 1)
    flagged, kept = mp.unsatisfied_lanes(adv, inst, cap=16)
    assert flagged == lanes and kept.numel() == 16
    res = mp.verify(adv, inst)
    print(name, "whole path: m", m, "lanes", lanes, "totals", res.total)
    assert res.total == totals(tiled) and res.users_failed == failing(tiled)
    assert all(sum(f[0] == kind for f in res.failures) <= 1024 for kind in KINDS)
    assert all(tiled[f[1]][KINDS.index(f[0])] for f in res.failures)
    assert checker(c).verify(adv, inst).total == res.total                     # and the path that keeps every record agrees


def test_instance_cells_every_row_of_every_circuit():
    for name in mc.NAMES:
        c = mc.case(name)
        cells = mc.instance_mutants(c)
        if not cells:
            assert name == "overflow_check_v2" and c.lay.instance() == [[]]     # no instance rows: nothing to change
            continue
        named = [[pair for pair in c.copies if ("instance", 0, row) in pair] for _, row in cells]
        assert all(named)
        adv, inst = batch(c, cells, 1, kind="instance")
        res = checker(c).verify(adv, inst)
        assert res.users_failed == list(range(len(cells))) and res.total == {"gate": 0, "copy": sum(map(len, named)), "lookup": 0}
        assert res.failures == sorted(("copy", b) + pair for b, pairs in enumerate(named) for pair in pairs)
        assert mc.host_verdicts(c, cells, 1, kind="instance") == [(0, len(pairs), 0, 0) for pairs in named]


# ---- b. the prover and the verifier against the same verdicts -------------------------------------------------------------------------
_KEYS = {}


@pytest.fixture(scope="module")
def keys():
    def get(name):
        if name not in _KEYS:
            c = mc.case(name)
            params = ParamsKZG.setup(c.k, SRS_S)
            vk = h.keygen_vk(params, c.cs, c.lay)
            _KEYS[name] = dict(params=params, vk=vk, pk=h.keygen_pk(params, vk, c.cs, c.lay, cosets=False))
        return _KEYS[name]
    yield get
    for entry in _KEYS.values():
        entry["params"].release()
    _KEYS.clear()


def prove(c, key, cells, verdicts, delta=1):
    """one create_proofs call, seeds = the mutants' indices, for the mutants whose lookup inputs are all in their tables -- the call
    with the others in it must raise NOT_FOUND naming exactly their proofs -> {mutant index: proof}"""
    m = len(cells)
    adv, _ = batch(c, cells, delta)
    missing = [b for b in range(m) if verdicts[b][2]]
    if missing:
        with pytest.raises(_lib.Halo2Mi355xError) as e:
            h.create_proofs(key["params"], key["pk"], adv, [c.proof_instance] * m, list(range(m)))
        assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.proofs == missing
        lookup_of = {ins[0].column: li for li, (ins, _) in enumerate(c.cs.lookups)}
        assert sorted(e.value.missing) == sorted(lookup_of[cells[b][0]] for b in missing)
        assert all(f"proof {b} " in str(e.value) for b in missing)
    kept = [b for b in range(m) if not verdicts[b][2]]
    proofs = h.create_proofs(key["params"], key["pk"], adv[kept].contiguous() if missing else adv, [c.proof_instance] * len(kept), kept)
    return dict(zip(kept, proofs))


def judge(c, key, proofs, trapdoor=None):
    """one BatchVerifier with the pairing and the transcripts on the device over ``proofs`` ({mutant index: proof}) -> the mutants whose
    proof does not verify; with the trapdoor the bisection's checks are made in G1, finalize() still pairs"""
    order = sorted(proofs)
    bv = BatchVerifier(key["params"], key["vk"], seed=5, pairing="device", transcript="device")
    try:
        for b in order:
            bv.add_proof(c.proof_instance, proofs[b])
        bad = bv.failing(trapdoor)
        assert bv.finalize() == (not bad)
    finally:
        bv.close()
    return [order[i] for i in bad]


COLUMNS = {"poseidon": 6, "overflow_check_v2": 5, "merkle_v3": 7}
_PROVED = {}


def proved(name, keys):
    """every mutant (delta 1) of a small circuit proved in one call, once -> (case, cells, verdicts, {mutant index: proof})"""
    if name not in _PROVED:
        c = mc.case(name)
        cells, verdicts = mc.verdicts(name, "one")
        _PROVED[name] = (c, cells, verdicts, prove(c, keys(name), cells, verdicts))
    return _PROVED[name]


def rejected(verdicts):
    """the mutants that are proved and whose proof must not verify: a gate or a copy catches them"""
    return [b for b, v in enumerate(verdicts) if (v[0] or v[1]) and not v[2]]


@pytest.mark.parametrize("name", list(COLUMNS))
def test_every_mutant_is_proved_in_one_call(name, keys):
    """exhaustive: all 384 / 160 / 896 mutants in ONE create_proofs call with seeds 0 .. m - 1 (m in the hundreds in blockIdx.y), all of
    them in one batch verifier: the pairing on the device rejects the batch, and the bisection (its checks made with the trapdoor; the
    next test makes them with the pairing, column by column) names the mutants a gate or a copy catches.  A mutant in a blinding row
    verifies: the prover overwrites those rows."""
    c, cells, verdicts, proofs = proved(name, keys)
    missing = sum(1 for v in verdicts if v[2])
    assert c.cs.num_advice == COLUMNS[name] and len(proofs) == len(cells) - missing and (missing > 0) == (name == "overflow_check_v2")
    bad = judge(c, keys(name), proofs, trapdoor=SRS_S)
    print(name, "proofs", len(proofs), "failing", len(bad))
    assert bad == rejected(verdicts)
    blinding = [b for b, (_, row) in enumerate(cells) if row >= c.usable]
    assert len(blinding) == 6 * c.cs.num_advice and not set(blinding) & set(bad)
    # the host verifier on 16 mutants: 8 rejected, 8 accepted, two of those in blinding rows
    rng = random.Random(16)
    good = sorted(set(proofs) - set(bad) - set(blinding))          # none in the range check: every usable cell is constrained
    accepted = rng.sample(good, min(6, len(good)))
    for b in rng.sample(bad, 8) + accepted + rng.sample(blinding, 8 - len(accepted)):
        assert h.verify_proof(keys(name)["params"], keys(name)["vk"], c.proof_instance, proofs[b], trapdoor=SRS_S) == (b not in bad), b


@pytest.mark.parametrize("name, column", [(name, column) for name, count in COLUMNS.items() for column in range(count)])
def test_the_device_pairing_names_the_rejected_mutants(name, column, keys):
    """the same proofs, one advice column at a time (every row of it), through finalize() and failing() with every check a pairing on the
    device: the bisection makes some 4 checks per rejected proof, which is why the batch is split and not the mutant set shrunk"""
    c, cells, verdicts, proofs = proved(name, keys)
    mine = {b: proof for b, proof in proofs.items() if cells[b][0] == column}
    assert len(mine) == c.n - sum(1 for b, v in enumerate(verdicts) if v[2] and cells[b][0] == column)
    assert judge(c, keys(name), mine) == [b for b in rejected(verdicts) if cells[b][0] == column]


def test_a_batched_mutant_proof_has_create_proof_bytes(keys):
    c, cells, verdicts, proofs = proved("poseidon", keys)
    bad = rejected(verdicts)
    free = next(b for b, (_, row) in enumerate(cells) if b not in bad and row < c.usable and b > 100)
    for b in (bad[0], bad[-1], free):
        adv, _ = batch(c, [cells[b]], 1)
        assert h.create_proof(keys("poseidon")["params"], keys("poseidon")["pk"], adv[0], c.proof_instance, b) == proofs[b], b


def test_the_sum_tree_sample_proves_as_the_yardstick_judges(keys):
    c = mc.case("merkle_sum_tree")
    cells, verdicts = mc.verdicts(c.name, "one")
    verdict = dict(zip(cells, verdicts))
    sample = mc.sum_tree_sample(c)
    sets = mc.caught_by(cells, verdicts)
    assert len(sample) <= 128 and sets["copy"] - sets["gate"] <= set(sample)
    assert sum(1 for cell in sample if not any(verdict[cell][:3])) == 16 and sum(1 for _, row in sample if row >= c.usable) == 4
    proofs = prove(c, keys(c.name), sample, [verdict[cell] for cell in sample])
    bad = judge(c, keys(c.name), proofs)
    print(c.name, "proofs", len(proofs), "failing", len(bad))
    assert bad == [b for b, cell in enumerate(sample) if any(verdict[cell][:2])] and len(proofs) == len(sample)
    # a diff byte plus a random element is in no table: on the lt row and on a row where nothing else reads it
    random_verdict = dict(zip(*mc.verdicts(c.name, "random")))
    diff = [(col, c.lay.lt_row) for col in range(12, 20)] + [(13, 4), (19, 90)]
    few = [sample[0]] + diff[:5] + [sample[-1]] + diff[5:]
    assert all(random_verdict[cell][2] == 1 for cell in diff)
    judged = [random_verdict[cell] if cell in diff else (0, 0, 0, 0) for cell in few]      # only WHICH proofs miss a lookup input is asked
    adv, _ = batch(c, few, mc.DELTAS["random"])
    with pytest.raises(_lib.Halo2Mi355xError) as e:
        h.create_proofs(keys(c.name)["params"], keys(c.name)["pk"], adv, [c.proof_instance] * len(few), 0)
    assert e.value.code == _lib.HM_ERR_NOT_FOUND and e.value.proofs == [b for b, v in enumerate(judged) if v[2]]
    assert sorted(e.value.missing) == sorted(cell[0] - 12 for cell in diff)
