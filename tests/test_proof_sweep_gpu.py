"""Every element of a proof through every device route of the verifier.  The proofs are made here, once per module, at the mutation
sweep's shapes (Poseidon k = 6, OverflowCheckV2<4, 4> k = 5 for the lookup kinds, three Poseidon circuits in one proof); the mutants
are tests/proof_mutations.py's.  One ``BatchVerifier`` per mode holds EVERY constructed mutant and swap of one proof between untouched
controls (first, 63, 64, last): ``verdicts()`` must be True exactly at the controls, the read kernel's flags must equal the host
twin's (``malformed()``) member by member and the class table, ``finalize()`` must be False.  With ``transcript="device"`` that is the
Blake2b / Keccak kernel binding every slot, with ``pairing="device"`` the device pairing refusing every well-formed wrong proof.  Then
a bit flipped in every byte of a proof (1856 members for Poseidon, 2368 in the "evm" encoding) in one launch per slot range; GWC,
which has no verdict per proof, through ``failing()`` by bisection kind by kind; the wrappers; every instance value; the key's
commitments; and a logUp proof -- which only ``verify_proof`` reads -- through the host sweep over all its elements."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import proof_layout as pl, synthesis as sy
from halo2_experiments_amd.kzg import ParamsKZG

import mutation_cases as mc
import proof_mutations as pm
import prover_multi_cases as pmc
from prover_cases import SRS_S

pytestmark = pytest.mark.gpu
SEED = 41
BYTE_PARTS = 4                                   # slot ranges of the every-byte batches: the host decoder's share is what is split
_KEYS: dict = {}
_PROOFS: dict = {}


@pytest.fixture(scope="module")
def keys():
    def get(name):
        if name not in _KEYS:
            c = mc.case(name)
            params = ParamsKZG.setup(c.k, SRS_S)
            vk = h.keygen_vk(params, c.cs, c.lay)
            advice = torch.from_numpy(sy.columns_to_words(c.advice).view(np.int64)).cuda()
            _KEYS[name] = dict(case=c, params=params, vk=vk, pk=h.keygen_pk(params, vk, c.cs, c.lay, cosets=False), advice=advice,
                               instance=c.proof_instance)
        return _KEYS[name]
    yield get
    for entry in _KEYS.values():
        entry["params"].release()
    _KEYS.clear()
    _PROOFS.clear()


def made(keys, name, encoding="halo2", multiopen="shplonk", circuits=1, lookup="halo2"):
    """one proof with its layout, instance, mutants and the host twin's classification of them, made once per mode"""
    at = (name, encoding, multiopen, circuits, lookup)
    if at in _PROOFS:
        return _PROOFS[at]
    key = keys(name)
    c = key["case"]
    if circuits > 1:
        _, _, adv, instance = pmc.build_multi("poseidon_k6", circuits, SEED)
        proof = h.create_proof_multi(key["params"], key["pk"], adv, instance, SEED)
    else:
        instance = key["instance"]
        proof = h.create_proof(key["params"], key["pk"], key["advice"], instance, SEED, encoding=encoding, multiopen=multiopen, lookup=lookup)
    layout = pl.ProofLayout(c.cs, c.k, encoding, circuits, multiopen, lookup)
    skipped = []
    mutants = pm.mutants(layout, proof, skipped)
    assert len(skipped) <= 1 and len(mutants) + len(skipped) == pm.expected_count(layout), f"{len(skipped)} byte-equal swap pairs left out: {skipped}"
    for m in mutants:
        if m.klass in pm.MUST_DECODE | pm.MUST_NOT_DECODE:
            assert pm.decodes(layout, m.bytes) == (m.klass in pm.MUST_DECODE), m.label
    entry = dict(key=key, instance=instance, proof=proof, layout=layout, mutants=mutants, modes=dict(encoding=encoding, multiopen=multiopen, circuits=circuits))
    _PROOFS[at] = entry
    return entry


def assemble(control, changed):
    """-> (members, the indices of the controls): ``changed`` between untouched controls at 0, 63, 64 (where the batch reaches them)
    and last"""
    n = len(changed) + 2
    inner = [i for i in (63, 64) if i < n + 1]
    n += len(inner)
    controls = sorted({0, n - 1, *inner})
    it = iter(changed)
    members = [control if b in controls else next(it) for b in range(n)]
    assert len(members) == len(changed) + len(controls) and next(it, None) is None
    return members, controls


def batch(p, members, **modes):
    bv = h.BatchVerifier(p["key"]["params"], p["key"]["vk"], seed=5, **dict(p["modes"], **modes))
    for inst, proof in members:
        bv.add_proof(inst, proof)
    return bv


def twin_flags(p, members):
    """``malformed()`` of the batch as a list of booleans: the integer twin, no device; the same for every mode of one batch"""
    if "flags" not in p:
        bv = batch(p, members)
        refused = set(bv.malformed())
        bv.close()
        p["flags"] = [b in refused for b in range(len(members))]
    return p["flags"]


# ---- verdicts: every constructed mutant of one proof in one launch per mode ------------------------------------------------------------------
# (system, encoding, circuits, pairing, transcript): the four pairing x transcript modes on halo2 / SHPLONK, then the other
# layouts with the transcript and the pairing on the device, then the circuit with lookups
VERDICT_MODES = [("poseidon", "halo2", 1, "host", "host"), ("poseidon", "halo2", 1, "host", "device"), ("poseidon", "halo2", 1, "device", "host"),
                 ("poseidon", "halo2", 1, "device", "device"), ("poseidon", "evm", 1, "device", "device"), ("poseidon", "evm", 1, "host", "host"),
                 ("poseidon", "halo2", 3, "device", "device"), ("overflow_check_v2", "halo2", 1, "device", "device"),
                 ("overflow_check_v2", "evm", 1, "device", "device")]


@pytest.mark.parametrize("name,encoding,circuits,pairing,transcript", VERDICT_MODES, ids=lambda v: str(v))
def test_verdicts_are_true_exactly_at_the_controls(keys, name, encoding, circuits, pairing, transcript):
    p = made(keys, name, encoding, circuits=circuits)
    control = (p["instance"], p["proof"])
    members, controls = assemble(control, [(p["instance"], m.bytes) for m in p["mutants"]])
    assert controls == [0, 63, 64, len(members) - 1]
    labels = iter(p["mutants"])
    by_index = [None if b in controls else next(labels) for b in range(len(members))]
    flags = twin_flags(p, members)
    for b, m in enumerate(by_index):                                         # the host twin against the class table
        if m is None:
            assert not flags[b], b
        elif m.klass in pm.MUST_DECODE | pm.MUST_NOT_DECODE:
            assert flags[b] == (m.klass in pm.MUST_NOT_DECODE), m.label
        else:
            assert flags[b] == (not pm.decodes(p["layout"], m.bytes)), m.label
    bv = batch(p, members, pairing=pairing, transcript=transcript)
    device_flags = bv._prepare()["bad"]
    wrong = [(b, by_index[b].label if by_index[b] else "control") for b in range(len(members)) if device_flags[b] != flags[b]]
    assert not wrong, f"the device's flags and malformed() disagree at {wrong}"
    # with the host's pairing a verdict costs one pairing on integers: the whole batch goes through the trapdoor, and the pairing
    # itself sees one mutant of every class below (test_the_wrappers_agree_on_a_mixed_batch)
    verdicts = bv.verdicts() if pairing == "device" else bv.verdicts(trapdoor=SRS_S)
    accepted = [by_index[b].label for b in range(len(members)) if verdicts[b] and by_index[b] is not None]
    assert not accepted, f"accepted: {accepted}"
    assert [b for b, ok in enumerate(verdicts) if ok] == controls
    assert bv.finalize() is False and bv.finalize(trapdoor=SRS_S) is False
    bv.close()


# ---- every byte ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(BYTE_PARTS))
@pytest.mark.parametrize("encoding", ["halo2", "evm"])
def test_a_flipped_bit_in_any_byte_is_refused(keys, encoding, part):
    p = made(keys, "poseidon", encoding)
    lay = p["layout"]
    flips = pm.byte_flips(lay, p["proof"], random.Random(f"{encoding} bytes"))
    assert len(flips) == 32 * lay.slots == {"halo2": 1856, "evm": 2368}[encoding]
    bounds = [lay.slots * i // BYTE_PARTS for i in range(BYTE_PARTS + 1)]
    mine = [m for m in flips if bounds[part] <= m.slot < bounds[part + 1]]
    assert sum(len([m for m in flips if bounds[i] <= m.slot < bounds[i + 1]]) for i in range(BYTE_PARTS)) == len(flips) and len(mine) > 256
    members, controls = assemble((p["instance"], p["proof"]), [(p["instance"], m.bytes) for m in mine])
    it = iter(mine)
    by_index = [None if b in controls else next(it) for b in range(len(members))]
    bv = batch(p, members, pairing="device", transcript="device")
    verdicts = bv.verdicts()
    assert [b for b, ok in enumerate(verdicts) if ok] == controls, [by_index[b].label for b, ok in enumerate(verdicts) if ok and by_index[b]]
    device_flags = bv._prepare()["bad"]
    wrong = [by_index[b].label for b in range(len(members)) if by_index[b] and device_flags[b] != (not pm.decodes(lay, by_index[b].bytes))]
    assert not wrong and not any(device_flags[b] for b in controls), f"the device's flags and the host decoder disagree at {wrong}"
    assert any(device_flags)                                                  # both roads are walked: a flipped point rarely decodes,
    if any(m.slot in lay.scalar_slots for m in mine):                         # a flipped scalar mostly does
        assert not all(device_flags[b] for b in range(len(members)) if b not in controls)
    bv.close()


# ---- GWC: no verdict per proof, so failing() by bisection, kind by kind ----------------------------------------------------------------------
@pytest.mark.parametrize("half", ["points", "evaluations"])
@pytest.mark.parametrize("encoding", ["halo2", "evm"])
@pytest.mark.parametrize("name", ["poseidon", "overflow_check_v2"])
def test_gwc_names_the_first_and_last_mutant_of_every_kind(keys, name, encoding, half):
    p = made(keys, name, encoding, multiopen="gwc")
    lay = p["layout"]
    control = (p["instance"], p["proof"])
    by_kind: dict = {}
    for m in p["mutants"]:
        if m.klass in ("plus_one", "plus_g"):
            by_kind.setdefault(pm.kind_of(m.key, m.klass == "plus_g"), []).append(m)
    assert set(by_kind) == {pm.kind_of(e[0], e[3]) for e in pm.elements(lay)} and "w" in by_kind and len(by_kind) >= 10
    mine = {kind: ms for kind, ms in by_kind.items() if kind.startswith("eval:") == (half == "evaluations")}
    assert len(mine) >= 5
    for kind, ms in mine.items():
        members = [control] * 8
        members[2], members[5] = (p["instance"], ms[0].bytes), (p["instance"], ms[-1].bytes)
        bv = batch(p, members, pairing="device", transcript="device")
        assert bv.finalize() is False, kind
        assert bv.failing() == [2, 5], (kind, ms[0].label, ms[-1].label)
        bv.close()
    bv = batch(p, [control] * 8, pairing="device", transcript="device")          # the controls alone
    assert bv.finalize() is True and bv.failing() == []
    bv.close()


# ---- the wrappers, and the host's pairing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ["halo2", "evm"])
def test_the_wrappers_agree_on_a_mixed_batch(keys, encoding):
    p = made(keys, "poseidon", encoding)
    picked = pm.one_per_class(p["mutants"])
    assert len(picked) == 9
    members, controls = assemble((p["instance"], p["proof"]), [(p["instance"], m.bytes) for m in picked])
    assert controls == [0, len(members) - 1]
    want = [b in controls for b in range(len(members))]
    insts, proofs = [i for i, _ in members], [q for _, q in members]
    params, vk = p["key"]["params"], p["key"]["vk"]
    for pairing, transcript in (("host", "host"), ("device", "device")):
        bv = batch(p, members, pairing=pairing, transcript=transcript)
        assert bv.verdicts() == want and bv.failing(method="each") == bv.failing() == [b for b in range(len(members)) if b not in controls]
        bv.close()
        assert h.verify_each(params, vk, insts, proofs, seed=9, pairing=pairing, transcript=transcript, encoding=encoding) == want
        assert h.verify_proofs(params, vk, insts, proofs, seed=9, pairing=pairing, transcript=transcript, encoding=encoding) is False
        assert h.verify_proofs(params, vk, [insts[0]] * 2, [proofs[0]] * 2, seed=9, pairing=pairing, transcript=transcript, encoding=encoding) is True


# ---- instance and key ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("circuits", [1, 3])
def test_every_instance_value_is_bound_on_the_device(keys, circuits):
    p = made(keys, "poseidon", circuits=circuits)
    changed = pm.instance_mutants(p["layout"], p["instance"])
    assert len(changed) == circuits * len(pl._layout_instances(p["layout"].lane, p["instance"][0] if circuits > 1 else p["instance"])[0]) >= circuits
    verify = (lambda inst: h.verify_proof_multi(p["key"]["params"], p["key"]["vk"], inst, p["proof"], trapdoor=SRS_S)) if circuits > 1 else \
        (lambda inst: h.verify_proof(p["key"]["params"], p["key"]["vk"], inst, p["proof"], trapdoor=SRS_S))
    assert verify(p["instance"]) and not any(verify(inst) for _, inst in changed)
    members, controls = assemble((p["instance"], p["proof"]), [(inst, p["proof"]) for _, inst in changed])
    for transcript in ("host", "device"):
        bv = batch(p, members, pairing="device", transcript=transcript)
        assert bv.verdicts() == [b in controls for b in range(len(members))] and bv.malformed() == [] and bv.finalize() is False
        bv.close()


@pytest.mark.parametrize("name", ["poseidon", "overflow_check_v2"])
def test_the_keys_commitments_are_bound_on_the_device(keys, name):
    p = made(keys, name)
    params, vk, cs = p["key"]["params"], p["key"]["vk"], p["key"]["case"].cs
    changed = pm.key_mutants(vk)
    assert len(changed) == cs.num_fixed + len(cs.equality)
    assert h.verify_proof(params, vk, p["instance"], p["proof"], trapdoor=SRS_S)
    for label, other in changed:                                               # every commitment on the host
        assert not h.verify_proof(params, other, p["instance"], p["proof"], trapdoor=SRS_S), label
    ends = [changed[0], changed[cs.num_fixed - 1], changed[cs.num_fixed], changed[-1]]
    assert [label for label, _ in ends] == ["fixed_0", f"fixed_{cs.num_fixed - 1}", "sigma_0", f"sigma_{len(cs.equality) - 1}"]
    for label, other in ends:                                                  # the first and the last of each on the device
        for transcript in ("host", "device"):
            bv = h.BatchVerifier(params, other, seed=5, pairing="device", transcript=transcript)
            for _ in range(3):
                bv.add_proof(p["instance"], p["proof"])
            assert bv.verdicts() == [False] * 3 and bv.finalize() is False, label
            bv.close()
    bv = h.BatchVerifier(params, vk, seed=5, pairing="device", transcript="device")     # the control: the key as it is
    bv.add_proof(p["instance"], p["proof"])
    assert bv.verdicts() == [True]
    bv.close()


# ---- logUp: the host verifier over all elements of a proof the device made --------------------------------------------------------------------
def _logup_layout():
    c = mc.case("overflow_check_v2")
    return pl.ProofLayout(c.cs, c.k, lookup="logup")


LOGUP_KINDS = sorted({pm.kind_of(e[0], e[3]) for e in pm.elements(_logup_layout())})


@pytest.mark.parametrize("kind", LOGUP_KINDS)
def test_a_logup_proof_through_the_host_sweep(keys, kind):
    p = made(keys, "overflow_check_v2", lookup="logup")
    params, vk = p["key"]["params"], p["key"]["vk"]
    if "verdicts" not in p:
        p["verdicts"] = {}

    def verify(data):
        if data not in p["verdicts"]:
            p["verdicts"][data] = bool(h.verify_proof(params, vk, p["instance"], data, trapdoor=SRS_S, lookup="logup"))
        return p["verdicts"][data]

    kind_of = lambda m: pm.kind_of(m.key[0] if m.klass == "swap" else m.key, not isinstance((m.key[0] if m.klass == "swap" else m.key)[0], tuple))
    assert sorted({kind_of(m) for m in p["mutants"]}) == LOGUP_KINDS and {"logup_m", "logup_phi", "eval:logup_m", "eval:logup_phi"} <= set(LOGUP_KINDS)
    mine = [m for m in p["mutants"] if kind_of(m) == kind]
    assert mine and verify(p["proof"])
    accepted = pm.sweep(verify, mine)
    assert not accepted, [m.label for m in accepted]
    for m in pm.one_per_class(mine):                                           # and through the pairing
        assert h.verify_proof(params, vk, p["instance"], m.bytes, lookup="logup") is False, m.label


def test_the_kinds_covered_are_the_kinds_a_layout_can_emit(keys):
    covered = set()
    for name in ("poseidon", "overflow_check_v2"):
        for multiopen in ("shplonk", "gwc"):
            covered |= pm.kinds_covered(made(keys, name, multiopen=multiopen)["layout"])
    covered |= pm.kinds_covered(made(keys, "overflow_check_v2", lookup="logup")["layout"])
    assert covered == {"advice", "lookup_a", "lookup_s", "lookup_z", "perm_z", "random", "h_piece", "h1", "h2", "w", "logup_m", "logup_phi"}
    assert all(made(keys, name)["layout"].nsets >= 2 for name in ("poseidon", "overflow_check_v2"))
