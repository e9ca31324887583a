"""Every element of a proof through the host verifier, without a GPU: on the recorded proofs (tests/golden/) every scalar and every
point slot is changed in every constructed way of tests/proof_mutations.py -- a well-formed wrong value, a non-canonical encoding of
the SAME value, zero, the negated point, P + G, the identity, a point off the curve -- and every pair of slots the swaps name is
exchanged; ``verify_proof`` / ``verify_proof_multi`` must refuse every one.  A wrong computation makes honest proofs fail and the
other tests see it; what these see is an element that is read but not bound, a high bit that is ignored, a scalar reduced instead of
refused, a set whose order is not bound.

The builder is pinned first (the class table against the host decoder, the counts against the layout), and the driver is shown to
have teeth: a verifier that ignores one slot is reported at exactly that slot's mutants.  The sweep is parametrised by (proof, kind of
element, chunk) so that no item runs more than a few seconds; the verdict of every byte string is computed once and shared."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import poseidon as ps, proof_layout as pl
from halo2_experiments_amd.domain import EvaluationDomain
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.kzg import G2_GENERATOR, g2_bytes, g2_mul

import gwc_cases as gc
import proof_mutations as pm
import prover_cases as pc
from conftest import GOLDEN

PARAMS = SimpleNamespace(g2=g2_bytes(G2_GENERATOR), s_g2=g2_bytes(g2_mul(pc.SRS_S)))
CHUNK = 24                                       # mutants per item: about half decode, at 0.1 - 0.2 s per host verification
RECORDED = [(system, mo, enc) for system in ("poseidon", "overflow_check_v2") for mo in ("gwc", "shplonk") for enc in ("halo2", "evm")]
PROOFS = ["poseidon_k6", "poseidon_k6_x3"] + [f"{system}:{mo}_{enc}" for system, mo, enc in RECORDED]
# what ProofLayout can emit for lookup="halo2": every kind of point, and perm_z only where a last-row evaluation exists
KINDS_HALO2 = {"advice", "lookup_a", "lookup_s", "lookup_z", "perm_z", "random", "h_piece", "h1", "h2", "w"}

_CASES: dict = {}


def case(name):
    """the recorded proof ``name`` with its layout, key, instance, mutants and a verifier of byte strings that remembers its answers"""
    if name in _CASES:
        return _CASES[name]
    if ":" in name:
        system, mode = name.split(":")
        mo, enc = mode.split("_")
        rec = gc.recorded(system)
        cs, k, vk, instance, proof, m = rec["case"].cs, rec["case"].k, rec["vk"], rec["instance"], rec["proofs"][(mo, enc)], 1
    else:
        cs, k = pc.constraint_system("poseidon_k6")
        meta = np.load(os.path.join(GOLDEN, f"proof_{name}.npz"))
        vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
        proof = open(os.path.join(GOLDEN, f"proof_{name}.bin"), "rb").read()
        m, mo, enc = (3, "shplonk", "halo2") if name.endswith("_x3") else (1, "shplonk", "halo2")
        instance = [ps.words_to_ints(i) for i in meta["instances"]] if m > 1 else ps.words_to_ints(meta["instance"])
    layout = pl.ProofLayout(cs, k, enc, m, mo)
    c = SimpleNamespace(name=name, cs=cs, vk=vk, instance=instance, proof=proof, layout=layout, skipped=[], verdicts={})
    c.mutants = pm.mutants(layout, proof, c.skipped)

    def verify(data: bytes, vk=vk, instance=instance, trapdoor=pc.SRS_S) -> bool:
        if m > 1:
            return h.verify_proof_multi(PARAMS, vk, instance, data, trapdoor=trapdoor)
        return h.verify_proof(PARAMS, vk, instance, data, trapdoor=trapdoor, encoding=enc, multiopen=mo)

    def remembered(data: bytes) -> bool:
        if data not in c.verdicts:
            c.verdicts[data] = bool(verify(data))
        return c.verdicts[data]

    c.verify, c.remembered = verify, remembered
    _CASES[name] = c
    return c


def kind_of_mutant(m) -> str:
    key = m.key[0] if m.klass == "swap" else m.key
    return pm.kind_of(key, not (isinstance(key[0], tuple)))


def items():
    """(proof, kind, chunk) for every chunk of at most CHUNK mutants of one kind of one proof"""
    out = []
    for name in PROOFS:
        by_kind: dict = {}
        for m in case(name).mutants:
            by_kind.setdefault(kind_of_mutant(m), []).append(m)
        for kind, ms in by_kind.items():
            out += [(name, kind, i) for i in range((len(ms) + CHUNK - 1) // CHUNK)]
    return out


ITEMS = items()


# ---- the builder, pinned ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROOFS)
def test_the_mutants_are_what_their_class_says(name):
    c = case(name)
    lay = c.layout
    assert c.remembered(c.proof), "the untouched proof is the control of every item"
    assert len(c.skipped) <= 1, f"{len(c.skipped)} byte-equal swap pairs left out: {c.skipped}"
    assert len(c.mutants) + len(c.skipped) == pm.expected_count(lay) \
        == 3 * lay.n_scalars + 5 * lay.n_points + pm.swap_count(lay), f"{len(c.skipped)} byte-equal swap pairs left out"
    assert len(pm.POINT_CLASSES[lay.encoding]) == 5                     # no class is absent for either encoding: x + p always fits
    assert len({m.bytes for m in c.mutants}) == len(c.mutants) and c.proof not in {m.bytes for m in c.mutants}
    assert len({m.label for m in c.mutants}) == len(c.mutants)
    seen = set()
    for m in c.mutants:
        assert len(m.bytes) == len(c.proof)
        reads = pm.decodes(lay, m.bytes)
        if m.klass in pm.MUST_DECODE:
            assert reads, m.label
        elif m.klass in pm.MUST_NOT_DECODE:
            assert not reads, m.label
        else:
            assert m.klass in ("zero", "identity"), m.label
            assert reads == (m.klass == "zero"), m.label              # what the decoder says of them; the table names neither
        seen.add(m.klass)
        # a single-slot mutant differs from the proof inside its own element only
        if m.klass != "swap":
            w = pm.width(lay) if m.slot in lay.point_slots else 1
            assert m.bytes[:32 * m.slot] == c.proof[:32 * m.slot] and m.bytes[32 * (m.slot + w):] == c.proof[32 * (m.slot + w):], m.label
    assert seen == set(pm.SCALAR_CLASSES) | set(pm.POINT_CLASSES[lay.encoding]) | {"swap"}
    # the values, through the decoder: plus_r is the SAME residue, plus_one the next, negated the other y, plus_g another point
    points, scalars = pl.read_proof_ints(lay, c.proof)
    order = "big" if lay.encoding == "evm" else "little"
    by = {(m.klass, m.slot): m for m in c.mutants if m.klass != "swap"}
    for i, s in enumerate(lay.scalar_slots):
        raw = int.from_bytes(by["plus_r", s].bytes[32 * s:32 * s + 32], order)
        assert raw >= pl.R and raw % pl.R == scalars[i]
        assert pl.read_proof_ints(lay, by["plus_one", s].bytes)[1][i] == (scalars[i] + 1) % pl.R
    for i, s in enumerate(lay.point_slots):
        x, y = points[i]
        assert pl.read_proof_ints(lay, by["negated", s].bytes)[0][i] == (x, pm.P - y)
        other = pl.read_proof_ints(lay, by["plus_g", s].bytes)[0][i]
        assert other[0] != x and pm.g1_on_curve(other)


def test_swaps_and_circuits():
    """what the swaps are on the three-circuit proof: per kind the first two and the last two, and every per-circuit element of
    circuit 0 with circuit 2's"""
    c = case("poseidon_k6_x3")
    lay = c.layout
    swaps = [m for m in c.mutants if m.klass == "swap"]
    across = [m for m in swaps if pm.circuit_of(lay, m.key[0], m.slot[0] in lay.point_slots)
              and pm.circuit_of(lay, m.key[0], m.slot[0] in lay.point_slots)[0] == pm.circuit_of(lay, m.key[1], m.slot[1] in lay.point_slots)[0]]
    per_circuit = sum(key[0] in ("advice", "perm_z") for key in lay.lane.point_keys) + sum(key[0][0] in ("advice", "perm_z") for key in lay.lane.eval_keys)
    assert len(across) == per_circuit == 6 + 2 + 16 + 5
    assert {pm.circuit_of(lay, m.key[0], m.slot[0] in lay.point_slots)[1] for m in across} == {0}
    assert {pm.circuit_of(lay, m.key[1], m.slot[1] in lay.point_slots)[1] for m in across} == {2}
    assert ((("advice", 0, 0), ("advice", 1, 0)) in {m.key for m in swaps}) and ((("advice", 4, 2), ("advice", 5, 2)) in {m.key for m in swaps})


def test_the_kinds_covered_are_the_kinds_a_layout_can_emit():
    covered = set()
    for name in PROOFS:
        covered |= pm.kinds_covered(case(name).layout)
    assert covered == KINDS_HALO2                                      # logup_m / logup_phi: tests/test_proof_sweep_gpu.py makes that proof
    assert all(case(name).layout.nsets >= 2 for name in PROOFS)         # every proof here has the last-row evaluation of a perm_z


def test_byte_flips_cover_every_byte_once():
    for name in ("poseidon_k6", "poseidon:shplonk_evm", "poseidon:gwc_halo2"):
        c = case(name)
        flips = pm.byte_flips(c.layout, c.proof, random.Random(name))
        assert len(flips) == len(c.proof) == 32 * c.layout.slots
        where = []
        for m in flips:
            diff = [i for i in range(len(c.proof)) if m.bytes[i] != c.proof[i]]
            assert len(diff) == 1 and bin(m.bytes[diff[0]] ^ c.proof[diff[0]]).count("1") == 1
            assert 32 * m.slot <= diff[0] < 32 * (m.slot + (pm.width(c.layout) if m.slot in c.layout.point_slots else 1))
            where.append(diff[0])
        assert where == list(range(len(c.proof)))
        assert pm.byte_flips(c.layout, c.proof, random.Random(name)) == flips


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,chunk", ITEMS, ids=[f"{n}-{k}-{i}" for n, k, i in ITEMS])
def test_every_mutant_is_refused(name, kind, chunk):
    c = case(name)
    ms = [m for m in c.mutants if kind_of_mutant(m) == kind][CHUNK * chunk:CHUNK * (chunk + 1)]
    assert ms and c.remembered(c.proof)                                   # the control
    accepted = pm.sweep(c.remembered, ms)
    assert not accepted, [m.label for m in accepted]


def test_the_items_cover_every_mutant_once():
    for name in PROOFS:
        c = case(name)
        covered = [m.label for n, kind, chunk in ITEMS if n == name
                   for m in [m for m in c.mutants if kind_of_mutant(m) == kind][CHUNK * chunk:CHUNK * (chunk + 1)]]
        assert sorted(covered) == sorted(m.label for m in c.mutants)


@pytest.mark.parametrize("name", PROOFS)
def test_the_pairing_agrees_with_the_trapdoor(name):
    c = case(name)
    picked = pm.one_per_class(c.mutants)
    assert len(picked) == 9
    assert c.verify(c.proof, trapdoor=None)
    for m in picked:
        assert c.verify(m.bytes, trapdoor=None) is c.remembered(m.bytes) is False, m.label


# ---- the driver has teeth -----------------------------------------------------------------------------------------------------------------
def chosen_slots(lay):
    """an advice commitment, the last perm_z evaluation, h2"""
    advice = lay.point_slots[lay.point_keys.index(("advice", 1))]
    last_z = lay.scalar_slots[max(i for i, (key, _) in enumerate(lay.eval_keys) if key[0] == "perm_z")]
    h2 = lay.point_slots[lay.point_keys.index(("h2",))]
    assert h2 == lay.slots - 1
    return {"advice": advice, "last perm_z evaluation": last_z, "h2": h2}


@pytest.mark.parametrize("which", ["advice", "last perm_z evaluation", "h2"])
def test_a_verifier_that_ignores_one_slot_is_reported_at_that_slot(which):
    """``verify_proof`` behind a wrapper that puts the original bytes of ONE slot back first -- a verifier that does not read that
    slot.  The sweep reports that slot's single-slot mutants, all of them, and nothing else.  A swap that touches the slot is NOT
    among them: its other half still holds foreign bytes, which a verifier ignoring one slot still sees; the next test covers swaps."""
    c = case("poseidon_k6")
    slot = chosen_slots(c.layout)[which]
    ignoring = lambda data: c.remembered(data[:32 * slot] + c.proof[32 * slot:32 * slot + 32] + data[32 * slot + 32:])
    accepted = pm.sweep(ignoring, c.mutants)
    want = [m for m in c.mutants if m.klass != "swap" and m.slot == slot]
    assert len(want) == (3 if which == "last perm_z evaluation" else 5)
    assert accepted == want, ([m.label for m in accepted], [m.label for m in want])
    assert pm.sweep(c.remembered, want) == []                             # and the real verifier refuses each of them


@pytest.mark.parametrize("which", ["advice", "last perm_z evaluation"])
def test_a_verifier_that_does_not_bind_the_order_is_reported_at_that_swap(which):
    """``verify_proof`` behind a wrapper that sorts the contents of two slots of one kind back into place: a verifier that binds the
    set but not its order.  The sweep reports the swap of those two slots and nothing else."""
    c = case("poseidon_k6")
    slot = chosen_slots(c.layout)[which]
    swap = next(m for m in c.mutants if m.klass == "swap" and pm.touches(m, slot))
    a, b = swap.slot
    cut = lambda data, s: data[32 * s:32 * s + 32]

    def unordered(data):
        if cut(data, a) == cut(c.proof, b) and cut(data, b) == cut(c.proof, a):
            data = pm._put(pm._put(data, a, cut(c.proof, a)), b, cut(c.proof, b))
        return c.remembered(data)

    assert pm.sweep(unordered, c.mutants) == [swap]
    assert not c.remembered(swap.bytes)


# ---- instance and key ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poseidon_k6", "poseidon_k6_x3", "poseidon:gwc_evm"])
def test_every_instance_value_is_bound(name):
    c = case(name)
    changed = pm.instance_mutants(c.layout, c.instance)
    assert len(changed) == c.layout.circuits * sum(len(col) for col in pl._layout_instances(c.layout.lane, c.instance[0] if c.layout.circuits > 1 else c.instance)) >= 1
    assert c.verify(c.proof, instance=c.instance)
    for label, inst in changed:
        assert inst != c.instance and not c.verify(c.proof, instance=inst), label


@pytest.mark.parametrize("name", ["poseidon_k6", "overflow_check_v2:shplonk_halo2", "overflow_check_v2:gwc_evm"])
def test_every_commitment_of_the_key_is_bound(name):
    c = case(name)
    keys = pm.key_mutants(c.vk)
    assert len(keys) == c.cs.num_fixed + len(c.cs.equality) >= 2
    assert c.verify(c.proof, vk=c.vk)
    for label, vk in keys:
        assert not c.verify(c.proof, vk=vk), label
