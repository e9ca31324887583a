"""create_proofs: m independent proofs of one key in one batched pass.  The defining property -- proof b is
``create_proof(params, pk, advice[b], instances[b], seeds[b])`` byte for byte -- for m = 1, 2, 3 on poseidon_k6 (no lookups) and
merkle_sum_d5_k9 (8 lookups, 3 permutation sets); the integer-seed shorthand; every proof verifies alone and the batch through the
BatchVerifier; a shrunk h budget (chunks of 2 + 1 proofs) gives the same bytes; a tampered witness in proof 1 breaks proof 1 and leaves
proofs 0 and 2 as they were; identical witnesses under different seeds are blinded differently; a lookup input missing from its table raises create_proof's
error naming the proof; the argument errors."""
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, prover, verifier
from halo2_experiments_amd.kzg import ParamsKZG

import prover_cases as pc
import prover_multi_cases as pmc

pytestmark = pytest.mark.gpu

CASES = ["poseidon_k6", "merkle_sum_d5_k9"]
SEEDS = [7, 1 << 20, 99]                       # pairwise distinct, not consecutive


@pytest.fixture(scope="module", params=CASES)
def keys(request):
    name = request.param
    cs, lay, advice, instances = pmc.build_multi(name, 3)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    singles = [h.create_proof(params, pk, advice[b], instances[b], SEEDS[b]) for b in range(3)]      # computed once, shared, never changed
    yield dict(name=name, cs=cs, lay=lay, params=params, vk=vk, pk=pk, advice=advice, instances=instances, singles=singles)
    params.release()


@pytest.mark.parametrize("m", [1, 2, 3, 65])
def test_every_proof_has_create_proofs_bytes(keys, m):
    c = keys
    if m == 65:
        # one wavefront of proofs and one more: the SAME witness under seeds 0 .. 64, each proof create_proof's bytes for its seed
        if c["name"] != "poseidon_k6":
            assert c["name"] == "merkle_sum_d5_k9"     # the small circuit alone
            return
        same = c["advice"][:1].expand(m, -1, -1, -1).contiguous()
        proofs = h.create_proofs(c["params"], c["pk"], same, [c["instances"][0]] * m, list(range(m)))
        assert len(proofs) == m == len(set(proofs))
        for b in range(m):
            assert proofs[b] == h.create_proof(c["params"], c["pk"], c["advice"][0], c["instances"][0], b), b
        return
    proofs = h.create_proofs(c["params"], c["pk"], c["advice"][:m], c["instances"][:m], SEEDS[:m])
    assert isinstance(proofs, list) and len(proofs) == m
    for b in range(m):
        assert proofs[b] == c["singles"][b], b
        assert len(proofs[b]) == verifier.proof_length(c["cs"], 1)
    as_list = h.create_proofs(c["params"], c["pk"], [c["advice"][b] for b in range(m)], c["instances"][:m], SEEDS[:m])
    assert as_list == proofs


def test_an_integer_seed_stands_for_consecutive_seeds(keys):
    c = keys
    short = h.create_proofs(c["params"], c["pk"], c["advice"], c["instances"], 40)
    assert short == h.create_proofs(c["params"], c["pk"], c["advice"], c["instances"], [40, 41, 42])
    assert short[1] == h.create_proof(c["params"], c["pk"], c["advice"][1], c["instances"][1], 41)
    assert short[1] != c["singles"][1]


def test_every_proof_verifies_and_the_batch_verifier_accepts(keys):
    c = keys
    proofs = h.create_proofs(c["params"], c["pk"], c["advice"], c["instances"], SEEDS)
    for b in range(3):
        assert h.verify_proof(c["params"], c["vk"], c["instances"][b], proofs[b], trapdoor=pc.SRS_S), b
    assert not h.verify_proof(c["params"], c["vk"], c["instances"][1], proofs[0], trapdoor=pc.SRS_S)    # each user's own proof
    assert h.verify_proofs(c["params"], c["vk"], c["instances"], proofs, seed=5)


def test_a_small_h_budget_gives_the_same_bytes(keys, monkeypatch):
    c = keys
    cs, dom = c["cs"], c["vk"].domain
    own = cs.permutation_sets() + 3 * len(cs.lookups) + cs.num_advice + cs.num_instance
    monkeypatch.setattr(prover, "H_COLUMN_BUDGET", 2 * own * dom.extended_len() * 32)                    # two proofs' columns: chunks of 2 + 1
    assert h.create_proofs(c["params"], c["pk"], c["advice"], c["instances"], SEEDS) == c["singles"]


def test_a_tampered_witness_breaks_its_own_proof_only(keys):
    c = keys
    _, _, _, _, cells = pc.build(c["name"])
    cell = sorted(cells.items())[0][1]
    bad = c["advice"].clone()
    bad[1] = pc.tampered(bad[1], cell)
    assert torch.equal(bad[0], c["advice"][0]) and not torch.equal(bad[1], c["advice"][1])
    proofs = h.create_proofs(c["params"], c["pk"], bad, c["instances"], SEEDS)
    assert not h.verify_proof(c["params"], c["vk"], c["instances"][1], proofs[1], trapdoor=pc.SRS_S)
    assert proofs[0] == c["singles"][0] and proofs[2] == c["singles"][2]
    assert not h.verify_proofs(c["params"], c["vk"], c["instances"], proofs, seed=5)


def test_identical_witnesses_are_blinded_differently(keys):
    c = keys
    twice = torch.stack([c["advice"][0], c["advice"][0]])
    proofs = h.create_proofs(c["params"], c["pk"], twice, [c["instances"][0]] * 2, [SEEDS[0], SEEDS[1]])
    assert proofs[0] == c["singles"][0]
    A = c["cs"].num_advice                     # a proof opens with its advice commitments, 32 bytes each
    for col in range(A):
        assert proofs[0][32 * col:32 * (col + 1)] != proofs[1][32 * col:32 * (col + 1)], col
    assert all(h.verify_proof(c["params"], c["vk"], c["instances"][0], p, trapdoor=pc.SRS_S) for p in proofs)


def test_a_missing_lookup_input_names_its_proof(keys):
    """a diff byte of proof 1 set to 300, which the u8 table lacks: create_proofs raises what create_proof raises for that witness --
    the same error class, code and lookup -- and says which proof it was"""
    c = keys
    if not c["cs"].lookups:
        assert c["name"] == "poseidon_k6"          # no lookups: nothing can be missing
        return
    lookup = 2
    column = c["cs"].lookups[lookup][0][0].column
    bad = c["advice"].clone()
    bad[1][column, 5] = pc.d([300])[0]
    with pytest.raises(_lib.Halo2Mi355xError) as single:
        h.create_proof(c["params"], c["pk"], bad[1], c["instances"][1], SEEDS[1])
    with pytest.raises(_lib.Halo2Mi355xError) as batch:
        h.create_proofs(c["params"], c["pk"], bad, c["instances"], SEEDS)
    assert batch.value.code == single.value.code == _lib.HM_ERR_NOT_FOUND
    assert single.value.missing == [lookup] and batch.value.missing == [lookup] and batch.value.proofs == [1]
    assert "proof 1" in str(batch.value) and "proof 0" not in str(batch.value)
    assert h.create_proofs(c["params"], c["pk"], c["advice"], c["instances"], SEEDS) == c["singles"]      # and the next call is unharmed


def test_wrong_arguments_raise(keys):
    c = keys
    p, pk, adv, inst = c["params"], c["pk"], c["advice"], c["instances"]
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(p, pk, adv, inst, [7, 8, 7])                         # equal seeds
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(p, pk, adv, inst, [7, 8, 7 + (1 << 48)])             # equal mod 2^48
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(p, pk, adv, inst, [7, 8])
    with pytest.raises(ValueError, match="instance"):
        h.create_proofs(p, pk, adv[:2], inst[:3], [1, 2])
    with pytest.raises(ValueError, match="advice"):
        h.create_proofs(p, pk, adv[:2].cpu(), inst[:2], [1, 2])
    with pytest.raises(ValueError, match="advice"):
        h.create_proofs(p, pk, adv[:2, :, :-1], inst[:2], [1, 2])            # a row short
    with pytest.raises(ValueError, match="advice"):
        h.create_proofs(p, pk, adv[0], inst[:1], [1])                        # three dimensions: not a batch
    with pytest.raises(ValueError, match="proof"):
        h.create_proofs(p, pk, [], [], [])
