"""create_proof_multi / verify_proof_multi: several circuits of one constraint system in ONE proof, on witnesses
of different users built by the batch witness writers.  With one circuit the bytes are create_proof's; with two and three the proof
has the counted length, verifies through the pairing and through the trapdoor, every commitment is [f(s)]G of the polynomial it
commits (Horner on the coefficients), a seed fixes the bytes and another seed gives other bytes that verify; two identical witnesses
in one proof get different blinding; a changed cell of one circuit, swapped instances, and the one-circuit verifier are refused."""
import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import pairing as pr, poseidon as ps, verifier
from halo2_experiments_amd.domain import fr_words
from halo2_experiments_amd.kzg import ParamsKZG

import prover_cases as pc
import prover_multi_cases as pmc

pytestmark = pytest.mark.gpu

MULTI = ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"]
SEED = 7


@pytest.fixture(scope="module", params=MULTI)
def keys(request):
    name = request.param
    cs, lay, advice, instances = pmc.build_multi(name, 3)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    yield dict(name=name, cs=cs, lay=lay, params=params, vk=vk, pk=pk, advice=advice, instances=instances)
    params.release()


@pytest.fixture(scope="module", params=[2, 3])
def proven(request, keys):
    m = request.param
    trace = {}
    advice, instances = keys["advice"][:m], keys["instances"][:m]
    proof = h.create_proof_multi(keys["params"], keys["pk"], advice, instances, SEED, _trace=trace)
    return dict(keys, m=m, advice=advice, instances=instances, proof=proof, trace=trace)


def both(c, instances, proof):
    a = h.verify_proof_multi(c["params"], c["vk"], instances, proof)
    b = h.verify_proof_multi(c["params"], c["vk"], instances, proof, trapdoor=pc.SRS_S)
    assert a == b, "the pairing and the trapdoor disagree"
    return a


@pytest.mark.parametrize("name", ["poseidon_k6", "merkle_sum_d5_k9"])
def test_one_circuit_gives_create_proofs_bytes(name):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    try:
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        single = h.create_proof(params, pk, advice, instance, SEED)
        assert h.create_proof_multi(params, pk, [advice], [instance], SEED) == single
        assert h.create_proof_multi(params, pk, advice.reshape(1, *advice.shape), [instance], SEED) == single
        assert h.verify_proof_multi(params, vk, [instance], single, trapdoor=pc.SRS_S) and h.verify_proof(params, vk, instance, single, trapdoor=pc.SRS_S)
    finally:
        params.release()


def test_prove_then_verify(proven):
    c = proven
    assert len(c["proof"]) == verifier.proof_length(c["cs"], c["m"])
    assert both(c, c["instances"], c["proof"])
    assert not h.verify_proof(c["params"], c["vk"], c["instances"][0], c["proof"], trapdoor=pc.SRS_S)
    assert not h.verify_proof(c["params"], c["vk"], c["instances"][0], c["proof"])


def test_commitments_are_evaluations_at_the_trapdoor(proven):
    c = proven
    polys, commits = c["trace"]["polys"], c["trace"]["commits"]
    keys_ = [key for key in commits if key in polys]
    assert len(keys_) == len(commits) - (c["cs"].degree() - 1) and ("random",) in keys_            # all but the h pieces, checked below
    assert sum(1 for key in keys_ if key[0] == "advice") == c["m"] * c["cs"].num_advice
    pieces = c["trace"]["pieces"]
    stack = torch.stack([polys[key] for key in keys_] + list(pieces))
    fs = ps.words_to_ints(h.eval_polynomial(stack, np.stack([fr_words(pc.SRS_S)] * stack.shape[0])))
    for key, f in zip(keys_ + [("h_piece", i) for i in range(len(pieces))], fs):
        assert commits[key] == pr.g1_mul(f), key


def test_seeds(proven):
    c = proven
    assert h.create_proof_multi(c["params"], c["pk"], c["advice"], c["instances"], SEED) == c["proof"]
    as_list = [c["advice"][i] for i in range(c["m"])]
    assert h.create_proof_multi(c["params"], c["pk"], as_list, c["instances"], SEED) == c["proof"]
    other = h.create_proof_multi(c["params"], c["pk"], c["advice"], c["instances"], SEED + 1)
    assert other != c["proof"] and len(other) == len(c["proof"])
    assert h.verify_proof_multi(c["params"], c["vk"], c["instances"], other, trapdoor=pc.SRS_S)


def test_identical_witnesses_are_blinded_differently(keys):
    c = keys
    twice = torch.stack([c["advice"][0], c["advice"][0]])
    trace = {}
    proof = h.create_proof_multi(c["params"], c["pk"], twice, [c["instances"][0]] * 2, SEED, _trace=trace)
    assert both(c, [c["instances"][0]] * 2, proof)
    commits = trace["commits"]
    for col in range(c["cs"].num_advice):
        assert commits[("advice", col, 0)] != commits[("advice", col, 1)], col
    nsets = c["cs"].permutation_sets()
    assert all(commits[("perm_z", i, 0)] != commits[("perm_z", i, 1)] for i in range(nsets))


def broken_cell(c):
    """(column, row) of an advice cell whose change breaks circuit 1: the cells tests/prover_cases.py names where it names some, else the
    first cell of row 1 that the single-circuit prover and verifier notice"""
    _, lay, _, _, cells = pc.build(c["name"])
    if cells:
        return sorted(cells.items())[0][1]
    for col in range(c["cs"].num_advice):
        single = h.create_proof(c["params"], c["pk"], pc.tampered(c["advice"][1], (col, 1)), c["instances"][1], SEED)
        if not h.verify_proof(c["params"], c["vk"], c["instances"][1], single, trapdoor=pc.SRS_S):
            return col, 1
    pytest.fail("no cell of row 1 breaks the single-circuit proof")


def test_a_changed_cell_in_one_circuit(proven):
    c = proven
    bad = c["advice"].clone()
    bad[1] = pc.tampered(bad[1], broken_cell(c))
    assert torch.equal(bad[0], c["advice"][0]) and not torch.equal(bad[1], c["advice"][1])
    proof = h.create_proof_multi(c["params"], c["pk"], bad, c["instances"], SEED)
    assert len(proof) == len(c["proof"]) and not both(c, c["instances"], proof)


def test_swapped_instances(proven):
    c = proven
    swapped = [c["instances"][1], c["instances"][0]] + c["instances"][2:]
    assert swapped != c["instances"]
    assert not both(c, swapped, c["proof"])
    lying = h.create_proof_multi(c["params"], c["pk"], c["advice"], swapped, SEED)
    assert not both(c, swapped, lying)


def test_wrong_arguments_raise(keys):
    c = keys
    p, pk, adv, inst = c["params"], c["pk"], c["advice"], c["instances"]
    with pytest.raises(ValueError, match="instance"):
        h.create_proof_multi(p, pk, adv[:2], inst[:3], SEED)
    with pytest.raises(ValueError, match="instance"):
        h.create_proof_multi(p, pk, adv[:2], inst[:1], SEED)
    with pytest.raises(ValueError, match="64"):
        h.create_proof_multi(p, pk, adv[:1].expand(65, *adv.shape[1:]), [inst[0]] * 65, SEED)
    with pytest.raises(ValueError, match="64"):
        h.create_proof_multi(p, pk, [], [], SEED)
    with pytest.raises(ValueError, match="advice"):
        h.create_proof_multi(p, pk, adv[0], inst[:1], SEED)                      # three dimensions: not a batch
    with pytest.raises(ValueError, match="advice"):
        h.create_proof_multi(p, pk, adv[:2, :, :-1], inst[:2], SEED)             # a row short
    with pytest.raises(ValueError, match="advice"):
        h.create_proof_multi(p, pk, [adv[0], adv[1][:-1]], inst[:2], SEED)       # a column short
    with pytest.raises(ValueError, match="advice"):
        h.create_proof_multi(p, pk, adv[:2].cpu(), inst[:2], SEED)
