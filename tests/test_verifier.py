"""verify_proof without a GPU, on proofs recorded by tests/golden/gen_golden_proofs.py (fixed seed, fixed SRS trapdoor): each golden proof
verifies through the pairing and through the trapdoor; a flipped byte in the first commitment, in an evaluation or in the last point,
a changed instance value and a truncated proof are refused by both; the proof length is the one counted from the constraint system."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import poseidon as ps, verifier
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.kzg import G2_GENERATOR, g2_bytes, g2_mul

import prover_cases as pc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def params():
    return SimpleNamespace(g2=g2_bytes(G2_GENERATOR), s_g2=g2_bytes(g2_mul(pc.SRS_S)))


@pytest.fixture(scope="module", params=[("poseidon_k6", "poseidon_k6"), ("merkle_sum_d5_k9", "merkle_sum_k9")], ids=lambda p: p[1])
def golden_proof(request):
    name, short = request.param
    cs, k = pc.constraint_system(name)
    meta = np.load(os.path.join(GOLDEN, f"proof_{short}.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, f"proof_{short}.bin"), "rb").read()
    return cs, vk, ps.words_to_ints(meta["instance"]), proof


def both(params, vk, instance, proof):
    a = h.verify_proof(params, vk, instance, proof)
    assert a == h.verify_proof(params, vk, instance, proof, trapdoor=pc.SRS_S), "the pairing and the trapdoor disagree"
    return a


def test_golden_proof_verifies(params, golden_proof):
    cs, vk, instance, proof = golden_proof
    assert len(proof) == verifier.proof_length(cs)
    assert both(params, vk, instance, proof)


def flipped(proof, at):
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


@pytest.mark.parametrize("what", ["first commitment", "an evaluation", "last point", "instance", "truncated", "one byte more"])
def test_refusals(params, golden_proof, what):
    cs, vk, instance, proof = golden_proof
    points_before_evals = cs.num_advice + 3 * len(cs.lookups) + cs.permutation_sets() + 1 + cs.degree() - 1
    if what == "first commitment":
        # x + 1 is either no x of the curve (a malformed proof) or another point (a failed check): False either way, never an exception
        assert not both(params, vk, instance, flipped(proof, 0))
    elif what == "an evaluation":
        assert not both(params, vk, instance, flipped(proof, 32 * points_before_evals + 32 * 3 + 1))
    elif what == "last point":
        assert not both(params, vk, instance, flipped(proof, len(proof) - 32))
    elif what == "instance":
        assert not both(params, vk, [(instance[0] + 1) % R] + instance[1:], proof)
    elif what == "truncated":
        assert not both(params, vk, instance, proof[:-32]) and not both(params, vk, instance, proof[:5]) and not both(params, vk, instance, b"")
    else:
        assert not both(params, vk, instance, proof + b"\0")
    scalar_ge_r = bytearray(proof)
    scalar_ge_r[32 * points_before_evals:32 * points_before_evals + 32] = R.to_bytes(32, "little")
    assert not h.verify_proof(params, vk, instance, bytes(scalar_ge_r), trapdoor=pc.SRS_S)
