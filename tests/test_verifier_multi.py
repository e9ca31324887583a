"""verify_proof_multi without a GPU, on the three-circuit Poseidon proof recorded by tests/golden/gen_golden_proofs_multi.py (fixed seed,
fixed SRS trapdoor): it verifies through the pairing and through the trapdoor; a flipped byte in each section of the proof, a truncated
proof, a proof with one byte more, a changed or swapped instance are refused by both; verify_proof (one circuit) refuses it."""
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

M = 3


@pytest.fixture(scope="module")
def params():
    return SimpleNamespace(g2=g2_bytes(G2_GENERATOR), s_g2=g2_bytes(g2_mul(pc.SRS_S)))


@pytest.fixture(scope="module")
def golden():
    cs, k = pc.constraint_system("poseidon_k6")
    meta = np.load(os.path.join(GOLDEN, "proof_poseidon_k6_x3.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, "proof_poseidon_k6_x3.bin"), "rb").read()
    return cs, vk, [ps.words_to_ints(i) for i in meta["instances"]], proof


def both(params, vk, instances, proof):
    a = h.verify_proof_multi(params, vk, instances, proof)
    assert a == h.verify_proof_multi(params, vk, instances, proof, trapdoor=pc.SRS_S), "the pairing and the trapdoor disagree"
    return a


def sections(cs, m):
    """name -> the offset of the first byte of each section of the proof, in the transcript's order"""
    adv_q, fix_q, _ = cs.queries()
    P, nsets, L = len(cs.equality), cs.permutation_sets(), len(cs.lookups)
    sizes = [("advice commitments", m * cs.num_advice), ("permuted lookup columns", 2 * m * L), ("permutation z", m * nsets), ("lookup z", m * L),
             ("random polynomial", 1), ("h pieces", cs.degree() - 1), ("advice evaluations", m * len(adv_q)), ("fixed evaluations", len(fix_q)),
             ("random evaluation", 1), ("sigma evaluations", P), ("permutation z evaluations", m * (3 * nsets - 1 if nsets else 0)),
             ("lookup evaluations", 5 * m * L), ("opening", 2)]
    out, at = {}, 0
    for name, count in sizes:
        if count:
            out[name] = at
        at += 32 * count
    assert at == verifier.proof_length(cs, m)
    return out


def test_the_recorded_proof_verifies(params, golden):
    cs, vk, instances, proof = golden
    assert len(instances) == M and len(proof) == verifier.proof_length(cs, M) > verifier.proof_length(cs)
    assert len({tuple(i) for i in instances}) == M                      # three different users
    assert both(params, vk, instances, proof)


def flipped(proof, at):
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


def test_a_flipped_byte_in_each_section_is_refused(params, golden):
    cs, vk, instances, proof = golden
    where = sections(cs, M)
    assert {"advice commitments", "permutation z", "random polynomial", "h pieces", "advice evaluations", "fixed evaluations", "random evaluation",
            "sigma evaluations", "permutation z evaluations", "opening"} <= set(where)
    for name, at in where.items():
        # the trapdoor route: a pairing per section would take a minute on the host; the two routes agree wherever both run
        assert not h.verify_proof_multi(params, vk, instances, flipped(proof, at + 1), trapdoor=pc.SRS_S), name
    # the LAST circuit's share of a per-circuit section, and the last point
    assert not h.verify_proof_multi(params, vk, instances, flipped(proof, where["advice commitments"] + 32 * (M * cs.num_advice - 1)), trapdoor=pc.SRS_S)
    assert not both(params, vk, instances, flipped(proof, len(proof) - 32))
    assert not both(params, vk, instances, flipped(proof, where["advice evaluations"] + 32 * 3 + 1))


def test_truncated_and_extended_proofs_are_refused(params, golden):
    cs, vk, instances, proof = golden
    assert not both(params, vk, instances, proof[:-32]) and not both(params, vk, instances, proof[:5]) and not both(params, vk, instances, b"")
    assert not both(params, vk, instances, proof + b"\0")
    scalar_ge_r = bytearray(proof)
    at = sections(cs, M)["advice evaluations"]
    scalar_ge_r[at:at + 32] = R.to_bytes(32, "little")
    assert not h.verify_proof_multi(params, vk, instances, bytes(scalar_ge_r), trapdoor=pc.SRS_S)


def test_wrong_instances_are_refused(params, golden):
    cs, vk, instances, proof = golden
    changed = [list(i) for i in instances]
    changed[1][0] = (changed[1][0] + 1) % R
    assert not both(params, vk, changed, proof)
    assert not h.verify_proof_multi(params, vk, [instances[1], instances[0], instances[2]], proof, trapdoor=pc.SRS_S)      # two users swapped
    assert not h.verify_proof_multi(params, vk, instances[:2], proof, trapdoor=pc.SRS_S)                                   # a circuit fewer
    assert not h.verify_proof_multi(params, vk, [], proof, trapdoor=pc.SRS_S)
    assert not h.verify_proof(params, vk, instances[0], proof, trapdoor=pc.SRS_S)                                          # not a one-circuit proof


def test_proof_length_counts_per_circuit_sections_once_per_circuit():
    for name in ("poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"):
        cs, _ = pc.constraint_system(name)
        one, two, five = (verifier.proof_length(cs, m) for m in (1, 2, 5))
        assert one == verifier.proof_length(cs) and (five - one) == 4 * (two - one) and two > one
