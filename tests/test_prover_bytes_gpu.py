"""The prover's bytes, pinned to recordings: every case of tests/golden/gen_prover_digests.py recomputed and compared with
tests/golden/prover_digests.json; fresh ``create_proof`` / ``create_proof_multi`` output against the recorded proofs the verifier tests
read (proof_poseidon_k6.bin, proof_merkle_sum_k9.bin, proof_poseidon_k6_x3.bin, the four entries of every gwc_proofs_<system>.npz); and
``create_proof_multi`` with three circuits under an h budget of two circuits' extended columns -- chunks of 2 + 1 chained through
PreviousValue -- against the recorded unchunked digest.  The other prover tests compare one entry point with another; these compare
each with what was written down."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import prover, synthesis as sy
from halo2_experiments_amd.kzg import ParamsKZG

import gwc_cases as gc
import prover_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_prover_digests", os.path.join(HERE, "golden", "gen_prover_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
with open(os.path.join(HERE, "golden", "prover_digests.json")) as f:
    RECORDED = json.load(f)


def recorded_file(name: str) -> bytes:
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def systems():
    """``gen.setup`` of a system, made on first use and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = gen.setup(name)
        return made[name]
    yield get
    for c in made.values():
        c["params"].release()


def test_the_recording_lists_the_cases_and_nothing_else():
    want = set()
    for name in gen.SYSTEMS:
        for mo in gen.MULTIOPENS:
            want |= {f"create_proof/{name}/{enc}/{mo}" for enc in gc.ENCODINGS} | {f"create_proof_multi/{name}/m{m}/{mo}" for m in (2, 3)}
            if name in gen.BATCHED:
                want |= {f"create_proofs/{name}/m3/{enc}/{mo}" for enc in gc.ENCODINGS}
    want |= {"create_proofs/poseidon_k6/m65", "trace/create_proof/merkle_sum_d5_k9", "trace/create_proof_multi/merkle_sum_d5_k9/m2"}
    assert set(RECORDED) == want and len(want) == 35


@pytest.mark.parametrize("name", gen.SYSTEMS)
def test_every_case_has_its_recorded_digest(systems, name):
    got = gen.system_digests(systems(name))
    assert got == {case: RECORDED[case] for case in got}
    assert set(got) == {case for case in RECORDED if case.split("/")[1] == name or case.split("/")[2] == name}


@pytest.mark.parametrize("name,file", [("poseidon_k6", "proof_poseidon_k6.bin"), ("merkle_sum_d5_k9", "proof_merkle_sum_k9.bin")])
def test_create_proof_writes_the_recorded_proof(systems, name, file):
    c = systems(name)
    assert h.create_proof(c["params"], c["pk"], c["advice"], c["instance"], pc.GOLDEN_SEED) == recorded_file(file)


def test_create_proof_multi_writes_the_recorded_proof(systems):
    c = systems("poseidon_k6")
    assert h.create_proof_multi(c["params"], c["pk"], c["users"], c["instances"], pc.GOLDEN_SEED) == recorded_file("proof_poseidon_k6_x3.bin")


@pytest.mark.parametrize("name", gc.SYSTEMS)
def test_create_proof_writes_the_recorded_gwc_and_shplonk_proofs(name):
    rec = gc.recorded(name)
    c = rec["case"]
    advice = torch.from_numpy(sy.columns_to_words(c.advice).view(np.int64)).cuda()
    params = ParamsKZG.setup(c.k, pc.SRS_S)
    try:
        vk = h.keygen_vk(params, c.cs, c.lay)
        pk = h.keygen_pk(params, vk, c.cs, c.lay, cosets=False)
        assert len(rec["proofs"]) == 4
        for (mo, enc), proof in rec["proofs"].items():
            assert h.create_proof(params, pk, advice, c.proof_instance, rec["seed"], encoding=enc, multiopen=mo) == proof, (mo, enc)
    finally:
        params.release()


@pytest.mark.parametrize("name", gen.SYSTEMS)
def test_a_small_h_budget_gives_the_recorded_multi_circuit_bytes(systems, name, monkeypatch):
    c = systems(name)
    cs, dom = c["cs"], c["vk"].domain
    own = cs.permutation_sets() + 3 * len(cs.lookups) + cs.num_advice + cs.num_instance
    monkeypatch.setattr(prover, "H_COLUMN_BUDGET", 2 * own * dom.extended_len() * 32)                    # two circuits' columns: chunks of 2 + 1
    proof = h.create_proof_multi(c["params"], c["pk"], c["users"], c["instances"], gen.MULTI_SEED)
    assert gen.sha(proof) == RECORDED[f"create_proof_multi/{name}/m3/shplonk"]
