"""Records tests/golden/prover_digests.json for tests/test_prover_bytes_gpu.py: one SHA-256 per prover case, so that the bytes of
``create_proof``, ``create_proof_multi`` and ``create_proofs`` are pinned to a recording and not only to one another.
``python tests/golden/gen_prover_digests.py [out_dir]`` on a machine with the GPU.  The SRS trapdoor, the witnesses and the seeds are
fixed (tests/prover_cases.py, tests/prover_multi_cases.py, tests/gwc_cases.py), so a rerun writes the same file.

The cases, per system (``system_digests``):
    create_proof/<system>/<encoding>/<multiopen>            the witness of prover_cases.build, seed GOLDEN_SEED
    create_proof_multi/<system>/m<2|3>/<multiopen>          the first m users of prover_multi_cases.build_multi(system, 3), seed 7
    create_proofs/<system>/m3/<encoding>/<multiopen>        the same three users, seeds 7, 2^20, 99; the proofs concatenated
    create_proofs/poseidon_k6/m65                           user 0 under seeds 0 .. 64 (one wavefront of proofs and one more), concatenated
    trace/create_proof/merkle_sum_d5_k9, trace/create_proof_multi/merkle_sum_d5_k9/m2
                                                            the sorted ``commits`` items and the ``challenges`` of ``_trace``"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import halo2_experiments_amd as h                    # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG      # noqa: E402
import gwc_cases as gc                               # noqa: E402
import prover_cases as pc                            # noqa: E402
import prover_multi_cases as pmc                     # noqa: E402

SYSTEMS = ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"]
BATCHED = ["poseidon_k6", "merkle_sum_d5_k9"]       # the systems create_proofs is recorded on
TRACED = "merkle_sum_d5_k9"
MULTIOPENS = ("shplonk", "gwc")
MULTI_SEED = 7
SEEDS = [7, 1 << 20, 99]
WAVE = 65
assert gc.GOLDEN_SEED == pc.GOLDEN_SEED


def sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def trace_digest(trace: dict) -> str:
    """over the commitments (affine integer pairs) in the order of their sorted keys, then the challenges by name"""
    return sha(repr((sorted(trace["commits"].items()), sorted(trace["challenges"].items()))).encode())


def setup(name: str) -> dict:
    """the keys and witnesses of one system: prover_cases' single witness and prover_multi_cases' three users.  The caller releases
    ``params``."""
    cs, lay, advice, instance, _ = pc.build(name)
    _, _, users, instances = pmc.build_multi(name, 3)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    return dict(name=name, cs=cs, params=params, vk=vk, pk=pk, advice=advice, instance=instance, users=users, instances=instances)


def system_digests(c: dict) -> dict:
    """{case: SHA-256} of one system, from what ``setup`` returned"""
    name, params, pk = c["name"], c["params"], c["pk"]
    out = {}
    for mo in MULTIOPENS:
        for enc in gc.ENCODINGS:
            out[f"create_proof/{name}/{enc}/{mo}"] = sha(h.create_proof(params, pk, c["advice"], c["instance"], pc.GOLDEN_SEED, encoding=enc,
                                                                        multiopen=mo))
        for m in (2, 3):
            out[f"create_proof_multi/{name}/m{m}/{mo}"] = sha(h.create_proof_multi(params, pk, c["users"][:m], c["instances"][:m], MULTI_SEED,
                                                                                   multiopen=mo))
        if name in BATCHED:
            for enc in gc.ENCODINGS:
                out[f"create_proofs/{name}/m3/{enc}/{mo}"] = sha(b"".join(h.create_proofs(params, pk, c["users"], c["instances"], SEEDS, encoding=enc,
                                                                                          multiopen=mo)))
    if name == "poseidon_k6":
        same = c["users"][:1].expand(WAVE, -1, -1, -1).contiguous()
        out[f"create_proofs/{name}/m{WAVE}"] = sha(b"".join(h.create_proofs(params, pk, same, [c["instances"][0]] * WAVE, list(range(WAVE)))))
    if name == TRACED:
        trace = {}
        h.create_proof(params, pk, c["advice"], c["instance"], pc.GOLDEN_SEED, _trace=trace)
        out[f"trace/create_proof/{name}"] = trace_digest(trace)
        trace = {}
        h.create_proof_multi(params, pk, c["users"][:2], c["instances"][:2], MULTI_SEED, _trace=trace)
        out[f"trace/create_proof_multi/{name}/m2"] = trace_digest(trace)
    return out


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    digests = {}
    for name in SYSTEMS:
        c = setup(name)
        try:
            digests.update(system_digests(c))
        finally:
            c["params"].release()
        print(f"{name}: {len(digests)} digests so far")
    with open(os.path.join(out_dir, "prover_digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
