"""Records tests/golden/proof_poseidon_k6_x3.bin and .npz (the three users' instance values and the verifying key's commitments) for
tests/test_verifier_multi.py: ``python tests/golden/gen_golden_proofs_multi.py [out_dir]`` on a machine with the GPU.  The SRS trapdoor
and the seed are fixed (tests/prover_cases.py), so a rerun writes the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import halo2_experiments_amd as h                    # noqa: E402
from halo2_experiments_amd import poseidon as ps     # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG      # noqa: E402
import prover_cases as pc                            # noqa: E402
import prover_multi_cases as pmc                     # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cs, lay, advice, instances = pmc.build_multi("poseidon_k6", 3)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    try:
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        proof = h.create_proof_multi(params, pk, advice, instances, pc.GOLDEN_SEED)
        assert h.verify_proof_multi(params, vk, instances, proof) and h.verify_proof_multi(params, vk, instances, proof, trapdoor=pc.SRS_S)
    finally:
        params.release()
    with open(os.path.join(out_dir, "proof_poseidon_k6_x3.bin"), "wb") as f:
        f.write(proof)
    np.savez(os.path.join(out_dir, "proof_poseidon_k6_x3.npz"), instances=np.stack([ps.ints_to_words(i) for i in instances]),
             fixed_commitments=vk.fixed_commitments, permutation_commitments=vk.permutation_commitments)
    print(f"poseidon_k6 x 3: {len(proof)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
