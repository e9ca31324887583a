"""Records tests/golden/proof_<case>.bin and proof_<case>.npz (the instance values and the verifying key's commitments) for
tests/test_verifier.py: ``python tests/golden/gen_golden_proofs.py [out_dir]`` on a machine with the GPU.  The SRS trapdoor and the seed are
fixed (tests/prover_cases.py), so a rerun writes the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import halo2_experiments_amd as h                    # noqa: E402
from halo2_experiments_amd import poseidon as ps     # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG      # noqa: E402
import prover_cases as pc                            # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for name, short in (("poseidon_k6", "poseidon_k6"), ("merkle_sum_d5_k9", "merkle_sum_k9")):
        cs, lay, advice, instance, _ = pc.build(name)
        params = ParamsKZG.setup(lay.k, pc.SRS_S)
        try:
            vk = h.keygen_vk(params, cs, lay)
            pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
            proof = h.create_proof(params, pk, advice, instance, pc.GOLDEN_SEED)
            assert h.verify_proof(params, vk, instance, proof) and h.verify_proof(params, vk, instance, proof, trapdoor=pc.SRS_S)
        finally:
            params.release()
        with open(os.path.join(out_dir, f"proof_{short}.bin"), "wb") as f:
            f.write(proof)
        np.savez(os.path.join(out_dir, f"proof_{short}.npz"), instance=ps.ints_to_words(instance), fixed_commitments=vk.fixed_commitments,
                 permutation_commitments=vk.permutation_commitments)
        print(f"{name}: {len(proof)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
