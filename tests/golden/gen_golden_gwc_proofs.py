"""Records tests/golden/gwc_proofs_<system>.npz for tests/test_gwc_host.py: per system (tests/gwc_cases.py) one GWC proof per encoding,
the SHPLONK proofs of the same witness and seed, the instance values, the seed and the verifying key's commitments.
``python tests/golden/gen_golden_gwc_proofs.py [out_dir]`` on a machine with the GPU.  The SRS trapdoor and the seed are fixed, so a
rerun writes the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import torch                                         # noqa: E402
import halo2_experiments_amd as h                    # noqa: E402
from halo2_experiments_amd import poseidon as ps, synthesis as sy     # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG      # noqa: E402
import gwc_cases as gc                               # noqa: E402
import mutation_cases as mc                          # noqa: E402
from prover_cases import SRS_S                       # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for name in gc.SYSTEMS:
        c = mc.case(name)
        advice = torch.from_numpy(sy.columns_to_words(c.advice).view(np.int64)).cuda()
        params = ParamsKZG.setup(c.k, SRS_S)
        try:
            vk = h.keygen_vk(params, c.cs, c.lay)
            pk = h.keygen_pk(params, vk, c.cs, c.lay, cosets=False)
            proofs = {}
            for mo in ("gwc", "shplonk"):
                for enc in gc.ENCODINGS:
                    proof = h.create_proof(params, pk, advice, c.proof_instance, gc.GOLDEN_SEED, encoding=enc, multiopen=mo)
                    assert h.verify_proof(params, vk, c.proof_instance, proof, trapdoor=SRS_S, encoding=enc, multiopen=mo)
                    assert h.verify_proof(params, vk, c.proof_instance, proof, encoding=enc, multiopen=mo)
                    proofs[f"{mo}_{enc}"] = np.frombuffer(proof, dtype=np.uint8)
        finally:
            params.release()
        flat = [] if c.proof_instance == [[]] else list(c.proof_instance)
        np.savez(os.path.join(out_dir, f"gwc_proofs_{name}.npz"), instance=ps.ints_to_words(flat).reshape(-1, 4), seed=np.int64(gc.GOLDEN_SEED),
                 fixed_commitments=vk.fixed_commitments, permutation_commitments=vk.permutation_commitments, **proofs)
        print(f"{name}: " + ", ".join(f"{key} {len(p)} bytes" for key, p in proofs.items()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
