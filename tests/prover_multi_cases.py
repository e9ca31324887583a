"""Several users' witnesses of one circuit, built by the batch witness writers, for the multi-circuit prover tests
(tests/test_prover_multi_gpu.py, tests/golden/gen_golden_proofs_multi.py).  The single-circuit cases: tests/prover_cases.py."""
import random

from halo2_experiments_amd import poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R

import prover_cases as pc


def build_multi(name, m, seed=0):
    """-> (cs, layout, advice (m, num_advice, n, 4) GPU tensor, [instance integers of user c]): m different users"""
    import torch
    rng = random.Random(len(name) * 104729 + 31 * m + seed)
    cs, k = pc.constraint_system(name)
    if name == "poseidon_k6":
        spec = ps.default_spec(5)
        lay = sy.PoseidonCircuitLayout(k, spec)
        adv, inst = sy.poseidon_circuit_witness(spec, pc.d([rng.randrange(R) for _ in range(4 * m)]).reshape(m, 4, 4), k)
    elif name == "merkle_v3_d5_k8":
        spec, depth = ps.default_spec(3), 5
        lay = sy.MerkleTreeV3Layout(depth, k, spec)
        idx = torch.tensor([rng.randrange(1 << depth) for _ in range(m)], dtype=torch.int64, device="cuda")
        adv, inst = sy.merkle_witness(spec, pc.d([rng.randrange(R) for _ in range(m)]).reshape(m, 4),
                                      pc.d([rng.randrange(R) for _ in range(m * depth)]).reshape(m, depth, 4), idx, k)
    else:
        spec, depth = ps.default_spec(5), {"merkle_sum_d5_k9": 5, "merkle_sum_d20_k10": 20}[name]
        lay = sy.MerkleSumTreeLayout(depth, k, spec)
        pair = lambda: [rng.randrange(R), rng.randrange(1 << 40)]
        idx = torch.tensor([rng.randrange(1 << depth) for _ in range(m)], dtype=torch.int64, device="cuda")
        adv, inst = sy.merkle_sum_witness(spec, pc.d([v for _ in range(m) for v in pair()]).reshape(m, 2, 4),
                                          pc.d([v for _ in range(m * depth) for v in pair()]).reshape(m, depth, 2, 4), idx, 1 << 50, k)
    lay.check_constraint_system(cs)
    return cs, lay, adv.contiguous(), [pc.ints(inst[c]) for c in range(m)]
