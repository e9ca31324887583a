#!/usr/bin/env python3
"""BatchVerifier.finalize() against a loop of verify_proof, on one MI355X.

For MerkleSumTree depth 20 / k = 10 and Poseidon k = 6, batches of B = 1, 16, 64, 256, 1024 proofs (four distinct proofs of each circuit,
tiled): a fresh BatchVerifier per repeat, every proof added, ``finalize()`` through the pairing -- wall-clock, median of five with
min .. max -- and its split as the object itself records it: the read kernel with its download, the plan and the program of the terms
kernel (built per BatchVerifier), the Blake2b transcripts on the host, the upload of the per-proof records, the terms kernel (waited
for), the sums (four MSMs and the column sum) and the one pairing check.  Beside it, in the same session, ``verify_proof`` in a loop
over at most 16 of the same proofs, per proof.  Prints one JSON object; ``--out FILE`` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG                            # noqa: E402
import prover_cases as pc                                                  # noqa: E402

REPEATS = 5
SIZES = (1, 16, 64, 256, 1024)
PHASES = ("read", "plan", "transcript", "upload", "terms", "msm", "pairing")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def circuit(name, sizes, repeats):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    try:
        proofs = [h.create_proof(params, pk, advice, instance, seed) for seed in (2, 3, 4, 5)]
        out = {"k": lay.k, "proof_bytes": len(proofs[0]), "batches": {}}
        single = []
        for i in range(min(16, max(sizes))):
            t0 = time.perf_counter()
            assert h.verify_proof(params, vk, instance, proofs[i % 4])
            single.append((time.perf_counter() - t0) * 1e3)
        out["verify_proof_per_proof"] = dict(spread(single), proofs=len(single))
        h.verify_proofs(params, vk, [instance], proofs[:1])                    # warm-up: library load, allocator pools
        for B in sizes:
            total, split = [], {p: [] for p in PHASES}
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bv = h.BatchVerifier(params, vk)
                for b in range(B):
                    bv.add_proof(instance, proofs[b % 4])
                ok = bv.finalize()
                torch.cuda.synchronize()
                total.append((time.perf_counter() - t0) * 1e3)
                assert ok
                for p in PHASES:
                    split[p].append(bv.timings[p] * 1e3)
            row = {"finalize": spread(total), "per_proof_ms": round(statistics.median(total) / B, 3),
                   "split_median_ms": {p: round(statistics.median(v), 3) for p, v in split.items()}}
            row["against_verify_proof_loop"] = round(out["verify_proof_per_proof"]["median_ms"] * B / statistics.median(total), 2)
            out["batches"][str(B)] = row
    finally:
        params.release()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    torch.cuda.init()
    result = {"tool": "tools/batch_verify_time.py", "repeats": args.repeats,
              "host": "the Blake2b transcripts and the pairing; everything else (read, terms, column sum, MSMs) on the device",
              "merkle_sum_d20_k10": circuit("merkle_sum_d20_k10", sizes, args.repeats), "poseidon_k6": circuit("poseidon_k6", sizes, args.repeats)}
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
