#!/usr/bin/env python3
"""BatchVerifier.finalize() against a loop of verify_proof, on one MI355X.

For MerkleSumTree depth 20 / k = 10 and Poseidon k = 6, batches of B = 1, 16, 64, 256, 1024 proofs (four distinct proofs of each circuit,
tiled): a fresh BatchVerifier per repeat, every proof added, ``finalize()`` through the pairing -- wall-clock, median of five with
min .. max -- and its split as the object itself records it: the read kernel with its download, the plan and the program of the terms
kernel (built per BatchVerifier), the Blake2b transcripts on the host, the upload of the per-proof records, the terms kernel (waited
for), the sums (four MSMs and the column sum) and the one pairing check.  Beside it, in the same session, ``verify_proof`` in a loop
over at most 16 of the same proofs, per proof.  Prints one JSON object; ``--out FILE`` also writes it.

``--transcript host|device|both`` and ``--pairing host|device|both`` choose where the transcripts and the pairing run (both default to
host: the figures above).  With more than one combination every one is measured in the SAME session, under ``modes`` by
"transcript/pairing"; in device mode ``read``, ``transcript`` and ``terms`` of the split are the times of queueing each call and only
their sum means anything.  With a device transcript the record also holds ``transcript_kernel_ms``: ``hm_verify_transcript_dev``
alone, on a prepared batch, timed with events around the call."""
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


def transcript_kernel_ms(bv, repeats):
    """hm_verify_transcript_dev alone on the arrays a prepared device-mode batch keeps: events around the call, one warm-up"""
    from halo2_experiments_amd import device_transcript as dt

    st = bv._prepare()
    d_bad = torch.zeros(st["B"], dtype=torch.int32, device=st["d_proofs"].device)
    d_records = st["d_records"].clone()
    ms = []
    for i in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        dt.challenges(bv.layout, bv._digest, None, st["d_proofs"], st["d_ybytes"], d_bad, d_records, preamble=st["preamble"], d_table=st["d_table"])
        end.record()
        end.synchronize()
        if i:
            ms.append(start.elapsed_time(end))
    assert torch.equal(d_records, st["d_records"]) and not d_bad.any()
    return spread(ms)


def circuit(name, sizes, repeats, modes=(("host", "host"),)):
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
        for transcript, pairing in modes:
            h.verify_proofs(params, vk, [instance], proofs[:1], transcript=transcript, pairing=pairing)   # warm-up: library load, allocator pools
        for B in sizes:
            for transcript, pairing in modes:
                total, split = [], {p: [] for p in PHASES}
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    bv = h.BatchVerifier(params, vk, transcript=transcript, pairing=pairing)
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
                if transcript == "device":
                    row["transcript_kernel_ms"] = transcript_kernel_ms(bv, repeats)
                if len(modes) == 1:
                    out["batches"][str(B)] = row
                else:
                    out.setdefault("modes", {}).setdefault(f"{transcript}/{pairing}", {})[str(B)] = row
                bv.close()
        if len(modes) > 1:
            del out["batches"]
    finally:
        params.release()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--transcript", choices=("host", "device", "both"), default="host")
    ap.add_argument("--pairing", choices=("host", "device", "both"), default="host")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    both = lambda choice: ("host", "device") if choice == "both" else (choice,)
    modes = tuple((t, p) for p in both(args.pairing) for t in both(args.transcript))
    torch.cuda.init()
    result = {"tool": "tools/batch_verify_time.py", "repeats": args.repeats, "modes_measured": [f"{t}/{p}" for t, p in modes],
              "host": "the Blake2b transcripts and the pairing, unless the mode (transcript/pairing) says device; everything else (read, "
                      "terms, column sum, MSMs) on the device",
              "merkle_sum_d20_k10": circuit("merkle_sum_d20_k10", sizes, args.repeats, modes),
              "poseidon_k6": circuit("poseidon_k6", sizes, args.repeats, modes)}
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
