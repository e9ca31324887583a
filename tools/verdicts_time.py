#!/usr/bin/env python3
"""BatchVerifier.verdicts() against finalize(), and failing(method="each") against the bisection, on one MI355X.

For MerkleSumTree depth 20 / k = 10 and Poseidon k = 6, batches of B = 1, 16, 64, 256, 1024 proofs (four distinct proofs of each circuit,
tiled), ``pairing="device"``, ``transcript="device"``, everything in ONE session and the compared routes alternating per B, median
of five with min .. max:

  sums_kernel_ms / msm_sums_ms   ``hm_verify_proof_sums_dev`` alone on a prepared batch, events around the call; beside it the four-MSM
                                 ``_sums`` of the whole batch (wall-clock: it folds on the host), the step ``finalize`` takes instead
  verdicts / finalize            wall-clock of each on the SAME prepared batch, a fresh BatchVerifier per repeat, the preparation
                                 (``prepare``) timed apart: the yardstick is the ``finalize`` beside it
  failing                        at the largest B with f = 0, 1, 8 tampered proofs at seeded positions: ``failing(method="each")``
                                 against ``failing()``, each on a fresh prepared batch, with the bisection's MSM count

Prints one JSON object; ``--out FILE`` also writes it."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd import _lib                                     # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG                            # noqa: E402
import prover_cases as pc                                                  # noqa: E402

REPEATS = 5
SIZES = (1, 16, 64, 256, 1024)
TAMPERED = (0, 1, 8)
MODES = dict(pairing="device", transcript="device")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def prepared(params, vk, members):
    bv = h.BatchVerifier(params, vk, **MODES)
    for inst, proof in members:
        bv.add_proof(inst, proof)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bv._prepare()
    torch.cuda.synchronize()
    return bv, (time.perf_counter() - t0) * 1e3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def sums_kernel_ms(bv, repeats):
    """the sums kernel alone on the arrays a prepared batch keeps: events around the call, one warm-up, an output array of its own"""
    st, lay = bv._prepare(), bv.layout
    dev = st["d_bases"].device
    d_pairs = torch.zeros((st["B"], 2, 8), dtype=torch.int64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ms = []
    for i in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _lib.check(_lib.load().hm_verify_proof_sums_dev(vp(st["d_bases"]), st["B"], lay.own_points, len(lay.shared_keys), vp(st["d_own"]),
                                                        vp(st["d_shared"]), vp(st["d_h2_r"]), vp(st["d_h2_l"]),
                                                        ctypes.cast(vp(st["d_bad"]), ctypes.POINTER(ctypes.c_uint32)), vp(d_pairs), stream))
        end.record()
        end.synchronize()
        if i:
            ms.append(start.elapsed_time(end))
    assert torch.equal(d_pairs, bv.proof_sums())
    return spread(ms)


def tamper(member):
    inst, proof = member
    return list(inst[:-1]) + [(inst[-1] + 1) % pc.R], proof


def circuit(name, sizes, repeats):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    try:
        made = [(instance, h.create_proof(params, pk, advice, instance, seed)) for seed in (2, 3, 4, 5)]
        out = {"k": lay.k, "terms_per_proof": None, "batches": {}, "failing": {}}
        warm, _ = prepared(params, vk, made[:1])                 # warm-up: library load, allocator pools, both routes once
        assert warm.verdicts() == [True] and warm.finalize()
        out["terms_per_proof"] = warm.layout.own_points + len(warm.layout.shared_keys) + 1
        warm.close()
        for B in sizes:
            members = [made[b % 4] for b in range(B)]
            prep, verdicts, finalize, msm_sums = [], [], [], []
            for r in range(repeats):
                bv, ms = prepared(params, vk, members)
                prep.append(ms)
                order = ("verdicts", "finalize") if r % 2 == 0 else ("finalize", "verdicts")    # the routes alternate
                for which in order:
                    if which == "verdicts":
                        got, ms = wall(bv.verdicts)
                        assert got == [True] * B
                        verdicts.append(ms)
                    else:
                        ok, ms = wall(bv.finalize)
                        assert ok
                        finalize.append(ms)
                        msm_sums.append(bv.timings["msm"] * 1e3)
                if r + 1 < repeats:
                    bv.close()
            row = {"prepare": spread(prep), "verdicts": spread(verdicts), "finalize": spread(finalize), "msm_sums_ms": spread(msm_sums),
                   "sums_kernel_ms": sums_kernel_ms(bv, repeats)}
            row["verdicts_over_finalize"] = round(row["verdicts"]["median_ms"] / row["finalize"]["median_ms"], 2)
            bv.close()
            out["batches"][str(B)] = row
            print(f"{name} B={B}: verdicts {row['verdicts']['median_ms']} ms, finalize {row['finalize']['median_ms']} ms, "
                  f"sums kernel {row['sums_kernel_ms']['median_ms']} ms", file=sys.stderr, flush=True)
        B = max(sizes)
        for f in TAMPERED:
            where = sorted(random.Random(f"verdicts {B} {f}").sample(range(B), min(f, B)))
            members = [made[b % 4] for b in range(B)]
            for b in where:
                members[b] = tamper(members[b])
            each, bisect, msms = [], [], []
            for r in range(repeats):
                for which in (("each", "bisect") if r % 2 == 0 else ("bisect", "each")):
                    bv, _ = prepared(params, vk, members)
                    got, ms = wall(lambda: bv.failing(method=which))
                    assert got == where
                    (each if which == "each" else bisect).append(ms)
                    if which == "bisect":
                        msms.append(bv.msm_calls)
                    bv.close()
            out["failing"][str(f)] = {"B": B, "positions": where, "each": spread(each), "bisect": spread(bisect),
                                      "bisect_msm_calls": int(statistics.median(msms))}
            print(f"{name} B={B} f={f}: each {spread(each)['median_ms']} ms, bisect {spread(bisect)['median_ms']} ms", file=sys.stderr, flush=True)
    finally:
        params.release()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--circuits", default="merkle_sum_d20_k10,poseidon_k6")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    torch.cuda.init()
    result = {"tool": "tools/verdicts_time.py", "repeats": args.repeats, "modes": MODES,
              "note": "verdicts, finalize and failing exclude the preparation (read, transcript, terms), which both routes share and "
                      "`prepare` states; sums_kernel_ms is device time between events, every other figure wall-clock"}
    for name in args.circuits.split(","):
        result[name] = circuit(name, sizes, args.repeats)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
