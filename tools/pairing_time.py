#!/usr/bin/env python3
"""The device pairing (csrc/pairing.inc) timed on one MI355X.

* ``hm_pairing_check_bn256_dev`` alone on n = 1, 64, 4096, 65536 checks of two pairs each (a KZG-shaped relation, the same for every
  check: the work does not depend on the data), buffers resident, hipEvent time around the call's two launches -- median of five with
  min .. max -- and beside it ``pairing.pairing_check`` of one such check on the host integers.
* ``BatchVerifier.finalize()`` on Poseidon k = 6 batches of B = 1, 16, 256, 1024 with ``pairing="host"`` and ``pairing="device"``,
  alternating in the same session: wall-clock and the object's own ``timings["pairing"]``, median of five.

Prints one JSON object; ``--out FILE`` also writes it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd import _lib, device_pairing as dp               # noqa: E402
from halo2_experiments_amd import pairing as pr                            # noqa: E402
from halo2_experiments_amd.bn256 import FR_MODULUS as R                    # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG, g2_mul                    # noqa: E402
import prover_cases as pc                                                  # noqa: E402

REPEATS = 5
CHECKS = (1, 64, 4096, 65536)
BATCHES = (1, 16, 256, 1024)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def device_checks(sizes, repeats):
    a, b = 0x1234567, 0x89ABCDEF0123
    check = [(pr.g1_mul(a), g2_mul(b)), (pr.g1_mul(-a * b % R), pr.G2_GENERATOR)]
    t0 = time.perf_counter()
    assert pr.pairing_check(check)
    host_ms = (time.perf_counter() - t0) * 1e3
    w1, w2, _ = dp._marshal([check])
    lib = _lib.load()
    vp, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
    out = {"host_pairing_check_ms": round(host_ms, 3), "pairs_per_check": 2, "checks": {}}
    for n in sizes:
        dev = lambda arr, t: torch.from_numpy(np.ascontiguousarray(arr).view(t)).to("cuda")
        d_g1, d_g2 = dev(np.tile(w1, (n, 1)), np.int64), dev(np.tile(w2, (n, 1)), np.int64)
        d_off = dev(np.arange(0, 2 * n + 1, 2, dtype=np.uint32), np.int32)
        work_bytes = lib.hm_pairing_work_bytes(2 * n, n)
        d_work = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device="cuda")
        d_status = torch.empty(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        call = lambda: _lib.check(lib.hm_pairing_check_bn256_dev(vp(d_g1.data_ptr()), vp(d_g2.data_ptr()), 2 * n, ctypes.cast(vp(d_off.data_ptr()), u32p),
                                                                 n, None, ctypes.cast(vp(d_status.data_ptr()), u32p), vp(d_work.data_ptr()),
                                                                 work_bytes, vp(stream)))
        call()                                                             # warm-up
        torch.cuda.synchronize()
        assert bool((d_status == 1).all())
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        row = spread(ms)
        row["per_check_us"] = round(statistics.median(ms) * 1e3 / n, 2)
        row["work_mib"] = round(work_bytes / 2 ** 20, 2)
        out["checks"][str(n)] = row
    return out


def finalize_batches(sizes, repeats):
    cs, lay, advice, instance, _ = pc.build("poseidon_k6")
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    out = {"circuit": "poseidon_k6", "batches": {}}
    try:
        proofs = [h.create_proof(params, pk, advice, instance, seed) for seed in (2, 3, 4, 5)]
        for mode in dp.MODES:                                              # warm-up: library load, allocator pools, both routes
            assert h.verify_proofs(params, vk, [instance], proofs[:1], pairing=mode)
        for B in sizes:
            total = {m: [] for m in dp.MODES}
            pairing = {m: [] for m in dp.MODES}
            for _ in range(repeats):
                for mode in dp.MODES:                                      # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    bv = h.BatchVerifier(params, vk, pairing=mode)
                    for b in range(B):
                        bv.add_proof(instance, proofs[b % 4])
                    ok = bv.finalize()
                    torch.cuda.synchronize()
                    total[mode].append((time.perf_counter() - t0) * 1e3)
                    pairing[mode].append(bv.timings["pairing"] * 1e3)
                    assert ok
            out["batches"][str(B)] = {m: {"finalize": spread(total[m]), "pairing": spread(pairing[m])} for m in dp.MODES}
    finally:
        params.release()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--checks", default=",".join(map(str, CHECKS)))
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.init()
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "device_checks": device_checks(tuple(int(s) for s in args.checks.split(",")), args.repeats),
              "batch_verifier_finalize": finalize_batches(tuple(int(s) for s in args.batches.split(",")), args.repeats)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
