#!/usr/bin/env python3
"""Device time of Poseidon over BN256 Fr and of the Merkle sum tree, hipEvent-timed on the current stream: n = 2^16 .. 2^24 hashes at
widths 3 and 5, a depth-20 and a depth-24 sum tree, 2^16 paths of the depth-20 tree; then, for scale, the CPU time per hash of a naive
big-integer permutation (the tests' checker, tests/poseidon_checker.py) on a small n.

    python tools/poseidon_time.py [--logs 16,18,20,22,24] [--depths 20,24] [--reps 3] [--json out.json]

The model beside every figure: Fr products per hash x hashes / 1.9e11 products/s, the rate ff29.h's product
runs at in the NTT and MSM kernels.  Products per hash: 64 rounds of WIDTH^2 MDS terms plus 3 per S-box (x^5), i.e. 64 W^2 +
3 (8 W + 56); the kernel folds the WIDTH terms of an MDS row into one reduction, so it does fewer wide multiplies than that count.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODEL_PRODUCTS_PER_S = 1.9e11


def products_per_hash(width: int, r_f: int = 8, r_p: int = 56) -> int:
    return (r_f + r_p) * width * width + 3 * (r_f * width + r_p)


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        best = ms if best is None else min(best, ms)
    return best


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--logs", default="16,18,20,22,24")
    ap.add_argument("--depths", default="20,24")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd import _lib
    from halo2_experiments_amd import poseidon as P
    from halo2_experiments_amd.arithmetic import _stream_ptr

    out = {"model_products_per_s": MODEL_PRODUCTS_PER_S, "hash": [], "tree": [], "paths": None, "cpu": []}
    for width in (3, 5):
        spec = P.default_spec(width)
        for log_n in (int(x) for x in args.logs.split(",")):
            n = 1 << log_n
            msgs = h.random_fr(n * (width - 1), 100 + log_n).reshape(n, width - 1, 4)
            ms = _time(lambda: P.poseidon_hash(spec, msgs), args.reps)
            model = products_per_hash(width) * n / MODEL_PRODUCTS_PER_S * 1e3
            row = {"width": width, "log_n": log_n, "ms": round(ms, 3), "model_ms": round(model, 3), "hashes_per_s": n / (ms * 1e-3),
                   "fraction_of_model": round(model / ms, 3)}
            out["hash"].append(row)
            print(json.dumps(row), flush=True)
            del msgs
            torch.cuda.empty_cache()

    for depth in (int(x) for x in args.depths.split(",")):
        n = 1 << depth
        leaves = h.random_fr(2 * n, 200 + depth).reshape(n, 2, 4)
        keep = {}

        def build():
            keep["tree"] = P.MerkleSumTree.build(leaves)
        ms = _time(build, args.reps)
        model = products_per_hash(5) * (n - 1) / MODEL_PRODUCTS_PER_S * 1e3
        row = {"sum_tree_depth": depth, "ms": round(ms, 3), "model_ms": round(model, 3), "fraction_of_model": round(model / ms, 3)}
        out["tree"].append(row)
        print(json.dumps(row), flush=True)
        if depth == 20:
            tree = keep["tree"]
            idx = torch.randint(0, n, (1 << 16,), dtype=torch.int64, device="cuda")
            dst = torch.empty((1 << 16, depth, 2, 4), dtype=torch.int64, device="cuda")

            def gather():
                _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(tree.nodes.data_ptr()), depth, 2,
                                                           ctypes.cast(ctypes.c_void_p(idx.data_ptr()), ctypes.POINTER(ctypes.c_uint64)),
                                                           1 << 16, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(_stream_ptr(dst))))
            out["paths"] = {"depth": depth, "paths": 1 << 16, "ms": round(_time(gather, args.reps), 3)}
            print(json.dumps(out["paths"]), flush=True)
            del tree, idx, dst
        keep.clear()
        del leaves
        torch.cuda.empty_cache()

    import poseidon_checker as chk
    rng = random.Random(1)
    for width in (3, 5):
        rc, mds, _ = P.default_spec(width).constants()
        msgs = [[rng.randrange(chk.R) for _ in range(width - 1)] for _ in range(args.cpu_n)]
        t0 = time.perf_counter()
        for m in msgs:
            chk.digest(m, rc, mds, 8, 56)
        row = {"width": width, "cpu_checker_ms_per_hash": round((time.perf_counter() - t0) * 1e3 / args.cpu_n, 3)}
        out["cpu"].append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
