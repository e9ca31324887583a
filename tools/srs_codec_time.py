#!/usr/bin/env python3
"""Device time of the SRS point encodings for 2^(k+1) points (g and g_lagrange of a k SRS) at k = 18 .. 24: decompression (one Fq
square root per point), compression and the checked raw format's validation, hipEvent-timed on the current stream; then the wall time
of ParamsKZG.read(format="processed") against ParamsKZG.read() on the same SRS at one k (written to a temporary file first).

    python tools/srs_codec_time.py [--ks 18,20,22,24] [--reps 3] [--read-k 20] [--json out.json]

Products per decompressed point: 251 squarings + 108 products for the square root, ~8 around it.  The rate is
set beside the ~1.4e11 Fq products/s of K3 to show a shortfall against the VALU floor.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K3_PRODUCTS_PER_S = 2.01e8 * 10 / 14e-3
PRODUCTS_PER_POINT = 251 + 108 + 8


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
    ap.add_argument("--ks", default="18,20,22,24")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--read-k", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd.arithmetic import G1_GENERATOR
    from halo2_experiments_amd.kzg import ParamsKZG

    rows = []
    for k in (int(x) for x in args.ks.split(",")):
        n = 2 << k
        pts = h.g1_fixed_base_mul(h.random_fr(n, 9000 + k), G1_GENERATOR)
        comp = h.g1_compress(pts)
        row = {"k": k, "points": n,
               "decompress_ms": round(_time(lambda: h.g1_decompress(comp), args.reps), 3),
               "compress_ms": round(_time(lambda: h.g1_compress(pts), args.reps), 3),
               "check_ms": round(_time(lambda: h.g1_check(pts), args.reps), 3)}
        rate = n * PRODUCTS_PER_POINT / (row["decompress_ms"] * 1e-3)
        row["decompress_products_per_s"] = rate
        row["fraction_of_k3_rate"] = round(rate / K3_PRODUCTS_PER_S, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pts, comp
        torch.cuda.empty_cache()

    read = None
    if args.read_k:
        k = args.read_k
        params = ParamsKZG.setup(k, 0x5EED, keep_points=True)
        with tempfile.TemporaryDirectory() as d:
            files = {fmt: os.path.join(d, fmt) for fmt in ("raw_unchecked", "processed")}
            for fmt, path in files.items():
                with open(path, "wb") as f:
                    params.write(f, format=fmt)
            params.release()
            read = {"k": k}
            for fmt, path in files.items():
                best = None
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with open(path, "rb") as f:
                        p = ParamsKZG.read(f, format=fmt)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                    p.release()
                    del p
                    best = ms if best is None else min(best, ms)
                read[f"read_{fmt}_ms"] = round(best, 1)
                read[f"file_{fmt}_bytes"] = os.path.getsize(path)
        print(json.dumps(read), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"k3_products_per_s": K3_PRODUCTS_PER_S, "rows": rows, "read": read}, f, indent=1)


if __name__ == "__main__":
    main()
