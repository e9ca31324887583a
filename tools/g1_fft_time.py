#!/usr/bin/env python3
"""Device time of g_to_lagrange (best_fft over BN256 G1 with omega^-1 and the n^-1 scale: hm_g1_fft_bn256_dev) at k = 16 .. 24, and
the Fq-product rate it implies, set beside K3's (the MSM's bucket accumulation kernel), so that a large shortfall against the VALU
floor shows.

    python tools/g1_fft_time.py [--ks 16,18,20,22,24] [--reps 2] [--json out.json]

Products per call: a butterfly is one binary scalar multiplication by a 254-bit twiddle -- 254 doublings of
~7 products and, in the wave-uniform stages, ~127 additions of ~16 (every bit costs an addition in the last six, lane-divergent
stages) -- plus two complete additions; the store pass adds the n^-1 multiplication and one Fermat inversion (~380 products) per point.
K3's rate: 2.01e8 mixed additions x ~10 products in ~14 ms = ~1.4e11 products/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K3_PRODUCTS_PER_S = 2.01e8 * 10 / 14e-3
DBL, ADD, INV = 7, 16, 380


def products(k: int) -> float:
    n = 1 << k
    uniform = max(k - 6, 0)
    per_uniform = 254 * DBL + 127 * ADD + 2 * ADD
    per_divergent = 254 * DBL + 254 * ADD + 2 * ADD
    stages = (n // 2) * (uniform * per_uniform + (k - uniform) * per_divergent)
    store = n * (254 * DBL + 127 * ADD + INV)
    return float(stages + store)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="16,18,20,22,24")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd.arithmetic import G1_GENERATOR

    rows = []
    for k in (int(x) for x in args.ks.split(",")):
        g = h.g1_fixed_base_mul(h.random_fr(1 << k, 7000 + k), G1_GENERATOR)
        h.g_to_lagrange(g, k)                         # first call: twiddles, allocator pool
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = h.g_to_lagrange(g, k)
            end.record()
            end.synchronize()
            ms = start.elapsed_time(end)
            best = ms if best is None else min(best, ms)
            del out
        rate = products(k) / (best * 1e-3)
        row = {"k": k, "device_ms": round(best, 2), "products": products(k), "products_per_s": rate,
               "fraction_of_k3_rate": round(rate / K3_PRODUCTS_PER_S, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"k3_products_per_s": K3_PRODUCTS_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
