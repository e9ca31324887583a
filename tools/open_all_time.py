#!/usr/bin/env python3
"""Device time of open_all (all KZG openings of a polynomial on its domain; csrc/g1_fft.hip) at k = 10, 14, 18, 20, the median of
five, split into its parts, and in the same session what it is compared with:

* the floor: g1_fft through the existing entry (hm_g1_fft_bn256_dev, no scale) at sizes 2n and n.  Their sum is what the two stage
  chains of open_all would cost as stand-alone transforms, load and store passes included;
* at k = 10 the looped open_at route (eval_polynomial, kate_division and one MSM per point) over all n points.

    python tools/open_all_time.py [--ks 10,14,18,20] [--reps 5] [--json profiles/r11_open_all_time.json]

Parts (events between the steps inside one call, hm_kzg_open_all_timed_bn256_dev): coefficient arrangement, the Fr NTT of size 2n,
load-multiply (2n scalar multiplications with a scalar per lane), the stages of size 2n, truncation, the stages of size n, the store
(one inversion per proof).  `whole` is the untimed entry between two events of its own, so it also holds the twiddle tables and the
stream-ordered allocation, which no part covers.  The table build (once per size) is timed apart.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("arrange", "ntt", "load_multiply", "stages_2n", "truncate", "stages_n", "store")
S = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F0123456789ABCDEF0


def _device_ms(fn, reps: int):
    import torch

    out = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        keep = fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
        del keep
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="10,14,18,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r11_open_all_time.json"))
    args = ap.parse_args()
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd import openings as op
    from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_words
    from halo2_experiments_amd.kzg import ParamsKZG

    med = statistics.median
    rows = []
    for k in (int(x) for x in args.ks.split(",")):
        n = 1 << k
        params = ParamsKZG.setup(k, S, keep_points=True)
        poly = h.random_fr(n, 9000 + k)
        g = params.g_points
        # the table: built from scratch every time (the cached object is bypassed)
        op.OpeningTable._build(g, k)
        torch.cuda.synchronize()
        table_ms = _device_ms(lambda: op.OpeningTable._build(g, k), args.reps)
        op.open_all(params, poly)                          # first call: the table, the NTT's twiddles, the allocator pool
        torch.cuda.synchronize()
        whole_ms = _device_ms(lambda: op.open_all(params, poly), args.reps)
        parts = []
        for _ in range(args.reps):
            ms = []
            op.open_all(params, poly, part_ms=ms)
            parts.append(ms)
        part_med = {name: med(p[i] for p in parts) for i, name in enumerate(PARTS)}
        # the floor: the two transforms as stand-alone calls of the existing entry
        floor = {}
        for size_k, omega in ((k + 1, op.domain_omega(k + 1)), (k, op.domain_omega(k))):
            pts = op.OpeningTable(params, k).table.clone() if size_k == k + 1 else g[:n].clone()
            w = fr_words(omega)
            h.g1_fft(pts, w, size_k)
            torch.cuda.synchronize()
            floor[size_k] = med(_device_ms(lambda: h.g1_fft(pts, w, size_k), args.reps))
        floor_ms = floor[k + 1] + floor[k]
        whole = med(whole_ms)
        row = {"k": k, "n": n, "reps": args.reps, "table_build_ms": round(med(table_ms), 3),
               "parts_ms": {name: round(v, 3) for name, v in part_med.items()}, "parts_sum_ms": round(sum(part_med.values()), 3),
               "whole_ms": round(whole, 3), "whole_min_max_ms": [round(min(whole_ms), 3), round(max(whole_ms), 3)],
               "us_per_proof": round(whole * 1e3 / n, 4),
               "g1_fft_2n_ms": round(floor[k + 1], 3), "g1_fft_n_ms": round(floor[k], 3), "floor_ms": round(floor_ms, 3),
               "whole_over_floor": round(whole / floor_ms, 3)}
        if k == 10:
            w = op.domain_omega(k)
            zs = [pow(w, i, R) for i in range(n)]
            op.open_at(params, poly, zs[1])
            loops = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for z in zs:
                    op.open_at(params, poly, z)
                torch.cuda.synchronize()
                loops.append((time.perf_counter() - t0) * 1e3)
            row["looped_open_at_wall_ms"] = round(med(loops), 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op.open_all(params, poly)
            torch.cuda.synchronize()
            row["open_all_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["looped_over_open_all"] = round(row["looped_open_at_wall_ms"] / max(row["open_all_wall_ms"], whole), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        params.release()
        del params, poly, g
        torch.cuda.empty_cache()
    with open(args.json, "w") as f:
        json.dump({"tool": "tools/open_all_time.py", "device": torch.cuda.get_device_name(0), "parts": list(PARTS), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
