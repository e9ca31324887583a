#!/usr/bin/env python3
"""Device time of ``tree.update`` and of ``path_roots``, hipEvent-timed on the current stream, beside two floors
taken in the same run: ``build`` of the same tree, and ``poseidon_hash`` of as many hashes as ``update_plan`` sums.

    python tools/merkle_update_time.py [--depths 20,24] [--step 4] [--reps 5] [--tree sum|plain] [--json out.json]

Per depth: m = 2^0, 2^step, ... 2^depth entries in two patterns, distinct uniform indices and one contiguous run of m leaves.  Every
row gives the hashes of the plan, the update's time, the time of the hash floor and both ratios; the last row per pattern names the
smallest m at which update is no longer faster than build.  Then ``path_roots`` of 2^16 and 2^20 paths at depth 20.
An update changes the tree, which changes nothing about the next one's work: the timed repeats run on the same tree.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    import torch
    fn()                                   # warm-up: code objects, the stream-ordered pool, this shape's launches
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    times.sort()
    return times[0], times[len(times) // 2]


def _plan_hashes(depth, idx):
    """sum of update_plan's levels 1 .. depth, computed with numpy (the pure-Python sets are slow at 2^24 entries)"""
    import numpy as np
    live = np.unique(np.asarray(idx, dtype=np.int64))
    total = 0
    for _ in range(depth):
        live = np.unique(live >> 1)
        total += int(live.size)
    return total


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depths", default="20,24")
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default="sum", choices=("sum", "plain"))
    ap.add_argument("--roots", default="16,20")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd import _lib
    from halo2_experiments_amd import poseidon as P

    cls = P.MerkleSumTree if args.tree == "sum" else P.MerkleTree
    spec = P.default_spec(cls.WIDTH)
    E = cls.ELEMS
    out = {"tree": args.tree, "update": [], "crossover": [], "roots": []}
    rng = random.Random(15)
    for depth in (int(x) for x in args.depths.split(",") if x):
        n = 1 << depth
        leaves = h.random_fr(n * E, 300 + depth).reshape(n, E, 4)
        build_ms, _ = _time(lambda: cls.build(leaves, spec), args.reps)
        tree = cls.build(leaves, spec)
        fresh = h.random_fr(n * E, 400 + depth).reshape(n, E, 4)
        msgs = h.random_fr(n * (cls.WIDTH - 1), 500 + depth).reshape(n, cls.WIDTH - 1, 4)
        print(json.dumps({"depth": depth, "build_ms": round(build_ms, 3)}), flush=True)
        for pattern in ("uniform", "run"):
            crossover = None
            for log_m in sorted(set(list(range(0, depth + 1, args.step)) + [depth])):
                m = 1 << log_m
                if pattern == "uniform":
                    idx = np.random.default_rng(depth * 100 + log_m).permutation(n)[:m].astype(np.int64)
                else:
                    idx = np.arange(m, dtype=np.int64) + rng.randrange(n - m + 1)
                hashes = _plan_hashes(depth, idx)
                d_idx = torch.from_numpy(idx).cuda()
                new = fresh[:m]
                best, median = _time(lambda: tree.update(d_idx, new), args.reps)
                floor, _ = _time(lambda: P.poseidon_hash(spec, msgs[:hashes]), args.reps)
                row = {"depth": depth, "pattern": pattern, "log_m": log_m, "plan_hashes": hashes, "update_ms": round(best, 4),
                       "update_median_ms": round(median, 4), "hash_floor_ms": round(floor, 4), "update_over_hash_floor": round(best / floor, 2),
                       "update_over_build": round(best / build_ms, 4)}
                out["update"].append(row)
                print(json.dumps(row), flush=True)
                if crossover is None and best >= build_ms:
                    crossover = log_m
            out["crossover"].append({"depth": depth, "pattern": pattern, "first_log_m_not_faster_than_build": crossover})
            print(json.dumps(out["crossover"][-1]), flush=True)
        if depth == 20 and args.roots:
            for log_m in (int(x) for x in args.roots.split(",")):
                m = 1 << log_m
                d_idx = torch.from_numpy(np.random.default_rng(log_m).integers(0, n, m).astype(np.int64)).cuda()
                sib = torch.empty((m, depth, E, 4), dtype=torch.int64, device="cuda")
                _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(tree.nodes.data_ptr()), depth, E,
                                                           ctypes.cast(ctypes.c_void_p(d_idx.data_ptr()), ctypes.POINTER(ctypes.c_uint64)), m,
                                                           ctypes.c_void_p(sib.data_ptr()), None))
                lv = tree.nodes[d_idx].contiguous()
                best, median = _time(lambda: cls.path_roots(lv, sib, d_idx, spec), args.reps)
                ok = bool(torch.equal(cls.path_roots(lv, sib, d_idx, spec), tree.nodes[-1:].expand(m, E, 4)))
                floor, _ = _time(lambda: P.poseidon_hash(spec, msgs[:min(n, m * depth)]), args.reps)
                row = {"depth": depth, "paths": m, "hashes": m * depth, "roots_ms": round(best, 3), "roots_median_ms": round(median, 3),
                       "hash_floor_hashes": min(n, m * depth), "hash_floor_ms": round(floor, 3), "all_equal_the_root": ok}
                out["roots"].append(row)
                print(json.dumps(row), flush=True)
                del sib, lv
        del tree, leaves, fresh, msgs
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
