#!/usr/bin/env python3
"""Ledger openings on one MI355X: what checking many users costs, and what making every user's opening costs.

Everything in ONE session, medians of five with min .. max, the compared routes taking turns inside every repeat, their order
rotating.  No range proof is made: the id column is uniformly random field elements, the balance columns uniformly random 48-bit
integers (range-sized, as real balances are), committed to -- all that the user checks read.

  users     at k = 16 with P = 1 and P = 4 assets, B = 64 / 4 096 / 65 536 rows drawn at random with repetition AT EVERY SIZE
            (so the largest batch holds about 63 % of the ledger's rows, some of them several times):
              pairs_kernel_ms     ``hm_kzg_ledger_pairs_bn256_dev`` alone on device arrays, events around the call
              verify_users_ms     ``ledger.verify_ledger_users`` end to end with a ``LedgerStatement`` made once per ledger (ids,
                                  balances and openings on the device, the rows an array); verify_users_public_ms: the same with
                                  the bare commitments, gamma and C_gamma derived in every call
              pairing_floor_ms    ``device_pairing.run_device`` alone on the rows the kernel wrote, wall-clock with its download
            and at B = 64, P = 1, taking turns with them, the route it replaces, ``solvency.verify_users(pairing="device")`` on the
            balance column's own openings, whose host scalar multiplications make a larger B pointless to time
  openings  at k = 16 and k = 18 with P = 4: ``ledger.ledger_openings`` (one combination, ONE open_all) against
            ``solvency.user_openings`` of the 4-column stack (four open_all), wall-clock

Prints one JSON object; ``--out FILE`` also writes it."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd import device_pairing, ledger as lg, solvency  # noqa: E402
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array, fr_ints, g1_ints    # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG                           # noqa: E402
from halo2_experiments_amd.openings import open_all                       # noqa: E402

REPEATS = 5
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def make_ledger(params, k, assets, seed):
    """a uniformly random id column and `assets` columns of uniformly random 48-bit balances, (P + 1, n, 4) -> a LedgerProof that
    carries them and their commitments"""
    n = 1 << k
    columns = torch.zeros((assets + 1, n, 4), dtype=torch.int64, device="cuda")
    columns[0] = h.random_fr(n, seed, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    plain = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    for p in range(assets):
        # the words (v, 0, 0, 0) are the Montgomery form of v 2^-256; times the field element 2^256 they become that of v
        plain[:, 0] = torch.randint(0, 1 << 48, (n,), dtype=torch.int64, device="cuda", generator=gen)
        h.linear_combination([plain], fr_array([pow(2, 256, R)]), out=columns[1 + p])
    points = [g1_ints(params.commit_lagrange(columns[j])) for j in range(assets + 1)]
    return lg.LedgerProof(points[0], points[1:], [], 0, [], None, columns)


def users_section(params, k, assets, sizes, repeats, with_yardstick):
    proof = make_ledger(params, k, assets, seed=7 + assets)
    n, cols = 1 << k, proof.columns
    openings = lg.ledger_openings(params, proof)
    statement = lg.ledger_statement(params, proof)
    out = {}
    for B in sizes:
        rng = random.Random(f"ledger rows {B}")
        rows = np.array([rng.randrange(n) for _ in range(B)], dtype=np.int64)                   # at random, with repetition, at every size
        idx = torch.from_numpy(rows).cuda()
        ids, bal, pis = cols[0][idx].contiguous(), cols[1:, idx].permute(1, 0, 2).contiguous(), openings[idx].contiguous()
        _, (d_g1, d_flags, d_g2) = lg.ledger_pairs(params, statement, rows, ids, bal, pis)      # warm-up, and the rows the floor runs on
        d_idx = idx.to(torch.int32)
        d_off = torch.arange(0, 2 * B + 1, 2, dtype=torch.int32, device="cuda")
        routes = {"whole": lambda: lg.verify_ledger_users(params, statement, rows, ids, bal, pis),
                  "public": lambda: lg.verify_ledger_users(params, proof, rows, ids, bal, pis),
                  "floor": lambda: (device_pairing.run_device(d_g1, d_g2, d_off, B).cpu() == 1).tolist()}
        if with_yardstick and B == min(sizes):
            own = open_all(params, cols[1], form="lagrange")[idx].contiguous()
            values = fr_ints(bal[:, 0].cpu().numpy().view(np.uint64))
            assert max(values) < 1 << 48
            routes["solvency"] = lambda: solvency.verify_users(params, proof.commitments[0], rows.tolist(), values, own, pairing="device", k=k)
        names = list(routes)
        for name in names:
            assert routes[name]() == [True] * B                                                 # warm-up of every route
        kernel, ms = [], {name: [] for name in names}
        for r in range(repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            got = lg.launch_pairs(k, statement.gamma, statement.c_gamma, d_idx, ids, bal, pis)
            end.record()
            end.synchronize()
            kernel.append(start.elapsed_time(end))
            assert torch.equal(got[0], d_g1)
            for name in names[r % len(names):] + names[:r % len(names)]:                        # the routes take turns, the order rotates
                ok, t = wall(routes[name])
                assert ok == [True] * B
                ms[name].append(t)
        row = {"pairs_kernel_ms": spread(kernel), "verify_users_ms": spread(ms["whole"]), "verify_users_public_ms": spread(ms["public"]),
               "pairing_floor_ms": spread(ms["floor"]), "distinct_rows": int(len(set(rows.tolist())))}
        row["us_per_user"] = round(row["verify_users_ms"]["median_ms"] * 1e3 / B, 3)
        row["kernel_us_per_user"] = round(row["pairs_kernel_ms"]["median_ms"] * 1e3 / B, 3)
        if "solvency" in ms:
            row["solvency_verify_users_ms"] = spread(ms["solvency"])
        out[str(B)] = row
        print(f"k={k} P={assets} B={B}: kernel {row['pairs_kernel_ms']['median_ms']} ms, verify_ledger_users "
              f"{row['verify_users_ms']['median_ms']} ms ({row['verify_users_public_ms']['median_ms']} from the commitments), pairing floor "
              f"{row['pairing_floor_ms']['median_ms']} ms", file=sys.stderr, flush=True)
    return out


def openings_section(params, k, assets, repeats):
    proof = make_ledger(params, k, assets, seed=31 + k)
    stack = proof.columns[1:].contiguous()
    lg.ledger_openings(params, proof)                                # warm-up: the opening table of this size, allocator pools
    one, per_asset = [], []
    for r in range(repeats):
        for which in (("one", "per_asset") if r % 2 == 0 else ("per_asset", "one")):
            if which == "one":
                one.append(wall(lambda: lg.ledger_openings(params, proof))[1])
            else:
                per_asset.append(wall(lambda: solvency.user_openings(params, stack))[1])
    row = {"ledger_openings_ms": spread(one), "user_openings_ms": spread(per_asset)}
    row["ratio"] = round(row["user_openings_ms"]["median_ms"] / row["ledger_openings_ms"]["median_ms"], 2)
    print(f"k={k} P={assets}: ledger_openings {row['ledger_openings_ms']['median_ms']} ms, user_openings {row['user_openings_ms']['median_ms']} ms",
          file=sys.stderr, flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--assets", default="1,4")
    ap.add_argument("--open-ks", default="16,18")
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    open_ks = tuple(int(s) for s in args.open_ks.split(",")) if args.open_ks else ()
    torch.cuda.init()
    result = {"tool": "tools/ledger_time.py", "repeats": args.repeats, "k": args.k, "users": {}, "openings": {},
              "note": "pairs_kernel_ms is device time between events; every other figure wall-clock with a synchronize on both sides, "
                      "verify_users_ms and pairing_floor_ms with their download; no hardware counters were taken"}
    params = {}
    for k in sorted(set((args.k,) + open_ks)):
        params[k] = ParamsKZG.setup(k, SRS_S, keep_points=True)
    for assets in (int(a) for a in args.assets.split(",")):
        result["users"][f"P={assets}"] = users_section(params[args.k], args.k, assets, sizes, args.repeats, with_yardstick=assets == 1)
    for k in open_ks:
        result["openings"][f"k={k}"] = openings_section(params[k], k, 4, args.repeats)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
