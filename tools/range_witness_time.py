#!/usr/bin/env python3
"""Times the range-check witness call (hm_range_witness_bn256_fr_dev, csrc/range.inc) against its floor, in one process and one run:

    copy floor   a device-to-device ``copy_`` of the same number of OUTPUT bytes (the kernel reads 32 bytes and writes
                 32 * (1 + acc_cols) per value; it hashes nothing, so moving the bytes is all of its floor)

Shapes: (max_bits, acc_cols) = (16, 4) at k = 17 with every usable row (2^17 - 6 values per circuit), m circuits so that m x rows
is about 2^20 and 2^24 values.  The values are in range (the Montgomery forms of 16-bit integers, taken from a limb column the kernel
itself wrote), so no lane reaches the counter's atomic.  Each figure is the median of --reps windows of --iters calls each after a
warm-up, witness and copy windows alternating; the smallest and largest window stand beside it.  Times are hipEvent times.

    python tools/range_witness_time.py [--values 1048576 16777216] [--reps 7] [--iters 50] [--json profiles/r14_range_witness_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--max-bits", type=int, default=16)
    ap.add_argument("--acc-cols", type=int, default=4)
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    from halo2_experiments_amd import random_fr, synthesis as sy

    k, n, rows, n_advice = args.k, 1 << args.k, (1 << args.k) - sy.BLINDING_ROWS, 1 + args.acc_cols
    sy.range_c_layout(k, args.max_bits, args.acc_cols, rows)
    results = []

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    def timed_pair(f, g):
        """medians of --reps windows of --iters calls each, the two alternating so that both see the same machine"""
        f()
        g()
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(args.reps):
            tf.append(window(f))
            tg.append(window(g))
        return statistics.median(tf), statistics.median(tg), (min(tf), max(tf)), (min(tg), max(tg))

    for count in args.values:
        m = max(1, (count + rows - 1) // rows)
        out = torch.empty((m, n_advice, n, 4), dtype=torch.int64, device="cuda")
        seed_adv, _ = sy.range_witness(random_fr(m * rows, 14, "cuda").view(m, rows, 4), k, args.max_bits, args.acc_cols, out=out)
        values = seed_adv[:, n_advice - 1, :rows].clone()             # the last limb column: Montgomery forms of max_bits-bit integers
        _, over = sy.range_witness(values, k, args.max_bits, args.acc_cols, out=out)
        assert int(over.sum()) == 0
        src = torch.empty_like(out)
        src.copy_(out)
        t_witness, t_copy, span_w, span_c = timed_pair(lambda: sy.range_witness(values, k, args.max_bits, args.acc_cols, out=out),
                                                       lambda: out.copy_(src))
        out_bytes = out.numel() * 8
        row = dict(max_bits=args.max_bits, acc_cols=args.acc_cols, k=k, circuits=m, values=m * rows, output_gib=round(out_bytes / (1 << 30), 3),
                   witness_ms=round(t_witness, 4), copy_floor_ms=round(t_copy, 4), ratio=round(t_witness / t_copy, 3),
                   witness_ms_span=[round(v, 4) for v in span_w], copy_floor_ms_span=[round(v, 4) for v in span_c],
                   witness_write_gbps=round(out_bytes / t_witness / 1e6, 1), copy_write_gbps=round(out_bytes / t_copy / 1e6, 1))
        print(json.dumps(row), flush=True)
        results.append(row)
        del out, src, values, seed_adv
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
