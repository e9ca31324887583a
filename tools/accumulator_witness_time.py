#!/usr/bin/env python3
"""Times the SafeAccumulator witness call (hm_accumulator_witness_bn256_fr_dev, csrc/accumulator.hip) against a yardstick, in one
process and one run:

    copy         a device-to-device ``copy_`` of the same number of OUTPUT bytes.  The kernels read 32 bytes a row twice (the reduce
                 pass and the row pass) and write 32 * (2 + 2 acc_cols) a row, and between the two passes one block per circuit scans
                 the block totals; the copy reads what it writes.  No ratio is fixed in advance.

Shapes: (max_bits, acc_cols) = (4, 4); one circuit with every usable row at k = 20 and k = 24 (2^k - 7 values), and 64 circuits at
k = 18.  The values are uniform below 2^max_bits, so on nearly every row the top limb is not zero and the lane reads its inverse from
the table -- the costlier case for the row pass; ``--sparse`` adds values that keep the top limb zero.  Each figure is the median of
--reps windows of --iters calls each after a warm-up, witness and copy windows alternating; the smallest and largest window stand
beside it.  Times are hipEvent times around the whole call; the split between its four launches (block totals, their scan, the rows,
the counters) comes from events the library records between them (``parts=``: the call then waits, so these are separate calls,
medians of --reps).

    python tools/accumulator_witness_time.py [--shapes 20:1 24:1 18:64] [--reps 7] [--iters 20] [--json profiles/r15_accumulator_witness_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:1", "24:1", "18:64"], help="k:m pairs")
    ap.add_argument("--max-bits", type=int, default=4)
    ap.add_argument("--acc-cols", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sparse", action="store_true", help="also time values so sparse that the top limb stays zero")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from halo2_experiments_amd import poseidon as ps, synthesis as sy

    b, A = args.max_bits, args.acc_cols
    small = torch.from_numpy(ps.ints_to_words(list(range(1 << b))).view(np.int64)).cuda()
    results = []

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / args.iters

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

    for shape in args.shapes:
        k, m = (int(x) for x in shape.split(":"))
        n, rows = 1 << k, (1 << k) - sy.BLINDING_ROWS - 1
        sy.accumulator_c_layout(k, b, A, rows)
        gen = torch.Generator(device="cuda").manual_seed(k * 100 + m)
        kinds = [("uniform", torch.randint(0, 1 << b, (m, rows), generator=gen, device="cuda"))]
        if args.sparse:
            capacity = (1 << (b * (A - 1))) - 1
            draw = torch.rand((m, rows), generator=gen, device="cuda") < min(1.0, capacity / ((1 << b) * rows))
            sparse = torch.where(draw, torch.randint(0, 1 << b, (m, rows), generator=gen, device="cuda"), 0)
            if int(sparse.sum(dim=1).max()) <= capacity:
                kinds.append(("sparse", sparse))
        initial = torch.zeros((m, A), dtype=torch.int64, device="cuda")
        out = torch.empty((m, 2 + 2 * A, n, 4), dtype=torch.int64, device="cuda")
        src = torch.empty_like(out)
        for kind, plain in kinds:
            values = small[plain].contiguous()
            _, finals, over = sy.accumulator_witness(values, initial, k, b, A, out=out)
            total = plain.sum(dim=1) & ((1 << (b * A)) - 1)
            got = sum(finals[:, i] << (b * (A - 1 - i)) for i in range(A))
            assert torch.equal(got, total), "the final limbs are not the sum of the values"
            src.copy_(out)
            t_witness, t_copy, span_w, span_c = timed_pair(lambda: sy.accumulator_witness(values, initial, k, b, A, out=out),
                                                           lambda: out.copy_(src))
            split = []
            for _ in range(args.reps):
                parts = []
                sy.accumulator_witness(values, initial, k, b, A, out=out, parts=parts)
                split.append(parts)
            split = [round(statistics.median(p[i] for p in split), 4) for i in range(4)]
            out_bytes = out.numel() * 8
            row = dict(max_bits=b, acc_cols=A, k=k, circuits=m, rows=rows, values=kind, failing_rows=int(over.sum()),
                       output_gib=round(out_bytes / (1 << 30), 3), witness_ms=round(t_witness, 4), copy_ms=round(t_copy, 4),
                       ratio=round(t_witness / t_copy, 3), witness_ms_span=[round(v, 4) for v in span_w],
                       copy_ms_span=[round(v, 4) for v in span_c], ratio_span=[round(span_w[0] / span_c[1], 3), round(span_w[1] / span_c[0], 3)],
                       launches_ms=dict(zip(("reduce", "scan", "rows", "count"), split)),
                       witness_write_gbps=round(out_bytes / t_witness / 1e6, 1), copy_write_gbps=round(out_bytes / t_copy / 1e6, 1))
            print(json.dumps(row), flush=True)
            results.append(row)
            del values
        del out, src, kinds
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
