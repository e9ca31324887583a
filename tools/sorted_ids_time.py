#!/usr/bin/env python3
"""Times the three device steps of the ledger's id proof against their yardsticks, in one process and one run:

  witness   ``synthesis.sorted_witness`` (hm_sorted_witness_bn256_fr_dev, csrc/sorted.inc) at (max_bits, acc_cols) = (16, 8), k = 17
            and k = 20, one circuit with every usable row live, against a device-to-device ``copy_`` of the same number of OUTPUT
            bytes (the kernel reads 64 bytes and writes 32 * (1 + acc_cols) per row and hashes nothing: moving the bytes is its floor).
            The ids ascend with gaps below 2^42, so no lane reaches the counter's atomic.  hipEvent times.
  order     ``ledger.ledger_order`` (hm_fr_argsort_bn256_dev, csrc/sorted.hip) on 2^16 / 2^20 / 2^24 uniformly random ids against
            ``torch.sort`` of n int64 keys returning indices -- a floor with a 32 times narrower key, not a target.  hipEvent times.
  prove     ``ledger.prove_ledger`` at k = 17, one asset, every usable row, with and without ``id_pk``, wall-clock.

Each figure is the median of --reps windows (of --iters calls each for the first two sections), the two routes of a pair alternating
so that both see the same machine; the smallest and largest window stand beside it.

    python tools/sorted_ids_time.py [--sections witness,order,prove] [--reps 7] [--iters 20] [--json profiles/r21_sorted_ids_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="witness,order,prove")
    ap.add_argument("--witness-ks", type=int, nargs="+", default=[17, 20])
    ap.add_argument("--order-sizes", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--prove-k", type=int, default=17)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sections = args.sections.split(",")

    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd import circuits, ledger as lg, synthesis as sy
    from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array
    from halo2_experiments_amd.kzg import ParamsKZG

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def timed_pair(f, g, iters, clock=window):
        """medians of --reps windows, the two alternating so that both see the same machine"""
        f()
        g()
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(args.reps):
            tf.append(clock(f, iters))
            tg.append(clock(g, iters))
        return statistics.median(tf), statistics.median(tg), [round(min(tf), 4), round(max(tf), 4)], [round(min(tg), 4), round(max(tg), 4)]

    def montgomery(plain):
        """(rows,) int64 plain integers below 2^63 -> (rows, 4) canonical Montgomery words: the words (v, 0, 0, 0) are the Montgomery
        form of v 2^-256; times the field element 2^256 they become that of v"""
        words = torch.zeros((plain.shape[0], 4), dtype=torch.int64, device="cuda")
        words[:, 0] = plain
        out = torch.empty_like(words)
        h.linear_combination([words], fr_array([pow(2, 256, R)]), out=out)
        return out

    def ascending(rows, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return montgomery(torch.cumsum(torch.randint(1, 1 << 42, (rows,), dtype=torch.int64, device="cuda", generator=gen), 0))

    result = {"tool": "tools/sorted_ids_time.py", "reps": args.reps, "iters": args.iters, "witness": [], "order": [], "prove": []}

    if "witness" in sections:
        max_bits, acc_cols = 16, 8
        for k in args.witness_ks:
            n, rows = 1 << k, (1 << k) - sy.BLINDING_ROWS
            sy.sorted_c_layout(k, max_bits, acc_cols, rows)
            ids = ascending(rows, seed=k)
            out = torch.empty((1, 1 + acc_cols, n, 4), dtype=torch.int64, device="cuda")
            _, over = sy.sorted_witness(ids, k, max_bits, acc_cols, out=out)
            assert int(over.sum()) == 0
            src = out.clone()
            t_w, t_c, span_w, span_c = timed_pair(lambda: sy.sorted_witness(ids, k, max_bits, acc_cols, out=out), lambda: out.copy_(src),
                                                  args.iters)
            out_bytes = out.numel() * 8
            row = dict(max_bits=max_bits, acc_cols=acc_cols, k=k, rows=rows, output_mib=round(out_bytes / (1 << 20), 1),
                       witness_ms=round(t_w, 4), copy_floor_ms=round(t_c, 4), ratio=round(t_w / t_c, 3), witness_ms_span=span_w,
                       copy_floor_ms_span=span_c, witness_write_gbps=round(out_bytes / t_w / 1e6, 1), copy_write_gbps=round(out_bytes / t_c / 1e6, 1))
            print(json.dumps(row), flush=True)
            result["witness"].append(row)
            del out, src, ids
            torch.cuda.empty_cache()

    if "order" in sections:
        for n in args.order_sizes:
            ids = h.random_fr(n, 21, "cuda")
            keys = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
            perm = lg.ledger_order(ids)
            assert int(perm.sum()) == n * (n - 1) // 2                                          # a permutation's sum, at least
            iters = max(1, min(args.iters, (1 << 22) // n))
            t_o, t_s, span_o, span_s = timed_pair(lambda: lg.ledger_order(ids), lambda: torch.sort(keys)[1], iters)
            row = dict(n=n, iters=iters, ledger_order_ms=round(t_o, 4), torch_sort_int64_ms=round(t_s, 4), ratio=round(t_o / t_s, 2),
                       ledger_order_ms_span=span_o, torch_sort_int64_ms_span=span_s, ns_per_id=round(t_o * 1e6 / n, 2))
            print(json.dumps(row), flush=True)
            result["order"].append(row)
            del ids, keys, perm
            torch.cuda.empty_cache()

    if "prove" in sections:
        k = args.prove_k
        rows = (1 << k) - sy.BLINDING_ROWS
        params = ParamsKZG.setup(k, SRS_S % R, keep_points=True)
        cs, lay = circuits.overflow_check_v2(16, 4, unblinded_value=True), sy.RangeCheckLayout(k, 16, 4, rows=rows)
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        id_cs, id_lay = circuits.sorted_column(16, 8), sy.SortedColumnLayout(k, 16, 8, rows=rows)
        id_vk = h.keygen_vk(params, id_cs, id_lay)
        id_pk = h.keygen_pk(params, id_vk, id_cs, id_lay, cosets=False)
        ids = ascending(rows, seed=5)
        gen = torch.Generator(device="cuda").manual_seed(6)
        bal = montgomery(torch.randint(0, 1 << 48, (rows,), dtype=torch.int64, device="cuda", generator=gen))
        proof = lg.prove_ledger(params, pk, ids, bal, seed=1, id_pk=id_pk)
        assert lg.verify_ledger(params, vk, proof, id_vk=id_vk)
        t_with, t_without, span_with, span_without = timed_pair(lambda: lg.prove_ledger(params, pk, ids, bal, seed=1, id_pk=id_pk),
                                                                lambda: lg.prove_ledger(params, pk, ids, bal, seed=1), 1, clock=wall)
        row = dict(k=k, rows=rows, assets=1, balance_circuit="overflow_check_v2(16, 4)", id_circuit="sorted_column(16, 8)",
                   prove_with_id_pk_ms=round(t_with, 2), prove_without_ms=round(t_without, 2), ratio=round(t_with / t_without, 3),
                   prove_with_id_pk_ms_span=span_with, prove_without_ms_span=span_without, id_proof_bytes=len(proof.id_proof))
        print(json.dumps(row), flush=True)
        result["prove"].append(row)

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
