#!/usr/bin/env python3
"""Times a circuit's witness call against its two floors, in one process and one run (--circuit: merkle_sum_tree, the default,
hm_merkle_sum_witness_bn256_dev; merkle_v3, hm_merkle_witness_bn256_dev at k = 10 depth 20; poseidon, hm_poseidon_witness_bn256_dev at
k = 6, one hash per user):

    hash floor   hm_poseidon_hash_bn256_fr_dev on the same number of hashes of the circuit's width (the arithmetic alone)
    write floor  hipMemsetAsync of the same output size (every word of the columns is written)

The yardstick is the SUM of the floors.  Shapes: k = 9 depth 5 and k = 10 depth 20, m x depth = 2^16, 2^18,
2^20 hashes, m cut into chunks so that the output stays below --max-gib.  At the default 2 GiB a chunk is 6 553 users (32 765 hashes)
at k = 9 and 3 276 users (65 520 hashes) at k = 10: a few hundred blocks, so the hash floor and the witness alike run on a chip that is
not full; a larger --max-gib shows the filled rate.  Each figure is the median of --reps timed runs after a
warm-up; times are hipEvent times around the whole chunk loop.  The chain kernel of tree-less paths is reported separately.

    python tools/witness_time.py [--circuit merkle_sum_tree] [--hashes 65536 262144 1048576] [--reps 5] [--max-gib 2] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["merkle_sum_tree", "merkle_v3", "poseidon"], default="merkle_sum_tree")
    ap.add_argument("--hashes", type=int, nargs="+", default=[1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-gib", type=float, default=2.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    from halo2_experiments_amd import poseidon as ps, random_fr, synthesis as sy

    # per circuit: spec width, advice columns, elements per node, the (k, depth) shapes
    width, n_advice, elems, shapes = {"merkle_sum_tree": (5, sy.N_ADVICE, 2, ((9, 5), (10, 20))),
                                      "merkle_v3": (3, sy.MerkleTreeV3Layout.N_ADVICE, 1, ((10, 20),)),
                                      "poseidon": (5, sy.PoseidonCircuitLayout.N_ADVICE, 0, ((6, 1),))}[args.circuit]
    spec = ps.default_spec(width)
    results = []
    torch.cuda.init()
    with open("/proc/self/maps") as f:              # the HIP runtime this process already runs on (torch's), not a second copy
        loaded = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    hip = ctypes.CDLL(loaded[0])                    # the write floor is the very call the library issues
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    for k, depth in shapes:
        user_bytes = n_advice * (32 << k)
        for hashes in args.hashes:
            m = hashes // depth
            chunk = max(1, min(m, int(args.max_gib * (1 << 30)) // user_bytes))
            out = torch.empty((chunk, n_advice, 1 << k, 4), dtype=torch.int64, device="cuda")
            msgs = random_fr(chunk * depth * (width - 1), 4, "cuda").view(chunk * depth, width - 1, 4)
            chunks = [chunk] * (m // chunk) + ([m % chunk] if m % chunk else [])
            leaves = sib = idx = nodes = None
            if elems:
                leaves = random_fr(chunk * elems, 1, "cuda").view(chunk, elems, 4)
                sib = random_fr(chunk * depth * elems, 2, "cuda").view(chunk, depth, elems, 4)
                idx = torch.arange(chunk, dtype=torch.int64, device="cuda") * 2654435761 % (1 << depth)
                nodes = random_fr(((2 << depth) - 1) * elems, 3, "cuda").view(-1, elems, 4)      # any node values: the time does not depend on them

            def witness(nodes_arg):
                for c in chunks:
                    if args.circuit == "merkle_sum_tree":
                        sy.merkle_sum_witness(spec, leaves[:c], sib[:c], idx[:c], 1 << 60, k, nodes=nodes_arg, out=out[:c])
                    elif args.circuit == "merkle_v3":
                        sy.merkle_witness(spec, leaves[:c], sib[:c], idx[:c], k, nodes=nodes_arg, out=out[:c])
                    else:
                        sy.poseidon_circuit_witness(spec, msgs[:c], k, out=out[:c])

            def hash_floor():
                for c in chunks:
                    ps.poseidon_hash(spec, msgs[: c * depth])

            def write_floor():
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                for c in chunks:
                    if hip.hipMemsetAsync(ctypes.c_void_p(out.data_ptr()), 0, ctypes.c_size_t(c * user_bytes), stream) != 0:
                        raise RuntimeError("hipMemsetAsync failed")

            t_tree = timed(lambda: witness(nodes))
            t_chain = timed(lambda: witness(None)) if elems else None          # the Poseidon circuit has no path and no chain
            t_hash, t_write = timed(hash_floor), timed(write_floor)
            row = dict(circuit=args.circuit, k=k, depth=depth, hashes=m * depth, users=m, chunk=chunk, output_gib=round(m * user_bytes / (1 << 30), 3),
                       witness_ms=round(t_tree, 3), hash_floor_ms=round(t_hash, 3), write_floor_ms=round(t_write, 3),
                       ratio=round(t_tree / (t_hash + t_write), 3), witness_without_tree_ms=round(t_chain, 3) if elems else None)
            print(json.dumps(row), flush=True)
            results.append(row)
            del leaves, sib, idx, nodes, out, msgs
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
