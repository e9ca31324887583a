#!/usr/bin/env python3
"""BatchVerifier.finalize() against a loop of verify_proof, on one MI355X.

For MerkleSumTree depth 20 / k = 10 and Poseidon k = 6, batches of B = 1, 16, 64, 256, 1024 proofs (four distinct proofs of each circuit,
tiled): a fresh BatchVerifier per repeat, every proof added, ``finalize()`` through the pairing -- wall-clock, median of five with
min .. max -- and its split as the object itself records it: the read kernel with its download, the plan and the program of the terms
kernel (built per BatchVerifier), the Blake2b transcripts on the host, the upload of the per-proof records, the terms kernel (waited
for), the sums (four MSMs and the column sum) and the one pairing check.  Beside it, in the same session, ``verify_proof`` in a loop
over at most 16 of the same proofs, per proof.  Prints one JSON object; ``--out FILE`` also writes it.

``--transcript host|device|both`` and ``--pairing host|device|both`` choose where the transcripts and the pairing run (both default to
host: the figures above).  With more than one combination every one is measured in the SAME session, under ``modes`` by
"transcript/pairing"; in device mode ``read``, ``transcript`` and ``terms`` of the split are the times of queueing each call and only
their sum means anything.  With a device transcript the record also holds ``transcript_kernel_ms``: ``hm_verify_transcript_dev``
alone, on a prepared batch, timed with events around the call, and ``read_kernel_ms``: the read kernel alone, likewise.

``--encoding halo2|evm|both`` chooses the proofs' wire format (default halo2: the figures above).  With ``evm``, or ``both``, the
rows stand under ``modes`` by "transcript/pairing/encoding"; ``both`` proves the same witnesses with the same seeds in the two
encodings and interleaves them per B in one session, so that the "halo2" rows are the yardstick of the "evm" rows beside them.  The
host transcript of "evm" is Keccak in pure Python (about half a millisecond per 136-byte block): large B is slow there.

``--multiopen shplonk|gwc|both`` chooses the multiopen scheme the proofs end in (default shplonk: the figures above).  With ``gwc``,
or ``both``, the rows stand under ``modes`` by "transcript/pairing/encoding/multiopen" and every row also holds ``terms_kernel_ms``, the
terms kernel of its scheme alone (events around the call on the prepared batch); ``both`` proves the same witnesses with the same
seeds under the two schemes and interleaves them per B in one session, the "shplonk" rows the yardstick of the "gwc" rows beside them.

``--circuits`` names the constraint systems; an INTEGER among its entries is a number of circuits per proof instead (``--circuits
1,4,16,64``, with or without names beside them) and asks for the multi-circuit measurement in place of the one
above: for every m and every B of ``--sizes``, in one session with the routes alternating, everything on the device --
``finalize()`` and ``verdicts()`` of B ``create_proof_multi`` proofs of m circuits (``BatchVerifier(circuits=m)``); the same two over
the B * m single-circuit proofs of the same witnesses (``create_proofs``), the yardstick; the host ``verify_proof_multi`` per proof,
the oracle; and the terms kernel alone, events around the call on the prepared batch: ``hm_verify_terms_multi_dev`` on the B proofs,
``hm_verify_terms_dev`` on B and on B * m single-circuit proofs."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG                            # noqa: E402
import prover_cases as pc                                                  # noqa: E402

REPEATS = 5
SIZES = (1, 16, 64, 256, 1024)
PHASES = ("read", "plan", "transcript", "upload", "terms", "msm", "pairing")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def read_kernel_ms(bv, repeats):
    """the read kernel of the batch's encoding alone on the proofs a prepared device-mode batch keeps: events around the call, one
    warm-up; the outputs go to arrays of their own"""
    st, lay = bv._prepare(), bv.layout
    B, dev = st["B"], st["d_proofs"].device
    d_bases = torch.zeros((B * lay.own_points + B, 8), dtype=torch.int64, device=dev)
    d_ybytes = None if st["d_ybytes"] is None else torch.zeros_like(st["d_ybytes"])
    d_scalars, d_bad = torch.zeros_like(st["d_scalars"]), torch.zeros(B, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ms = []
    for i in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        bv._queue_read(st["d_proofs"], st["d_table"], d_bases, d_bases[B * lay.own_points:], d_ybytes, d_scalars, d_bad, stream)
        end.record()
        end.synchronize()
        if i:
            ms.append(start.elapsed_time(end))
    assert torch.equal(d_scalars, st["d_scalars"]) and not d_bad.any()
    return spread(ms)


def transcript_kernel_ms(bv, repeats):
    """hm_verify_transcript_dev (or its "evm" sibling) alone on the arrays a prepared device-mode batch keeps: events around the call,
    one warm-up"""
    from halo2_experiments_amd import device_transcript as dt

    st = bv._prepare()
    d_bad = torch.zeros(st["B"], dtype=torch.int32, device=st["d_proofs"].device)
    d_records = st["d_records"].clone()
    ms = []
    for i in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        dt.challenges(bv.layout, bv._digest, None, st["d_proofs"], st["d_ybytes"], d_bad, d_records, preamble=st["preamble"], d_table=st["d_table"])
        end.record()
        end.synchronize()
        if i:
            ms.append(start.elapsed_time(end))
    assert torch.equal(d_records, st["d_records"]) and not d_bad.any()
    return spread(ms)


def terms_kernel_ms(bv, repeats):
    """the terms kernel alone -- the entry the batch's ``circuits`` chooses -- on the arrays a prepared device-mode batch keeps: events
    around the call, one warm-up; the outputs go to arrays of their own"""
    st = bv._prepare()
    dev = st["d_records"].device
    gwc = getattr(bv, "multiopen", "shplonk") == "gwc"             # d_w_left stands where SHPLONK has d_h2_r, and there is no d_h2_l
    out = [torch.empty_like(st[name]) for name in (("d_own", "d_shared", "d_w_left") if gwc else ("d_own", "d_shared", "d_h2_r", "d_h2_l"))]
    out += [None] if gwc else []
    d_bad = torch.zeros(st["B"], dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ms = []
    for i in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        bv._queue_terms(st["plan"], st["B"], st["d_records"], st["d_scalars"], st["d_inst"], d_bad, *out, stream)
        end.record()
        end.synchronize()
        if i:
            ms.append(start.elapsed_time(end))
    assert torch.equal(out[0], st["d_own"]) and torch.equal(out[1], st["d_shared"]) and not d_bad.any()
    return spread(ms)


def multi_circuit(name, counts, sizes, repeats):
    """the multi-circuit measurement of one constraint system (the module's docstring): {m: {B: row}}"""
    import prover_multi_cases as pmc

    out, params, key = {"circuits_per_proof": {}}, None, None
    try:
        for m in counts:
            cs, lay, adv, instances = pmc.build_multi(name, m)
            if params is None:
                params = ParamsKZG.setup(lay.k, pc.SRS_S)
                vk = h.keygen_vk(params, cs, lay)
                key = (vk, h.keygen_pk(params, vk, cs, lay, cosets=False))
                out["k"] = lay.k
            vk, pk = key
            multi = [h.create_proof_multi(params, pk, adv, instances, seed) for seed in (2, 3)]
            singles = h.create_proofs(params, pk, adv, instances, 100)
            inst_arg = instances if m > 1 else instances[0]
            oracle = []
            for proof in multi[:1 if m >= 16 else 2]:
                t0 = time.perf_counter()
                assert h.verify_proof_multi(params, vk, instances, proof)
                oracle.append((time.perf_counter() - t0) * 1e3)
            rows = {"proof_bytes": len(multi[0]), "single_proof_bytes": len(singles[0]),
                    "verify_proof_multi_per_proof": dict(spread(oracle), proofs=len(oracle))}

            def route(B, which):
                """one fresh BatchVerifier, everything on the device: (finalize ms from the constructor on, verdicts ms, the object,
                the ms of the constructor and the add_proof calls alone)"""
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "multi":
                    bv = h.BatchVerifier(params, vk, transcript="device", pairing="device", circuits=m)
                    for b in range(B):
                        bv.add_proof(inst_arg, multi[b % 2])
                else:
                    bv = h.BatchVerifier(params, vk, transcript="device", pairing="device")
                    for b in range(B * m):
                        bv.add_proof(instances[b % m], singles[b % m])
                t_added = time.perf_counter()
                ok = bv.finalize()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                verdicts = bv.verdicts()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                assert ok and all(verdicts)
                return (t1 - t0) * 1e3, (t2 - t1) * 1e3, bv, (t_added - t0) * 1e3

            for which in ("multi", "single"):                    # warm-up: library load, allocator pools, the plans
                route(1, which)[2].close()
            phases = PHASES + ("sums", "verdict_pairing")
            for B in sizes:
                times = {which: ([], []) for which in ("multi", "single")}
                split = {which: {p: [] for p in ("layout_and_add",) + phases} for which in ("multi", "single")}
                kept = {}
                for _ in range(repeats):
                    for which in ("multi", "single"):            # the routes alternate inside every repeat
                        fin, ver, bv, added = route(B, which)
                        times[which][0].append(fin)
                        times[which][1].append(ver)
                        split[which]["layout_and_add"].append(added)
                        for p in phases:
                            split[which][p].append(bv.timings[p] * 1e3)
                        if which in kept:
                            kept[which].close()
                        kept[which] = bv
                row = {"multi": {"proofs": B, "finalize": spread(times["multi"][0]), "verdicts_after_finalize": spread(times["multi"][1]),
                                 "terms_kernel_ms": terms_kernel_ms(kept["multi"], repeats)},
                       "single_yardstick": {"proofs": B * m, "finalize": spread(times["single"][0]),
                                            "verdicts_after_finalize": spread(times["single"][1]),
                                            "terms_kernel_ms": terms_kernel_ms(kept["single"], repeats)}}
                for which, route_name in (("multi", "multi"), ("single", "single_yardstick")):
                    row[route_name]["split_median_ms"] = {p: round(statistics.median(v), 3) for p, v in split[which].items()}
                for bv in kept.values():
                    bv.close()
                lanes = h.BatchVerifier(params, vk, transcript="device", pairing="device")     # the single-circuit kernel on B lanes
                for b in range(B):
                    lanes.add_proof(instances[b % m], singles[b % m])
                row["single_terms_kernel_ms_at_B_proofs"] = terms_kernel_ms(lanes, repeats)
                lanes.close()
                row["per_circuit_ms"] = {"multi": round(row["multi"]["finalize"]["median_ms"] / (B * m), 4),
                                         "single_yardstick": round(row["single_yardstick"]["finalize"]["median_ms"] / (B * m), 4),
                                         "verify_proof_multi": round(rows["verify_proof_multi_per_proof"]["median_ms"] / m, 4)}
                rows[str(B)] = row
                print(f"{name} m={m} B={B}: multi {row['multi']['finalize']['median_ms']} ms, {B * m} singles "
                      f"{row['single_yardstick']['finalize']['median_ms']} ms, terms {row['multi']['terms_kernel_ms']['median_ms']} / "
                      f"{row['single_terms_kernel_ms_at_B_proofs']['median_ms']} ms", file=sys.stderr, flush=True)
            out["circuits_per_proof"][str(m)] = rows
    finally:
        if params is not None:
            params.release()
    return out


def circuit(name, sizes, repeats, modes=(("host", "host"),), encodings=("halo2",), multiopens=("shplonk",)):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    try:
        schemes = multiopens != ("shplonk",)                     # a second scheme asked for: its name goes into every key
        made = {(e, mo): [h.create_proof(params, pk, advice, instance, seed, encoding=e, multiopen=mo) for seed in (2, 3, 4, 5)]
                for e in encodings for mo in multiopens}
        plain = encodings == ("halo2",) and not schemes          # the record's shape before there was a second encoding or scheme
        first = (encodings[0], multiopens[0])
        out = {"k": lay.k, "batches": {},
               "proof_bytes": len(made[first][0]) if plain else {"/".join(key) if schemes else key[0]: len(p[0]) for key, p in made.items()}}
        single = []
        for i in range(min(16, max(sizes))):
            t0 = time.perf_counter()
            assert h.verify_proof(params, vk, instance, made[first][i % 4], encoding=first[0], multiopen=first[1])
            single.append((time.perf_counter() - t0) * 1e3)
        out["verify_proof_per_proof"] = dict(spread(single), proofs=len(single), encoding=encodings[0])
        if schemes:
            out["verify_proof_per_proof"]["multiopen"] = multiopens[0]
        runs = [(t, p, e, mo) for t, p in modes for e in encodings for mo in multiopens]   # encodings and schemes of one mode side by side
        for transcript, pairing, encoding, mo in runs:            # warm-up: library load, allocator pools
            h.verify_proofs(params, vk, [instance], made[(encoding, mo)][:1], transcript=transcript, pairing=pairing, encoding=encoding,
                            multiopen=mo)
        for B in sizes:
            for transcript, pairing, encoding, mo in runs:
                proofs = made[(encoding, mo)]
                total, split = [], {p: [] for p in PHASES}
                for _ in range(repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    bv = h.BatchVerifier(params, vk, transcript=transcript, pairing=pairing, encoding=encoding, multiopen=mo)
                    for b in range(B):
                        bv.add_proof(instance, proofs[b % 4])
                    ok = bv.finalize()
                    torch.cuda.synchronize()
                    total.append((time.perf_counter() - t0) * 1e3)
                    assert ok
                    for p in PHASES:
                        split[p].append(bv.timings[p] * 1e3)
                row = {"finalize": spread(total), "per_proof_ms": round(statistics.median(total) / B, 3),
                       "split_median_ms": {p: round(statistics.median(v), 3) for p, v in split.items()}}
                row["against_verify_proof_loop"] = round(out["verify_proof_per_proof"]["median_ms"] * B / statistics.median(total), 2)
                if transcript == "device":
                    row["transcript_kernel_ms"] = transcript_kernel_ms(bv, repeats)
                    row["read_kernel_ms"] = read_kernel_ms(bv, repeats)
                if schemes:
                    row["terms_kernel_ms"] = terms_kernel_ms(bv, repeats)
                if len(runs) == 1 and plain:
                    out["batches"][str(B)] = row
                else:
                    key = f"{transcript}/{pairing}" if plain else f"{transcript}/{pairing}/{encoding}" + (f"/{mo}" if schemes else "")
                    out.setdefault("modes", {}).setdefault(key, {})[str(B)] = row
                bv.close()
                print(f"{name} B={B} {transcript}/{pairing}/{encoding}/{mo}: {row['finalize']['median_ms']} ms", file=sys.stderr, flush=True)
        if "modes" in out:
            del out["batches"]
    finally:
        params.release()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--transcript", choices=("host", "device", "both"), default="host")
    ap.add_argument("--pairing", choices=("host", "device", "both"), default="host")
    ap.add_argument("--encoding", choices=("halo2", "evm", "both"), default="halo2")
    ap.add_argument("--multiopen", choices=("shplonk", "gwc", "both"), default="shplonk")
    ap.add_argument("--circuits", default="merkle_sum_d20_k10,poseidon_k6")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    both = lambda choice: ("host", "device") if choice == "both" else (choice,)
    modes = tuple((t, p) for p in both(args.pairing) for t in both(args.transcript))
    encodings = ("halo2", "evm") if args.encoding == "both" else (args.encoding,)
    multiopens = ("shplonk", "gwc") if args.multiopen == "both" else (args.multiopen,)
    torch.cuda.init()
    result = {"tool": "tools/batch_verify_time.py", "repeats": args.repeats, "modes_measured": [f"{t}/{p}" for t, p in modes],
              "encodings_measured": list(encodings),
              "host": "the transcripts (Blake2b by hashlib; Keccak in pure Python) and the pairing, unless the mode (transcript/pairing) says "
                      "device; everything else (read, terms, column sum, MSMs) on the device"}
    if multiopens != ("shplonk",):
        result["multiopens_measured"] = list(multiopens)
    entries = args.circuits.split(",")
    counts = [int(e) for e in entries if e.isdigit()]
    names = [e for e in entries if not e.isdigit()] or ["merkle_sum_d20_k10", "poseidon_k6"]
    if counts:
        result.update(modes_measured=["device/device"], encodings_measured=["halo2"], circuits_per_proof=counts,
                      routes="multi: B create_proof_multi proofs of m circuits; single_yardstick: the B * m single-circuit proofs of the "
                             "same witnesses; both finalize() then verdicts() on a fresh BatchVerifier, transcript and pairing on the device")
    for name in names:
        result[name] = multi_circuit(name, counts, sizes, args.repeats) if counts else circuit(name, sizes, args.repeats, modes, encodings, multiopens)
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
