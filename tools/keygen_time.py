#!/usr/bin/env python3
"""Time of keygen's permutation assembly on the device beside its pure-Python twin, and of ``keygen_vk`` / ``keygen_pk`` whole
(DESIGN.md section 16).

    python tools/keygen_time.py [--shapes real10,tiled18,single18] [--reps 5] [--no-twin] [--json out.json]

Shapes: ``real10`` the MerkleSumTree depth-20 layout at k = 10 (12 equality columns); ``tiled18`` k = 18 / P = 12, that layout's copies
tiled down the rows 256 times; ``single18`` k = 18 / P = 12 with all 3.1 M cells in one class (a chain in ascending order).
Per shape: the device assembly (``hm_permutation_assemble_dev``) and the materialisation (``hm_permutation_columns_bn256_fr_dev``),
hipEvent-timed, best and median of ``--reps``; the upload of the pairs; ``synthesis.permutation_cells`` plus the torch scatter of
``synthesis.permutation_columns`` (wall clock, once); and for the first two shapes ``keygen_vk`` and ``keygen_pk`` whole (wall clock,
synchronised; the fixed columns and the layout tiled likewise; ``ParamsKZG.setup`` is outside the timed part).  The device result is
compared with the twin's whenever the twin runs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_time(fn, reps):
    import torch
    fn()
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
    return round(times[0], 4), round(times[len(times) // 2], 4)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 2)


class TiledLayout:
    """``base`` (a layout at k0) repeated down the rows of a 2^k column: copies, fixed columns and row count tiled alike"""

    def __init__(self, base, k):
        self.base, self.k, self.n, self.tiles = base, k, 1 << k, 1 << (k - base.k)

    def check_constraint_system(self, cs):
        self.base.check_constraint_system(cs)

    def copies(self):
        n0 = self.base.n
        return [((ka, ca, ra + t * n0), (kb, cb, rb + t * n0)) for t in range(self.tiles) for (ka, ca, ra), (kb, cb, rb) in self.base.copies()]

    def fixed_columns(self):
        return [col * self.tiles for col in self.base.fixed_columns()]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="real10,tiled18,single18")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-twin", action="store_true", help="skip the pure-Python twin (minutes at k = 18)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from halo2_experiments_amd import circuits, keygen, synthesis as sy
    from halo2_experiments_amd.domain import EvaluationDomain
    from halo2_experiments_amd.kzg import ParamsKZG

    cs = circuits.merkle_sum_tree()
    base = sy.MerkleSumTreeLayout(20, 10)
    P = len(cs.equality)
    rows = []
    for shape in args.shapes.split(","):
        k = 10 if shape == "real10" else 18
        n = 1 << k
        lay = base if shape == "real10" else TiledLayout(base, k) if shape == "tiled18" else None
        if lay is not None:
            pairs, pairs_ms = _wall(lambda: keygen.copy_pairs(cs, lay))
        else:
            pairs = np.stack([np.arange(P * n - 1, dtype=np.uint32), np.arange(1, P * n, dtype=np.uint32)], axis=1)
            pairs_ms = None
        row = {"shape": shape, "k": k, "columns": P, "copies": int(pairs.shape[0]), "copy_pairs_ms": pairs_ms}
        d_pairs, row["upload_ms"] = _wall(lambda: torch.from_numpy(np.ascontiguousarray(pairs)).cuda())
        row["assemble_ms"], row["assemble_median_ms"] = _event_time(lambda: keygen.permutation_cells_dev(d_pairs, P, k), args.reps)
        cells = keygen.permutation_cells_dev(d_pairs, P, k)
        omega = EvaluationDomain(cs.degree(), k).omega
        row["columns_ms"], row["columns_median_ms"] = _event_time(
            lambda: keygen.permutation_columns_from_cells(cells, P, k, omega, keygen.FR_DELTA), args.reps)
        print(json.dumps(row), flush=True)
        if not args.no_twin:
            stand_in = lay if lay is not None else SimpleNamespace(
                n=n, copies=lambda: [(cs.equality[a // n] + (a % n,), cs.equality[b // n] + (b % n,)) for a, b in pairs.tolist()])
            t0 = time.perf_counter()
            twin = sy.permutation_cells(cs, stand_in)
            row["twin_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps({"shape": shape, "twin_cells_ms": row["twin_cells_ms"]}), flush=True)
            flat = np.array([j * n + i for col in twin for (j, i) in col], dtype=np.uint32)
            row["cells_equal_the_twin"] = bool(np.array_equal(cells.cpu().numpy(), flat))
            del twin, flat
            _, row["twin_columns_ms"] = _wall(lambda: sy.permutation_columns(cs, stand_in, omega, keygen.FR_DELTA))
        if lay is not None:
            params = ParamsKZG.setup(k, 0x1234567)
            try:
                keygen.keygen_vk(params, cs, lay)                                   # warm-up: code objects, tables, pools
                vk, row["keygen_vk_ms"] = _wall(lambda: keygen.keygen_vk(params, cs, lay))
                _, row["keygen_pk_ms"] = _wall(lambda: keygen.keygen_pk(params, vk, cs, lay))
                _, row["keygen_pk_no_cosets_ms"] = _wall(lambda: keygen.keygen_pk(params, vk, cs, lay, cosets=False))
                _, row["fixed_columns_host_ms"] = _wall(lambda: lay.fixed_columns())
            finally:
                params.release()
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
