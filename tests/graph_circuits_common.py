"""What the two suites of hm_graph_evaluate_circuits_dev share (tests/test_graph_circuits_host.py, tests/test_graph_circuits_gpu.py): the
programs of tests/graph_programs.py that have the admitted shape, hand-made programs for the shapes that list lacks, per-circuit
inputs, and the host replay of the fold (csrc/host_check.cpp: hc_graph_circuits_replay)."""
import ctypes
import random
from dataclasses import dataclass, replace
from typing import List

import numpy as np

import graph_programs as gp
from halo2_experiments_amd import evaluation as ev

R = gp.R


def is_admitted(p: gp.Program) -> bool:
    try:
        ev.linear_in_previous(p.lower()["calcs"])
        return True
    except ValueError:
        return False


def three_terms() -> gp.Program:
    """Horner(PreviousValue, [a0 * a1(+1), f2(-1, period 4) + i0(+3), a2(-1) * a2(-1) - f0], 7): a PROGRAM constant as the factor, a negative
    rotation that wraps, and the short column Fixed(2)."""
    b = gp.Builder("three_terms", "hand-made: program-constant factor, three Horner steps")
    t0 = b.mul(gp._col("Advice", 0, 0), gp._col("Advice", 1, 1))
    t1 = b.add(gp._col("Fixed", 2, -1), gp._col("Instance", 0, 3))
    t2 = b.sub(b.square(gp._col("Advice", 2, -1)), gp._col("Fixed", 0, 0))
    b.horner(gp.PREV, [t0, t1, t2], gp.C_SEVEN)
    return b.finish()


def not_admitted() -> List[gp.Program]:
    """programs hm_graph_evaluate_circuits_dev must refuse, by the rule each one breaks"""
    out = []
    A0, A1, Y, BETA = gp._col("Advice", 0, 0), gp._col("Advice", 1, 1), ("Y",), ("Beta",)
    b = gp.Builder("previous_twice")
    t = b.add(gp.PREV, A0)
    b.horner(gp.PREV, [t], Y)
    out.append(b.finish())
    b = gp.Builder("previous_outside_the_chain")
    t = b.mul(gp.PREV, A0)
    b.horner(A1, [t], Y)
    out.append(b.finish())
    b = gp.Builder("previous_as_a_part")
    b.horner(A0, [gp.PREV], Y)
    out.append(b.finish())
    b = gp.Builder("two_factors")
    t = b.horner(gp.PREV, [A0], Y)
    b.horner(t, [A1], BETA)
    out.append(b.finish())
    b = gp.Builder("column_factor")
    b.horner(gp.PREV, [A0], A1)
    out.append(b.finish())
    b = gp.Builder("chain_not_last")
    t = b.horner(gp.PREV, [A0], Y)
    b.add(t, A1)
    out.append(b.finish())
    b = gp.Builder("no_previous")
    b.horner(A0, [A1], Y)
    out.append(b.finish())
    b = gp.Builder("store_of_previous")
    b.horner(gp.PREV, [], Y)
    out.append(b.finish())
    return out


def raw_chain_step_read_twice() -> np.ndarray:
    """five-word calculations: t0 = Prev * c1 + c0; t1 = t0 * t0; t2 = t0 * c1 + t1 -- PreviousValue is read once and starts the chain,
    but a step of the chain is read outside it, so the value is quadratic in PreviousValue"""
    inter = lambda i: (1 << 30) | i
    return np.array([[7, 3 << 30, 1, 0, 0], [2, inter(0), inter(0), 0, 1], [7, inter(0), 1, inter(1), 2]], dtype=np.uint32)


@dataclass
class Circuits:
    """m circuits of one program: data[c] is circuit c's inputs; the scalars and the short columns are those of data[0] for all; the
    columns listed in ``shared`` (table indices) too.  data[0].previous is the entry value."""
    data: List[gp.Data]
    shared: set

    @property
    def m(self):
        return len(self.data)


def make_circuits(seed: int, seg: int, segments: int, m: int, shared=(), all_shared: bool = False) -> Circuits:
    rng = random.Random(seed)
    first = gp.make_data(rng, seg, segments)
    n_cols = len(first.table)
    shared = set(range(n_cols)) if all_shared else set(gp.SHORT) | set(shared)
    data = [first]
    for _ in range(1, m):
        d = gp.make_data(rng, seg, segments)
        table = [first.table[i] if i in shared else d.table[i] for i in range(n_cols)]
        data.append(replace(first, table=table))
    return Circuits(data, shared)


def chained_oracle(p: gp.Program, cs: Circuits, rows=None) -> List[int]:
    """m successive evaluations chained through PreviousValue, by oracle/graph_ref: on all rows, or the listed ones -> their values"""
    d0 = cs.data[0]
    rows = list(range(d0.size)) if rows is None else list(rows)
    prev = {r: d0.previous[r] for r in rows}
    for d in cs.data:
        full = [prev.get(r, 0) for r in range(d0.size)]
        got = gp.oracle_rows(p, d, rows, full)
        prev = dict(zip(rows, got))
    return [prev[r] for r in rows]


def stacked_words(cs: Circuits, internal: bool, repeat_one_row: bool = True):
    """-> per column (word array, stride in u32 words): circuit c's column c * stride words behind the first; 0 for a shared one.
    repeat_one_row: a one-row column as the library reads it (two rows); False: as ``CompiledGraph`` takes it (one row)."""
    per = [gp.column_words(d, internal) for d in cs.data]
    out = []
    for i in range(len(per[0])):
        col0 = per[0][i]
        if repeat_one_row and i in gp.SHORT and gp.SHORT[i] == 0:
            col0 = np.repeat(col0, 2, axis=0)                      # as CompiledGraph passes a one-row column
        if i in cs.shared:
            out.append((col0, 0))
        else:
            out.append((np.ascontiguousarray(np.concatenate([per[c][i] for c in range(cs.m)])), col0.shape[0] * 8))
    return out


@dataclass
class FoldReplay:
    rc: int
    values: np.ndarray
    tracked_bound: np.ndarray
    fold_bound: np.ndarray         # partial as reduced, accumulator entering the product, sum before its reduction, accumulator stored
    error: str = ""


def hostcheck():
    hc = gp.hostcheck()
    hc.hc_graph_circuits_replay.restype = ctypes.c_int
    hc.hc_graph_linear_shape.restype = ctypes.c_int
    return hc


def host_linear_shape(hc, low):
    """graph_linear_shape of csrc/graph_lower.h on the arguments of hm_graph_create -> (factor source, steps) or the refusal's text"""
    calcs = np.ascontiguousarray(low["calcs"], dtype=np.uint32).reshape(-1, 5)
    out = np.zeros(2, dtype=np.uint32)
    rc = hc.hc_graph_linear_shape(calcs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(calcs.shape[0]),
                                  ctypes.c_size_t(len(low["constants"])), ctypes.c_size_t(low["n_dynamic"]), ctypes.c_size_t(len(low["rotations"])),
                                  ctypes.c_size_t(low["n_columns"]), ctypes.c_uint32(low["n_intermediates"]),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return (int(out[0]), int(out[1])) if rc == 0 else hc.hc_graph_last_error().decode()


def host_fold_replay(hc, p: gp.Program, cs: Circuits, internal: bool) -> FoldReplay:
    P32, P64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    low, d0 = p.lower(), cs.data[0]
    calcs = np.ascontiguousarray(low["calcs"], dtype=np.uint32).reshape(-1, 5)
    consts = gp.words(low["constants"])
    sc = d0.scalars()
    dyn = gp.words(list(sc["challenges"]) + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]])
    rots = np.array(list(low["rotations"]) or [0], dtype=np.int32)
    cols = stacked_words(cs, internal)
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c, _ in cols])
    strides = np.array([s for _, s in cols], dtype=np.uint64)
    rows = np.array([c.shape[0] if s == 0 else s // 8 for c, s in cols], dtype=np.uint64)
    values = gp.words(d0.previous).copy()
    tb, fb = np.zeros(max(calcs.shape[0], 1)), np.zeros(4)
    PD = ctypes.POINTER(ctypes.c_double)
    rc = hc.hc_graph_circuits_replay(calcs.ctypes.data_as(P32), ctypes.c_size_t(calcs.shape[0]), consts.ctypes.data_as(P64),
                                     ctypes.c_size_t(len(low["constants"])), dyn.ctypes.data_as(P64), ctypes.c_size_t(low["n_dynamic"]),
                                     rots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_size_t(len(low["rotations"])), ptrs,
                                     strides.ctypes.data_as(P64), rows.ctypes.data_as(P64), ctypes.c_size_t(low["n_columns"]), ctypes.c_size_t(cs.m),
                                     ctypes.c_uint32(low["n_intermediates"]), ctypes.c_uint32(d0.seg.bit_length() - 1), ctypes.c_uint32(d0.segments),
                                     ctypes.c_uint32(1 if internal else 0), values.ctypes.data_as(P32), tb.ctypes.data_as(PD), fb.ctypes.data_as(PD))
    return FoldReplay(rc, values, tb, fb, hc.hc_graph_last_error().decode() if rc == -1 else "")
