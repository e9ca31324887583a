"""The graph evaluator's host side without a GPU: csrc/graph_lower.h's ``graph_check_call`` and ``graph_launch_plan``, the two pure
functions the one driver (graph.hip: graph_run) asks before it takes a stream slot, through libhm_hostcheck.so.

* the plan against a Python restatement of the three formulas it replaced -- the ``blocks`` / ``log_c`` / ``b_scratch`` passages of
  graph_evaluate, graph_evaluate_circuits and graph_evaluate_proofs and mock.hip's mock_blocks, as they stood before graph_run --
  over kind x log_size 0..30 x segments {1, 2, 5, 8} x units {1, 2, 3, 4, 7, 64, 65, 2^20} x n_slots {0, 1, 37} x max_blocks
  {1, 5, 1280}, restricted to the shapes the check admits;
* the invariants of every such row;
* the refusal table: every row tests/test_graph_circuits_gpu.py and tests/test_graph_proofs_gpu.py send that this check decides
  (null arrays and unknown handles are the C entry's, a program that is not linear is graph_linear_shape's:
  tests/test_graph_circuits_host.py), the single kind's rows, and the order in which two broken rules are reported;
* the same sweep in a stand-alone program (tests/graph_plan_host.cpp) built with AddressSanitizer and UBSan."""
import ctypes
import itertools
import os
import subprocess

import pytest

import graph_programs as gp
from halo2_experiments_amd import _lib

SINGLE, CIRCUITS, PROOFS = 0, 1, 2
KINDS = {"single": SINGLE, "circuits": CIRCUITS, "proofs": PROOFS}
LOG_SIZES = range(31)
SEGMENTS = (1, 2, 5, 8)
UNITS = (1, 2, 3, 4, 7, 64, 65, 1 << 20)
N_SLOTS = (0, 1, 37)
MAX_BLOCKS = (1, 5, 1280)
N_DYN = 6
# the argument blocks as the kernels read them: 256 pointers, (256 strides,) 16 x 9 constant words, (9 fold words,) the counts;
# a struct with pointers is a multiple of 8 bytes
SIZEOF_COLUMNS = (256 * 8 + 16 * 9 * 4 + 4 + 7) // 8 * 8
SIZEOF_CIRCUIT_COLUMNS = 256 * 8 + 256 * 8 + 16 * 9 * 4 + 9 * 4 + 4
SIZEOF_PROOF_COLUMNS = 256 * 8 + 256 * 8 + 2 * 4
BASE = 0x7F0000001000              # an aligned address; nothing is ever read through it


@pytest.fixture(scope="module")
def hc():
    lib = gp.hostcheck()
    lib.hc_graph_check_call.restype = ctypes.c_char_p
    lib.hc_graph_launch_plan.restype = None
    return lib


def check(hc, kind, n_columns=6, units=1, n_dyn=N_DYN, log_size=6, segments=1, flags=0, values=BASE, values_stride=0, bases=None, strides=None,
          program_columns=6, program_dynamic=N_DYN):
    """-> None for an admitted call, else the reason"""
    bases = [BASE + 0x1000 * (i + 1) for i in range(n_columns)] if bases is None else bases
    if strides is None and kind != SINGLE:
        strides = [0] * n_columns
    ba = (ctypes.c_uint64 * max(len(bases), 1))(*bases)
    sa = None if strides is None else (ctypes.c_uint64 * max(len(strides), 1))(*strides)
    why = hc.hc_graph_check_call(kind, ctypes.c_uint64(n_columns), ctypes.c_uint64(units), ctypes.c_uint64(n_dyn), log_size, segments, flags,
                                 ctypes.c_uint64(values), ctypes.c_uint64(values_stride), ba, sa, ctypes.c_uint64(program_columns),
                                 ctypes.c_uint64(program_dynamic))
    return None if why is None else why.decode()


def plan(hc, kind, size, units, n_slots, n_dyn, max_blocks):
    out = (ctypes.c_uint64 * 8)()
    hc.hc_graph_launch_plan(kind, ctypes.c_uint64(size), ctypes.c_uint64(units), n_slots, ctypes.c_uint64(n_dyn), max_blocks, out)
    return dict(zip(("size", "lanes", "blocks", "T", "log_c", "rows_per", "scratch_bytes", "args_bytes"), out))


def before_graph_run(kind, size, units, n_slots, n_dyn, max_blocks):
    """(blocks, log_c, scratch bytes, argument bytes) as the three drivers computed them, each in its own words"""
    if kind == SINGLE:
        blocks = min((size + 255) // 256, max_blocks)
        return blocks, 0, n_slots * 9 * (blocks * 256) * 4, SIZEOF_COLUMNS
    if kind == CIRCUITS:
        log_c = 0
        while log_c < 8 and (1 << log_c) < units and ((size << log_c) + 255) // 256 < max_blocks:
            log_c += 1
        rows_per = 256 >> log_c
        blocks = min((size + rows_per - 1) // rows_per, max_blocks)
        return blocks, log_c, n_slots * 9 * (blocks * 256) * 4, SIZEOF_CIRCUIT_COLUMNS
    lanes = units * size
    blocks = min((lanes + 255) // 256, max_blocks)
    return blocks, 0, n_slots * 9 * (blocks * 256) * 4, (SIZEOF_PROOF_COLUMNS // 4 + max(units * n_dyn, 1) * 9) * 4


def mock_blocks_before(lanes, max_blocks):
    return min((lanes + 255) // 256, max(max_blocks, 1))


def admitted_shapes(hc, kind):
    for log_size, segments, units in itertools.product(LOG_SIZES, SEGMENTS, (1,) if kind == SINGLE else UNITS):
        if check(hc, kind, units=units, log_size=log_size, segments=segments, values_stride=(segments << log_size) * 8) is None:
            yield segments << log_size, units


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_plan_is_the_three_formulas_and_keeps_its_invariants(hc, kind):
    k = KINDS[kind]
    shapes = list(admitted_shapes(hc, k))
    # what the check leaves of the sweep: rows <= 2^32 and units * rows <= 2^32
    assert len(shapes) == sum(1 for ls, s, u in itertools.product(LOG_SIZES, SEGMENTS, (1,) if k == SINGLE else UNITS)
                              if (s << ls) <= 1 << 32 and u * (s << ls) <= 1 << 32) > 100
    for (size, units), n_slots, max_blocks in itertools.product(shapes, N_SLOTS, MAX_BLOCKS):
        p = plan(hc, k, size, units, n_slots, N_DYN, max_blocks)
        row = (kind, size, units, n_slots, max_blocks, p)
        assert (p["blocks"], p["log_c"], p["scratch_bytes"], p["args_bytes"]) == before_graph_run(k, size, units, n_slots, N_DYN, max_blocks), row
        assert p["size"] == size and 1 <= p["blocks"] <= max_blocks and p["T"] == 256 * p["blocks"], row
        assert p["blocks"] * 256 >= min(p["lanes"], 256 * max_blocks), row
        assert p["rows_per"] << p["log_c"] == 256 and p["log_c"] <= 8 and (1 << p["log_c"]) < 2 * units, row
        assert p["lanes"] == (units * size if k == PROOFS else size << p["log_c"]), row
        if k != CIRCUITS:
            assert p["log_c"] == 0, row
        if units == 1:                                         # one circuit, one proof: the single kind's grid
            single = plan(hc, SINGLE, size, 1, n_slots, N_DYN, max_blocks)
            assert [p[f] for f in ("lanes", "blocks", "T", "log_c", "rows_per", "scratch_bytes")] == \
                   [single[f] for f in ("lanes", "blocks", "T", "log_c", "rows_per", "scratch_bytes")], row
        if k == SINGLE:                                        # the witness checker's grid (mock.hip: mock_blocks)
            assert p["blocks"] == mock_blocks_before(size, max_blocks), row


def test_the_argument_block_follows_the_constants(hc):
    for units, n_dyn in [(1, 0), (1, 6), (3, 0), (3, 16), (81, 6)]:
        assert plan(hc, PROOFS, 64, units, 1, n_dyn, 1280)["args_bytes"] == SIZEOF_PROOF_COLUMNS + max(units * n_dyn, 1) * 36
        assert plan(hc, CIRCUITS, 64, units, 1, n_dyn, 1280)["args_bytes"] == SIZEOF_CIRCUIT_COLUMNS
    assert plan(hc, SINGLE, 64, 1, 1, 16, 1280)["args_bytes"] == SIZEOF_COLUMNS


def refused(why, text):
    assert why is not None and why.startswith("graph:") and text in why, why
    return True


def test_what_the_circuits_suite_sends(hc):
    """tests/test_graph_circuits_gpu.py: test_argument_errors_launch_nothing, 64 rows, 2 circuits"""
    def call(**kw):
        return check(hc, CIRCUITS, **dict(dict(units=2, strides=[0, 0, 0, 512, 512, 512]), **kw))

    assert call() is None
    assert refused(call(units=0), "circuits must be >= 1")
    assert refused(call(n_columns=257, bases=[BASE] * 257, strides=[0] * 257), "more columns than the column table holds")
    assert refused(call(bases=[BASE + 8] + [BASE] * 5), "a column base is not 16-byte aligned")
    assert refused(call(strides=[0, 0, 0, 64 * 8 + 2, 512, 512]), "a column stride is not a multiple of 4 words")
    assert refused(call(units=(1 << 32) // 64 + 1), "circuits * rows > 2^32")
    assert refused(call(units=(1 << 26) + 1, log_size=6, segments=1), "circuits * rows > 2^32")
    assert refused(call(n_columns=5, strides=[0] * 5), "another number of columns")
    assert refused(call(n_dyn=N_DYN - 1), "another number of per-call constants")
    assert refused(call(flags=2), "unknown flag") and refused(call(segments=0), "segments must be >= 1")
    assert call(units=(1 << 32) // 64) is None and call(flags=1) is None


def test_what_the_proofs_suite_sends(hc):
    """tests/test_graph_proofs_gpu.py: test_argument_errors_launch_nothing, 64 rows, 2 proofs; test_one_proof_equals_the_single_entry"""
    size = 64

    def call(**kw):
        return check(hc, PROOFS, **dict(dict(units=2, values_stride=size * 8, strides=[0, 0, 0, 512, 512, 512]), **kw))

    assert call() is None
    assert refused(call(units=0), "proofs must be >= 1")
    for vstride in (size * 8 - 4, 0, size * 8 + 2):
        assert refused(call(values_stride=vstride), "the values stride must be a multiple of 4 words and hold the rows of one proof")
    assert refused(call(n_columns=257, bases=[BASE] * 257, strides=[0] * 257), "more columns than the column table holds")
    assert refused(call(bases=[BASE + 8] + [BASE] * 5), "a column base is not 16-byte aligned")
    assert refused(call(values=BASE + 8), "the values are not 16-byte aligned")
    assert refused(call(strides=[0, 0, 0, size * 8 + 2, 512, 512]), "a column stride is not a multiple of 4 words")
    assert refused(call(units=(1 << 32) // 64 + 1), "proofs * rows > 2^32")
    assert refused(call(n_columns=5, strides=[0] * 5), "another number of columns")
    assert refused(call(n_dyn=N_DYN - 1), "another number of per-call constants")
    assert refused(call(flags=2), "unknown flag") and refused(call(segments=0), "segments must be >= 1")
    assert refused(call(log_size=31), "log_size > 30")
    assert call(units=1, values_stride=0, strides=[0] * 6) is None          # one proof: the stride is not read
    assert call(values_stride=size * 8 + 4) is None                          # values inside a wider tensor


def test_the_single_kind_is_held_to_the_same_alignment(hc):
    """tests/test_graph_programs_gpu.py: the single entries' refusals; the two alignment rows are what this entry used to let through"""
    def call(**kw):
        return check(hc, SINGLE, **kw)

    assert call() is None and call(segments=8, log_size=3, flags=1) is None
    assert refused(call(values=BASE + 8), "the values are not 16-byte aligned")
    assert refused(call(bases=[BASE] * 3 + [BASE + 8] + [BASE] * 2), "a column base is not 16-byte aligned")
    assert refused(call(bases=[BASE] * 5 + [0]), "null column pointer")
    assert refused(call(flags=2), "unknown flag") and refused(call(segments=0), "segments must be >= 1")
    assert refused(call(log_size=31), "log_size > 30")
    assert refused(call(n_columns=5), "another number of columns") and refused(call(n_columns=7), "another number of columns")
    assert refused(call(n_dyn=N_DYN + 1), "another number of per-call constants")
    assert refused(call(log_size=30, segments=8), "rows <= 2^32") and call(log_size=30, segments=4) is None
    # a program of 256 columns is the table's limit; the single kind names a 257th column as a wrong count, as it always has
    assert refused(call(n_columns=257, bases=[BASE] * 257, program_columns=256), "another number of columns")


@pytest.mark.parametrize("kind", list(KINDS))
def test_two_broken_rules_are_reported_in_the_entries_order(hc, kind):
    """flag, units, table size, column count, constant count, log_size, rows, units * rows, values, values stride, then column by column
    null, base, stride"""
    k = KINDS[kind]
    worst = dict(flags=2, units=0, n_columns=257, bases=[BASE + 8] * 257, strides=[2] * 257, n_dyn=N_DYN + 1, log_size=31, segments=0, values=BASE + 8,
                 values_stride=2)
    order = [("flags", 0, "unknown flag"), ("units", 2, "must be >= 1"), ("n_columns", 6, "more columns than the column table holds")]
    if k == SINGLE:
        worst.update(units=1, strides=None)
        order = [order[0], ("n_columns", 6, "another number of columns")]
    order += [("n_dyn", N_DYN, "per-call constants"), ("log_size", 6, "log_size > 30"), ("segments", 1, "segments must be >= 1")]
    if k == PROOFS:
        order += [("values", BASE, "values are not 16-byte aligned"), ("values_stride", 512, "values stride"), ("bases", None, "column base")]
    else:
        order += [("values", BASE, "values are not 16-byte aligned"), ("bases", None, "column base")]
    if k != SINGLE:
        order += [("strides", None, "column stride")]
    call = dict(worst)
    for field, good, text in order:
        assert refused(check(hc, k, **call), text), (field, call)
        if field == "n_columns":
            call.update(n_columns=good, bases=[BASE + 8] * good, strides=None if k == SINGLE else [2] * good)
        elif field == "bases":
            call["bases"] = [BASE] * 6
        elif field == "strides":
            call["strides"] = [0] * 6
        else:
            call[field] = good
    assert check(hc, k, **call) is None
    if k != SINGLE:                                            # units * rows comes after the rows themselves and before the values
        assert refused(check(hc, k, units=1 << 27, values=BASE + 8, strides=[0] * 6), "* rows > 2^32")
        assert refused(check(hc, k, units=1 << 27, segments=0, strides=[0] * 6), "segments must be >= 1")


def test_the_sweep_under_the_sanitizers(hc, tmp_path):
    """tests/graph_plan_host.cpp walks column tables of exactly n_columns entries and asserts the invariants itself; its row count and
    checksum are those of this file's sweep through libhm_hostcheck.so"""
    exe = str(tmp_path / "graph_plan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", _lib.CSRC, os.path.join(os.path.dirname(os.path.abspath(__file__)), "graph_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr[-2000:])
    rows = refused = total = 0
    for k in KINDS.values():
        swept = list(itertools.product(LOG_SIZES, SEGMENTS, (1,) if k == SINGLE else UNITS))
        shapes = list(admitted_shapes(hc, k))
        refused += len(swept) - len(shapes)
        for (size, units), n_slots, max_blocks in itertools.product(shapes, N_SLOTS, MAX_BLOCKS):
            p = plan(hc, k, size, units, n_slots, N_DYN, max_blocks)
            rows += 1
            total += p["blocks"] + 3 * p["log_c"] + 5 * p["lanes"] + 7 * p["scratch_bytes"] + 11 * p["args_bytes"]
    assert r.stdout.split() == ["rows", str(rows), "refused", str(refused), "checksum", str(total % (1 << 64))]
