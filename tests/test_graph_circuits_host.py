"""CPU suite of hm_graph_evaluate_circuits_dev (several circuits of one constraint system folded in one launch):
the header and the binding have the entry; without a device it answers HM_ERR_NO_DEVICE; ``CompiledGraph.evaluate_circuits`` and the
library's own check (csrc/graph_lower.h: graph_linear_shape, through libhm_hostcheck.so) refuse every program that is not linear in
PreviousValue, and agree on every program of tests/graph_programs.py; the HM_BOUNDS host replay of the kernel's fold
(hc_graph_circuits_replay) equals the chain of single evaluations by oracle/graph_ref word for word and stays inside its classes.

The replays run in a child process: an HM_BOUNDS violation aborts the process, and the test reports the program instead."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_circuits_common as gc
import graph_programs as gp
from halo2_experiments_amd import _lib, evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "hm_graph_evaluate_circuits_dev"
SWEEP_SEEDS = range(7000, 7320)                  # the seeds of tests/test_graph_lowering_host.py


def admitted_programs():
    return [p for p in gp.hand_written() if gc.is_admitted(p)] + [gc.three_terms()] + \
           [p for p in (gp.random_program(s) for s in SWEEP_SEEDS) if gc.is_admitted(p)]


def test_header_and_binding_have_the_entry():
    text = open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()
    assert f"int {ENTRY}(uint64_t handle, const void* const* column_bases, const uint64_t* column_strides," in text
    fn = getattr(_lib.load(), ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    assert ENTRY in open(os.path.join(ROOT, "rust", "halo2-mi355x-sys", "src", "lib.rs")).read()


def test_without_a_device_the_entry_says_so():
    """null arguments are HM_ERR_BAD_ARG everywhere; with valid-looking (never dereferenced) arguments a box without a device gets
    HM_ERR_NO_DEVICE, and a box with one HM_ERR_NOT_FOUND for a handle nobody holds"""
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    values = ctypes.c_void_p(0x1000)
    assert fn(ctypes.c_uint64(1 << 40), None, None, 0, 1, None, 0, 3, 1, None, 0, None) == _lib.HM_ERR_BAD_ARG
    one = (ctypes.c_void_p * 1)(0x2000)
    assert fn(ctypes.c_uint64(1 << 40), one, None, 1, 1, None, 0, 3, 1, values, 0, None) == _lib.HM_ERR_BAD_ARG          # no strides
    rc = fn(ctypes.c_uint64(1 << 40), None, None, 0, 1, None, 0, 3, 1, values, 0, None)
    assert rc == (_lib.HM_ERR_NOT_FOUND if lib.hm_device_count() > 0 else _lib.HM_ERR_NO_DEVICE)


def _graph_with(calcs):
    """a CompiledGraph that was never uploaded: evaluate_circuits must refuse the program before it calls down"""
    g = ev.CompiledGraph.__new__(ev.CompiledGraph)
    g.calcs, g.handle = np.ascontiguousarray(calcs, dtype=np.uint32).reshape(-1, 5), 0
    return g


@pytest.mark.parametrize("p", gc.not_admitted(), ids=lambda p: p.name)
def test_evaluate_circuits_refuses_a_program_of_another_shape(p):
    with pytest.raises(ValueError, match="evaluate_circuits"):
        _graph_with(p.lower()["calcs"]).evaluate_circuits([], None, None, 2)
    assert isinstance(gc.host_linear_shape(gc.hostcheck(), p.lower()), str)


def test_a_chain_step_read_outside_the_chain_is_refused():
    calcs = gc.raw_chain_step_read_twice()
    with pytest.raises(ValueError, match="evaluate_circuits"):
        _graph_with(calcs).evaluate_circuits([], None, None, 2)
    low = dict(calcs=calcs, constants=[0, 1, 2], n_dynamic=0, rotations=[0], n_columns=1, n_intermediates=3)
    assert "outside the chain" in gc.host_linear_shape(gc.hostcheck(), low)


def test_the_library_and_the_binding_agree_on_every_program():
    """factor and step count where both admit, a refusal where either refuses: the hand-written list and the sweep's seeds"""
    hc = gc.hostcheck()
    programs = gp.hand_written() + [gc.three_terms()] + gc.not_admitted() + [gp.random_program(s) for s in SWEEP_SEEDS]
    admitted = 0
    for p in programs:
        low = p.lower()
        lib_says = gc.host_linear_shape(hc, low)
        try:
            py_says = ev.linear_in_previous(low["calcs"])
            admitted += 1
        except ValueError:
            py_says = None
        assert (lib_says == py_says) if py_says is not None else isinstance(lib_says, str), p.describe()
    assert admitted >= 20
    factor, steps = ev.linear_in_previous(gc.three_terms().lower()["calcs"])
    assert (factor, steps) == (gp.CONSTANTS.index(7), 3)                     # a program constant, three Horner steps


def child_main() -> None:
    emit = lambda s: print(s, flush=True)
    hc = gc.hostcheck()
    failures, worst = {}, [0.0] * 4
    for n, p in enumerate(admitted_programs()):
        n_calcs = len(p.lower()["calcs"])
        for seg, segments, m in ((2, 2, 3), (64, 1, 2)) if n_calcs <= 40 else ((2, 2, 3),):
            cs = gc.make_circuits(900 + n, seg, segments, m)
            want = gp.words(gc.chained_oracle(p, cs))
            for internal in (False, True):
                what = f"{p.name} seg={seg} segments={segments} circuits={m} {'internal' if internal else 'external'}"
                emit("BEGIN " + what)
                r = gc.host_fold_replay(hc, p, cs, internal)
                bad = []
                if r.rc != 0:
                    bad.append(f"{what}: hc_graph_circuits_replay returned {r.rc} {r.error}")
                elif not np.array_equal(r.values, want):
                    bad.append(f"{what}: the fold differs from the chain of single evaluations")
                worst = [max(a, float(b)) for a, b in zip(worst, r.fold_bound)]
                if bad:
                    failures.setdefault(p.name, []).extend(bad + [p.describe()])
    emit("RESULT " + json.dumps(dict(failures=failures, worst=worst, programs=len(admitted_programs()))))


@pytest.fixture(scope="module")
def fold():
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_graph_circuits_host as t; t.child_main()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    lines = r.stdout.splitlines()
    begun = [ln[6:] for ln in lines if ln.startswith("BEGIN ")]
    result = next((json.loads(ln[7:]) for ln in lines if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or result is None:
        return dict(aborted=begun[-1] if begun else "(before the first program)", returncode=r.returncode, stderr=r.stderr[-2000:])
    return result


def test_the_fold_replay_equals_the_chain_of_single_evaluations(fold):
    assert "aborted" not in fold, f"the replay process ended with {fold['returncode']} in: {fold['aborted']}\n{fold['stderr']}"
    assert fold["programs"] >= 20
    assert not fold["failures"], "\n".join(f"{k}:\n  " + "\n  ".join(v) for k, v in list(fold["failures"].items())[:5])


def test_the_fold_stays_inside_its_classes(fold):
    """ff29.h's classes, in units of r: a partial is reduced below 3 before it goes to LDS; the accumulator enters the product below 3
    (fe_mul takes < 18); product + partial is below 6 < GE_CAP, which ge_reduce accepts; what is stored is below 3 (fe_to_ext).  Every
    precondition of a primitive is checked by the HM_BOUNDS build itself: a violation aborts the child."""
    assert "aborted" not in fold, f"the replay process ended with {fold['returncode']} in: {fold['aborted']}\n{fold['stderr']}"
    partial, acc_in, total, acc_out = fold["worst"]
    assert 0 < partial <= 3.0 and 0 < acc_in <= 3.0 and 0 < total <= 6.0 and 0 < acc_out <= 3.0


if __name__ == "__main__":
    child_main()
