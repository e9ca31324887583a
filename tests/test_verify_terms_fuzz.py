"""The two phases of the batch verifier's terms kernel on the host, under bound tracking (``hc_verify_terms``: a violated bound aborts the
process), on the records of tests/verify_terms_cases.py: about 150 records per constraint system, k and instance shape -- random, edge
values, degenerate and flagged, degenerate and exact.  The numerator is the twin's; every record ends flagged exactly where
``terms_from_challenges`` raises ``MalformedProof``, and every other record gives the twin's words; phase a leaves the record's limbs
canonical (``hc_verify_terms_record``), which no output word can show.  The kernel itself, with the numerator
program around the same two phases, meets the same records in tests/test_verify_terms_fuzz_gpu.py; this file keeps the case list alive
where there is no device."""
import ctypes

import numpy as np
import pytest

from halo2_experiments_amd import _lib
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array, fr_ints

import verify_terms_cases as vt

SEED, TOTAL = 20241, 150


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.hc_verify_terms.restype = ctypes.c_int
    lib.hc_verify_terms.argtypes = [u32p, ctypes.c_size_t, ctypes.c_size_t] + [u32p] * 9 + [ctypes.POINTER(ctypes.c_char_p)]
    return lib


def terms_on_the_host(hc, plan, lay, record, evals, inst_row, numerator):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    w = lambda values: np.ascontiguousarray(fr_array(values)).view(np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    rec, ev_, iw, num = w(record), w(evals), w(inst_row), w([numerator])
    vals, own = np.zeros((plan.n_vals, 8), dtype=np.uint32), np.zeros((lay.own_points, 8), dtype=np.uint32)
    shared, h2r, h2l = np.zeros((len(lay.shared_keys), 8), dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    why = ctypes.c_char_p()
    rc = hc.hc_verify_terms(p(plan.words), len(plan.words), plan.n_columns, p(rec), p(ev_), p(iw), p(num), p(vals), p(own), p(shared), p(h2r),
                            p(h2l), ctypes.byref(why))
    ints = lambda a: fr_ints(a.view(np.uint64))
    return rc, why.value, ints(own), ints(shared), ints(h2r)[0], ints(h2l)[0]


def test_the_edge_values_are_the_ones_named():
    assert len(vt.EDGE) == len(set(vt.EDGE)) == 15 and all(0 <= v < R for v in vt.EDGE)
    assert vt.EDGE[-2] * 2 ** 261 % R == 1 and vt.EDGE[-1] * 2 ** 256 % R == 1 and {0, R - 1, 2 ** 261 % R} <= set(vt.EDGE)


@pytest.mark.parametrize("config", list(vt.CONFIGS))
def test_the_classes_hold_what_they_promise(config):
    s = vt.setup(config)
    lay, first = s.layout, s.layout.sets[0][0]
    judged = vt.judged(config, SEED, TOTAL)                                    # asserts the flags class by class
    labels = [case[0] for case, _, _ in judged]
    assert len(labels) == len(set(labels)) == TOTAL
    count = lambda letter: sum(label[0] == letter for label in labels)
    outside = len(lay.super_rotations) - len(first)
    assert count("C") == 2 * (6 + outside) and count("D") == len(first) + 9 and count("A") >= 40 and count("B") >= 40
    for (label, ch, rb, evals, inst), scalars, _ in judged:
        assert len(evals) == lay.n_scalars and [len(c) for c in inst] == [s.rows] * s.cs.num_instance
        assert all(0 <= v < R for v in list(ch.values()) + [rb] + evals + [v for c in inst for v in c])
        if label.startswith("D:u=x"):
            assert scalars[0][-1] == 0                                          # u on a point of the first set: the scalar of [h] is zero
        if label == "D:rb=0":
            assert scalars == ([0] * lay.own_points, [0] * len(lay.shared_keys), 0, 0)
    assert any(label == "B:evals=0" for label in labels) and any(label == "B:evals=r-1" for label in labels)


@pytest.mark.parametrize("config", ["poseidon_k3_rows1", "merkle_sum_k9_rows1", "overflow_v2_k5_rows0"])
def test_phase_a_keeps_the_record_canonical(hc, config):
    """The interpreter reads beta, gamma, theta and y from the lane's workspace as constants, which it takes for canonical, so phase a
    must leave the record's limbs below r -- not merely below 3r like everything else it keeps.  The conversion's Montgomery product
    alone does not: it leaves 2^-261 mod r, whose internal form is 1, as r + 1 (the one value of EDGE it does this to; none of 2 000
    uniform values).  No output word shows the difference -- every later step accepts values below 3r, and a kernel without the
    canonical step passes the device test on those very lanes -- so the limbs themselves are read here."""
    s = vt.setup(config)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    hc.hc_verify_terms_record.restype = ctypes.c_int
    hc.hc_verify_terms_record.argtypes = [u32p, ctypes.c_size_t, ctypes.c_size_t] + [u32p] * 4
    w = lambda values: np.ascontiguousarray(fr_array(values)).view(np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    (_, ch, rb, evals, inst), _, _ = vt.judged(config, SEED, TOTAL)[0]
    ev_, iw = w(evals), w(s.plan.instance_row(inst))
    records = [[e] * 9 for e in vt.EDGE] + [[ch[name] for name in vt.bvm.RECORD] + [rb]]
    records += [[vt.EDGE[(i + j) % len(vt.EDGE)] for j in range(9)] for i in range(len(vt.EDGE))]
    for record in records:
        limbs = np.zeros(81, dtype=np.uint32)
        rc = hc.hc_verify_terms_record(p(s.plan.words), len(s.plan.words), s.plan.n_columns, p(w(record)), p(ev_), p(iw), p(limbs))
        assert rc in (0, 1)
        assert int(limbs.max()) < 1 << 29
        got = [sum(int(l) << (29 * i) for i, l in enumerate(limbs[9 * j:9 * j + 9])) for j in range(9)]
        assert got == [v * (1 << 261) % R for v in record], record


@pytest.mark.parametrize("config", list(vt.CONFIGS))
def test_the_phases_agree_with_the_twin_record_by_record(hc, config):
    s = vt.setup(config)
    flagged = exact = 0
    for (label, ch, rb, evals, inst), scalars, numerator in vt.judged(config, SEED, TOTAL):
        record = [ch[name] for name in vt.bvm.RECORD] + [rb]
        rc, why, own, shared, h2r, h2l = terms_on_the_host(hc, s.plan, s.layout, record, evals, s.plan.instance_row(inst),
                                                           5 if numerator is None else numerator)
        assert why is None, (label, why)
        if scalars is None:
            assert rc == 0, label                                               # flagged, and no bound violated on the way
            flagged += 1
        else:
            assert rc == 1, label
            assert (own, shared, h2r, h2l) == scalars, label
            exact += 1
    assert flagged >= 14 and exact >= 100
