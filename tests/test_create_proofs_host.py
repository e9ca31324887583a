"""CPU suite of create_proofs and its three device entries: the header, the binding and the Rust sys file have
hm_graph_evaluate_proofs_dev, hm_fr_linear_combination_batch_dev and hm_shplonk_set_quotient_batch_bn256_fr_dev with the stated argument
counts; without a device they answer HM_ERR_BAD_ARG for nulls and HM_ERR_NO_DEVICE otherwise; the address rule of the proofs kernel
(csrc/graph_lower.h: graph_proofs_*, through libhm_hostcheck.so) equals a Python statement of it, on the wave-straddling case and the
stride-0 case; ``create_proofs`` refuses wrong arguments before any device call."""
import ctypes
import os
import types

import numpy as np
import pytest

import graph_programs as gp
import halo2_experiments_amd as h
from halo2_experiments_amd import _lib
from halo2_experiments_amd.domain import fr_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hm_graph_evaluate_proofs_dev": 13, "hm_fr_linear_combination_batch_dev": 7, "hm_shplonk_set_quotient_batch_bn256_fr_dev": 11}
_u64p = ctypes.POINTER(ctypes.c_uint64)


def test_header_binding_and_rust_have_the_entries():
    text = open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()
    rust = open(os.path.join(ROOT, "rust", "halo2-mi355x-sys", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, count in ENTRIES.items():
        assert f"int {name}(" in text, name
        fn = getattr(_lib.load(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == count, name
        assert f"pub fn {name}(" in rust and f"pub fn {name}(" in doc, name
    assert "void* d_values, uint64_t values_stride, uint32_t flags, void* stream);" in text
    assert hasattr(h, "create_proofs") and "create_proofs" in h.__all__


def test_without_a_device_the_entries_say_so():
    """null arguments are HM_ERR_BAD_ARG everywhere; with valid-looking (never dereferenced) arguments a box without a device gets
    HM_ERR_NO_DEVICE (a box with one: HM_ERR_NOT_FOUND for a handle nobody holds; nothing else is called there)"""
    lib = _lib.load()
    BAD, NO_DEVICE = _lib.HM_ERR_BAD_ARG, _lib.HM_ERR_NO_DEVICE
    has_device = lib.hm_device_count() > 0
    graph = lib.hm_graph_evaluate_proofs_dev
    values = ctypes.c_void_p(0x1000)
    assert graph(ctypes.c_uint64(1 << 40), None, None, 0, 1, None, 0, 3, 1, None, 64, 0, None) == BAD
    one = (ctypes.c_void_p * 1)(0x2000)
    assert graph(ctypes.c_uint64(1 << 40), one, None, 1, 1, None, 0, 3, 1, values, 64, 0, None) == BAD          # no strides
    rc = graph(ctypes.c_uint64(1 << 40), None, None, 0, 1, None, 0, 3, 1, values, 64, 0, None)
    assert rc == (_lib.HM_ERR_NOT_FOUND if has_device else NO_DEVICE)

    lc = lib.hm_fr_linear_combination_batch_dev
    w = np.stack([fr_words(3), fr_words(4)])
    assert lc(None, w.ctypes.data_as(_u64p), 1, 8, None, 2, None) == BAD
    polys = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    outs = (ctypes.c_void_p * 2)(0x4000, 0x5000)
    assert lc(polys, None, 1, 8, outs, 2, None) == BAD
    assert lc((ctypes.c_void_p * 2)(0x2000, None), w.ctypes.data_as(_u64p), 1, 8, outs, 2, None) == BAD
    assert lc(polys, w.ctypes.data_as(_u64p), 1, 8, (ctypes.c_void_p * 2)(0x4000, 0x4000), 2, None) == BAD       # one output twice
    assert lc(polys, w.ctypes.data_as(_u64p), 1, 8, (ctypes.c_void_p * 2)(0x3000, 0x5000), 2, None) == BAD       # proof 1's input
    if not has_device:
        assert lc(polys, w.ctypes.data_as(_u64p), 1, 8, outs, 2, None) == NO_DEVICE

    sq = lib.hm_shplonk_set_quotient_batch_bn256_fr_dev
    pts = np.stack([fr_words(5), fr_words(6)])
    sc = np.stack([fr_words(1), fr_words(1)])
    wp, pp, sp = w.ctypes.data_as(_u64p), pts.ctypes.data_as(_u64p), sc.ctypes.data_as(_u64p)
    assert sq(None, wp, 1, 8, pp, 1, sp, outs, 0, 2, None) == BAD
    assert sq(polys, wp, 1, 8, pp, 1, sp, None, 0, 2, None) == BAD
    assert sq(polys, wp, 1, 8, pp, 1, sp, outs, 0, 0, None) == BAD                                               # no proof
    assert sq(polys, wp, 0, 8, pp, 1, sp, outs, 0, 2, None) == BAD and sq(polys, wp, 1, 8, pp, 5, sp, outs, 0, 2, None) == BAD
    assert sq(polys, wp, 1, 1, pp, 1, sp, outs, 0, 2, None) == BAD                                               # n < t + 1
    same = np.stack([fr_words(5), fr_words(5)])
    assert sq(polys, wp, 2, 8, same.ctypes.data_as(_u64p), 2, sp, (ctypes.c_void_p * 1)(0x4000), 0, 1, None) == BAD   # two equal points
    assert sq(polys, wp, 1, 8, pp, 1, sp, (ctypes.c_void_p * 2)(0x4000, 0x4008), 0, 2, None) == BAD              # a misaligned output
    assert sq(polys, wp, 1, 8, pp, 1, sp, (ctypes.c_void_p * 2)(0x3000, 0x5000), 0, 2, None) == BAD              # proof 1's input
    if not has_device:
        assert sq(polys, wp, 1, 8, pp, 1, sp, outs, 0, 2, None) == NO_DEVICE


# ---- the address rule ---------------------------------------------------------------------------------------------------------------------
def python_address(lane, rows, log_segment, rotation, log_rows, stride_words, n_dynamic, word):
    """the rule as section 21 states it: rows run fastest; a rotation wraps inside its segment of its own proof, then inside a short
    column's period; proof b's cell lies b strides behind the base; its constants at b * n_dynamic * 9"""
    proof, row = divmod(lane, rows)
    seg = 1 << log_segment
    read = row - row % seg + (row % seg + rotation) % seg
    if log_rows:
        read %= 1 << log_rows
    return [proof, row, read, stride_words * proof + read * 8, proof * n_dynamic * 9 + word]


def library_address(hc, *args):
    out = np.zeros(5, dtype=np.uint64)
    lane, rows, log_segment, rotation, log_rows, stride, n_dynamic, word = args
    hc.hc_graph_proofs_address(ctypes.c_uint64(lane), ctypes.c_uint64(rows), ctypes.c_uint32(log_segment), ctypes.c_int64(rotation),
                               ctypes.c_uint32(log_rows), ctypes.c_uint64(stride), ctypes.c_uint32(n_dynamic), ctypes.c_uint32(word),
                               out.ctypes.data_as(_u64p))
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def hc():
    lib = gp.hostcheck()
    lib.hc_graph_proofs_address.restype = None
    return lib


def test_a_wave_that_straddles_proofs(hc):
    """16 rows a proof: the 64 lanes of wave 0 belong to proofs 0 .. 3, each with its own row of the constant table; a rotation past the
    last row of a proof comes back to that proof's first row"""
    rows, stride = 16, 16 * 8
    seen = set()
    for lane in range(5 * rows):
        for rotation in (0, 1, -1, 3, 300, -300):
            args = (lane, rows, 4, rotation, 0, stride, 6, 7)
            got = library_address(hc, *args)
            assert got == python_address(*args), args
            assert got[3] // stride == lane // rows and got[4] == (lane // rows) * 54 + 7        # never another proof's cell or constant
        seen.add(library_address(hc, lane, rows, 4, 0, 0, stride, 6, 0)[0])
    assert seen == {0, 1, 2, 3, 4}
    assert library_address(hc, 2 * rows - 1, rows, 4, 1, 0, stride, 6, 0)[2:4] == [0, stride]       # proof 1's last row + 1 -> its row 0


def test_a_shared_column_and_the_other_shapes(hc):
    for lane in (0, 5, 63, 64, 1023, 1024, 3 * 1024 + 17):
        args = (lane, 1024, 9, -2, 0, 0, 16, 143)                           # stride 0: the same cells for every proof; two segments
        got = library_address(hc, *args)
        assert got == python_address(*args) and got[3] == got[2] * 8
        args = (lane, 1024, 9, 3, 2, 0, 4, 0)                               # a short column of four rows
        assert library_address(hc, *args) == python_address(*args) and library_address(hc, *args)[2] < 4
    big = (1 << 32) - 1                                                     # the last lane the entry admits
    for args in ((big, 1 << 32, 30, 1, 0, 0, 1, 0), (big, 1 << 31, 30, -1, 0, 1 << 34, 16, 143), (big, 1, 0, 5, 0, 8, 2, 17)):
        assert library_address(hc, *args) == python_address(*args), args


# ---- create_proofs refuses before any device call -------------------------------------------------------------------------------------
def fake_keys(num_advice=2, k=3):
    """what create_proofs reads before it touches the device: the shapes"""
    cs = types.SimpleNamespace(num_advice=num_advice)
    vk = types.SimpleNamespace(cs=cs, domain=types.SimpleNamespace(k=k))
    return types.SimpleNamespace(k=k), types.SimpleNamespace(vk=vk)


def test_create_proofs_checks_its_arguments_before_any_device_call():
    import torch
    params, pk = fake_keys()
    adv = torch.zeros((3, 2, 8, 4), dtype=torch.int64)                        # on the host
    inst = [[1], [2], [3]]
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(params, pk, adv, inst, [5, 6, 5])
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(params, pk, adv, inst, [5, 6, 5 + (3 << 48)])
    with pytest.raises(ValueError, match="seed"):
        h.create_proofs(params, pk, adv, inst, [5, 6])
    with pytest.raises(ValueError, match="instance"):
        h.create_proofs(params, pk, adv, inst[:2], 5)
    with pytest.raises(ValueError, match="advice"):
        h.create_proofs(params, pk, adv[0], inst[:1], 5)
    with pytest.raises(ValueError, match="advice"):
        h.create_proofs(params, pk, "advice", inst, 5)
    with pytest.raises(ValueError, match="proof"):
        h.create_proofs(params, pk, [], [], [])
    with pytest.raises(ValueError, match="GPU tensor"):
        h.create_proofs(params, pk, adv, inst, 5)                             # a CPU tensor
    with pytest.raises(ValueError, match="differ in k"):
        h.create_proofs(types.SimpleNamespace(k=4), pk, adv, inst, 5)
