"""keygen's permutation assembly, the parts that need no GPU: the exports, ``copy_pairs``, the C ABI's argument checks, and the assembly's
key packing and link rule (keygen.inc's ``perm_key`` / ``perm_link``, the arithmetic its kernels run) built for the host, over a
host-sorted key list and a sequential union-find, against ``synthesis.permutation_cells``.  Every comparison is exact."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import keygen_cases as kc
from halo2_experiments_amd import _lib, keygen, synthesis as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_ERR_BAD_ARG, HM_ERR_NO_DEVICE = -1, -2
NEW_ENTRIES = ("hm_permutation_assemble_dev", "hm_permutation_columns_bn256_fr_dev")
_u32p, _u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


def _u32(a, offset=0):
    return ctypes.cast(ctypes.c_void_p(a.ctypes.data + offset), _u32p)


def test_package_exports_the_feature():
    import halo2_experiments_amd as h
    for name in ("copy_pairs", "permutation_cells_dev", "permutation_columns_dev", "keygen_vk", "keygen_pk", "VerifyingKey", "ProvingKey"):
        assert name in h.__all__ and getattr(h, name) is getattr(keygen, name)
    header = open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib._SIGNATURES and hasattr(_lib.load(), name) and hasattr(_lib.load_fi(), name)
        assert f"int {name}(" in header
    assert keygen.FR_DELTA == pow(7, 1 << 28, keygen.R)


def test_copy_pairs_are_the_layouts_copies_as_cell_ids():
    for name, cs, lay in kc.real_layouts():
        pairs = keygen.copy_pairs(cs, lay)
        copies = lay.copies()
        assert pairs.dtype == np.uint32 and pairs.shape == (len(copies), 2) and len(copies) > 0, name
        index = {col: j for j, col in enumerate(cs.equality)}
        for (a, b), ((ka, ca, ra), (kb, cb, rb)) in zip(pairs.tolist(), copies):
            assert (a, b) == (index[(ka, ca)] * lay.n + ra, index[(kb, cb)] * lay.n + rb), name


def test_copy_pairs_rejects_a_column_without_equality():
    name, cs, lay = kc.real_layouts()[2]
    narrowed = SimpleNamespace(equality=cs.equality[1:])
    with pytest.raises(ValueError) as twin:
        sy.permutation_cells(narrowed, lay)
    with pytest.raises(ValueError) as got:
        keygen.copy_pairs(narrowed, lay)
    assert str(got.value) == str(twin.value) and "a column without equality" in str(got.value)


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    assert hasattr(lib, "hc_permutation_assemble")
    lib.hc_permutation_assemble.argtypes = [_u32p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p]
    return lib


def host_assemble(hc, pairs, P, k):
    arr = np.ascontiguousarray(np.array(pairs, dtype=np.uint32).reshape(-1, 2))
    out = np.full((P << k) + 1, 0xDEADBEEF, dtype=np.uint32)
    dropped = np.full(1, 77, dtype=np.uint32)
    assert hc.hc_permutation_assemble(_u32(arr), arr.shape[0], P, k, _u32(out), _u32(dropped)) == 0
    assert out[P << k] == 0xDEADBEEF
    return out[:P << k].tolist(), int(dropped[0])


def test_the_kernels_rule_on_the_host_equals_permutation_cells_on_the_real_layouts(hc):
    for name, cs, lay in kc.real_layouts():
        P, n = len(cs.equality), lay.n
        got, dropped = host_assemble(hc, keygen.copy_pairs(cs, lay), P, lay.k)
        exp = [j * n + i for col in sy.permutation_cells(cs, lay) for (j, i) in col]
        assert got == exp and dropped == 0, name
        assert sum(1 for c, s in enumerate(got) if s != c) > 0, name


@pytest.mark.parametrize("name,pairs", kc.small_sets(), ids=[n for n, _ in kc.small_sets()])
def test_the_kernels_rule_on_the_host_equals_permutation_cells_on_small_sets(hc, name, pairs):
    got, dropped = host_assemble(hc, pairs, 3, 4)
    assert got == kc.twin_cells(pairs, 3, 4) and dropped == 0
    assert sorted(got) == list(range(48))                                          # a permutation of the cells
    assert host_assemble(hc, pairs[::-1], 3, 4)[0] == got                          # the order of the copies does not matter
    assert host_assemble(hc, [(b, a) for a, b in pairs], 3, 4)[0] == got           # nor the order inside a pair


def test_the_host_build_drops_and_counts_pairs_out_of_range(hc):
    pairs = [(1, 2), (48, 3), (2, 40), (7, 1 << 31), (0xFFFFFFFF, 0xFFFFFFFF), (5, 5)]
    got, dropped = host_assemble(hc, pairs, 3, 4)
    assert dropped == 3 and got == kc.twin_cells([(1, 2), (2, 40), (5, 5)], 3, 4)
    assert hc.hc_permutation_assemble(None, 0, 0, 4, None, None) != 0 and hc.hc_permutation_assemble(None, 0, 3, 31, None, None) != 0


def _aligned(nbytes):
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + nbytes]


def test_bad_arguments_are_reported_before_anything_else():
    """host buffers throughout: every call here is refused by the argument checks, so nothing can be launched on them"""
    lib = _lib.load()
    copies, cells, dropped, out, w = _aligned(64), _aligned(48 * 4), _aligned(64), _aligned(48 * 32), _aligned(64)
    ok = dict(copies=_u32(copies), m=4, columns=3, k=4, cells=_u32(cells), dropped=_u32(dropped))

    def assemble(**kw):
        a = dict(ok, **kw)
        return lib.hm_permutation_assemble_dev(a["copies"], a["m"], a["columns"], a["k"], a["cells"], a["dropped"], None)
    assert assemble(copies=None) == HM_ERR_BAD_ARG and b"null" in lib.hm_last_error()
    assert assemble(cells=None) == HM_ERR_BAD_ARG
    assert assemble(cells=None, m=0, copies=None) == HM_ERR_BAD_ARG                  # m = 0 still writes the identity
    assert assemble(columns=0) == HM_ERR_BAD_ARG and b"columns" in lib.hm_last_error()
    assert assemble(columns=3, k=31) == HM_ERR_BAD_ARG and b"2^32" in lib.hm_last_error()
    assert assemble(columns=1, k=33) == HM_ERR_BAD_ARG
    assert assemble(columns=(1 << 28) + 1, k=4) == HM_ERR_BAD_ARG
    assert assemble(m=(1 << 30) + 1) == HM_ERR_BAD_ARG and b"2^31" in lib.hm_last_error()
    assert assemble(copies=_u32(copies, 4)) == HM_ERR_BAD_ARG and b"aligned" in lib.hm_last_error()
    assert assemble(cells=_u32(cells, 2)) == HM_ERR_BAD_ARG
    assert assemble(dropped=_u32(dropped, 1)) == HM_ERR_BAD_ARG
    assert assemble(copies=_u32(cells, 8)) == HM_ERR_BAD_ARG and b"overlaps" in lib.hm_last_error()

    okc = dict(cells=_u32(cells), columns=3, k=4, omega=w.ctypes.data_as(_u64p), delta=w.ctypes.data_as(_u64p), out=ctypes.c_void_p(out.ctypes.data))

    def columns(**kw):
        a = dict(okc, **kw)
        return lib.hm_permutation_columns_bn256_fr_dev(a["cells"], a["columns"], a["k"], a["omega"], a["delta"], a["out"], None)
    for name in ("cells", "omega", "delta", "out"):
        assert columns(**{name: None}) == HM_ERR_BAD_ARG and b"null" in lib.hm_last_error(), name
    assert columns(columns=0) == HM_ERR_BAD_ARG
    assert columns(columns=5, k=30) == HM_ERR_BAD_ARG and b"2^32" in lib.hm_last_error()
    assert columns(out=ctypes.c_void_p(out.ctypes.data + 8)) == HM_ERR_BAD_ARG and b"aligned" in lib.hm_last_error()
    assert columns(cells=_u32(cells, 2)) == HM_ERR_BAD_ARG
    assert columns(cells=_u32(out, 16)) == HM_ERR_BAD_ARG and b"overlaps" in lib.hm_last_error()


def test_the_wrapper_validates_a_host_list_before_anything_is_uploaded():
    with pytest.raises(ValueError):
        keygen.permutation_cells_dev([(0, 48)], 3, 4)
    with pytest.raises(ValueError):
        keygen.permutation_cells_dev([(-1, 2)], 3, 4)
    with pytest.raises(ValueError):
        keygen.permutation_cells_dev([(0, 1)], 0, 4)
    with pytest.raises(ValueError):
        keygen.permutation_cells_dev([(0, 1)], 5, 30)
