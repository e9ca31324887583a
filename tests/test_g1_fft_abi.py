"""CPU checks of best_fft over G1: the two entry points are exported and bound, their argument checks answer before any device is
needed, and the drop-in's try_best_fft routes bn256::G1 to the host form."""
import ctypes
import os
import re

import numpy as np
import pytest

from halo2_experiments_amd import _lib
import halo2_experiments_amd as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_ERR_BAD_ARG = -1


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def test_both_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hm_g1_fft_bn256_dev", "hm_g1_fft_bn256"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["hm_g1_fft_bn256_dev"][1]) == 5 and len(_lib._SIGNATURES["hm_g1_fft_bn256"][1]) == 4


def test_argument_errors_come_before_the_device():
    lib = _lib.load()
    w = np.zeros(4, dtype=np.uint64)
    pts = np.zeros((2, 12), dtype=np.uint64)
    assert lib.hm_g1_fft_bn256_dev(None, _u64(w), 1, None, None) == HM_ERR_BAD_ARG
    assert b"null" in lib.hm_last_error()
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(0x1000), None, 1, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(0x1000), _u64(w), 25, None, None) == HM_ERR_BAD_ARG
    assert b"log_n > 24" in lib.hm_last_error()
    assert lib.hm_g1_fft_bn256(None, _u64(w), 1, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_fft_bn256(_u64(pts), None, 1, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_fft_bn256(_u64(pts), _u64(w), 25, None) == HM_ERR_BAD_ARG
    assert b"log_n > 24" in lib.hm_last_error()
    assert pts.sum() == 0


def test_no_device_means_error_not_fallback():
    lib = _lib.load()
    if lib.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    w = np.zeros(4, dtype=np.uint64)
    pts = np.zeros((2, 12), dtype=np.uint64)
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(0x1000), _u64(w), 1, None, None) == -2     # never dereferenced
    with pytest.raises(_lib.Halo2Mi355xError) as e:
        h.g1_fft_host(pts, w, 1)
    assert e.value.code == -2


def test_python_mirror_checks_its_arguments():
    w = np.zeros(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="1 << log_n"):
        h.g1_fft_host(np.zeros((3, 12), dtype=np.uint64), w, 1)
    with pytest.raises(TypeError):
        h.g1_fft_host([[0] * 12], w, 0)
    with pytest.raises(TypeError):
        h.g1_fft(np.zeros((2, 8), dtype=np.uint64), w, 1)
    with pytest.raises(ValueError, match="one field element"):
        h.g1_fft_host(np.zeros((2, 12), dtype=np.uint64), np.zeros(8, dtype=np.uint64), 1)


def test_try_best_fft_routes_g1_to_the_host_form():
    glue = open(os.path.join(ROOT, "rust", "halo2_proofs-patch", "src", "mi355x.rs")).read()
    body = glue[glue.index("pub fn try_best_fft<"):]
    body = body[:body.index("\n}\n")]
    assert "TypeId::of::<G1>()" in body
    g1 = glue[glue.index("fn try_best_fft_g1<"):]
    g1 = g1[:g1.index("\n}\n")]
    assert "sys::hm_g1_fft_bn256(" in g1 and "HM_ERR_PARTIAL_OUTPUT" in g1 and "g1_from_words" in g1
    assert re.search(r"pub const GPU_MIN_LOG_N_G1_FFT: u32 = \d+;", glue)
    assert "hm_g1_fft_bn256" in open(os.path.join(ROOT, "rust", "halo2_proofs.patch")).read()
