"""CPU checks of the KZG openings (halo2_experiments_amd/openings.py, csrc/g1_fft.hip): the integer twin's two routes against
the closed form for a known s, the argument checks of the entry points before any device is needed, and verify_opening on proofs
made with integers."""
import ctypes

import pytest

from halo2_experiments_amd import _lib, openings as op
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, FR_MODULUS as R, g1_words
from halo2_experiments_amd.kzg import g2_bytes, g2_mul, G2_GENERATOR
from halo2_experiments_amd.pairing import G1_GEN, g1_mul

S = 0x1234567890ABCDEF1234567 % R


def _coeffs(n, salt=1):
    return [pow(7 + salt, 3 * j + 1, R) * (j + 2) % R for j in range(n)]


def _closed_form(f, s, k):
    """pi_i = [(f(s) - f(w^i)) / (s - w^i)]G"""
    w = op.domain_omega(k)
    ev = lambda z: sum(c * pow(z, j, R) for j, c in enumerate(f)) % R
    return [g1_mul((ev(s) - ev(pow(w, i, R))) * pow(s - pow(w, i, R), -1, R) % R, G1_GEN) for i in range(len(f))]


@pytest.mark.parametrize("n", [2, 4, 8])
def test_circulant_route_equals_definition_equals_closed_form(n):
    k = n.bit_length() - 1
    g = [g1_mul(pow(S, i, R), G1_GEN) for i in range(n)]
    f = _coeffs(n)
    by_def = op.open_all_ints(g, f, route="definition")
    by_circ = op.open_all_ints(g, f, route="circulant")
    assert by_def == by_circ == _closed_form(f, S, k)
    assert all(p is not None for p in by_def)


def test_integer_twin_edge_polynomials():
    n, k = 4, 2
    g = [g1_mul(pow(S, i, R), G1_GEN) for i in range(n)]
    for route in ("definition", "circulant"):
        assert op.open_all_ints(g, [5, 0, 0, 0], route=route) == [None] * n                     # a constant: f_0 never enters
        assert op.open_all_ints(g, [9, 1, 0, 0], route=route) == [G1_GEN] * n                   # f = X: every proof is g_0
        assert op.open_all_ints(g, [0, 0, 0, 1], route=route) == _closed_form([0, 0, 0, 1], S, k)   # X^(n-1): y_0 and h_(n-1)
        assert op.open_all_ints([G1_GEN], [3], route=route) == [None]                           # n = 1
    with pytest.raises(ValueError):
        op.open_all_ints(g, [1, 2, 3])
    with pytest.raises(ValueError):
        op.open_all_ints(g, [1, 2, 3, 4], route="other")


def test_entry_points_check_their_arguments_before_the_device():
    lib = _lib.load()
    a, b, c = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), ctypes.c_void_p(0x300000)
    assert lib.hm_kzg_open_table_bn256_dev(None, 3, b, None) == -1 and b"null" in lib.hm_last_error()
    assert lib.hm_kzg_open_table_bn256_dev(a, 3, None, None) == -1
    assert lib.hm_kzg_open_table_bn256_dev(a, 24, b, None) == -1 and b"log_n > 23" in lib.hm_last_error()
    assert lib.hm_kzg_open_table_bn256_dev(a, 3, ctypes.c_void_p(0x100000 + 64 * 8 - 64), None) == -1       # the table overlaps the points
    assert b"overlaps" in lib.hm_last_error()
    assert lib.hm_kzg_open_all_bn256_dev(None, b, 3, 1, c, None) == -1 and b"null" in lib.hm_last_error()
    assert lib.hm_kzg_open_all_bn256_dev(a, None, 3, 1, c, None) == -1
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 3, 1, None, None) == -1
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 24, 1, c, None) == -1 and b"log_n > 23" in lib.hm_last_error()
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 3, 65536, c, None) == -1
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 3, 1, ctypes.c_void_p(0x100000 + 128 * 8 - 64), None) == -1  # the proofs overlap the table
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 3, 2, ctypes.c_void_p(0x200000 + 2 * 32 * 8 - 32), None) == -1  # ... the coefficients
    assert b"overlap" in lib.hm_last_error()
    ms = (ctypes.c_double * 7)()
    assert lib.hm_kzg_open_all_timed_bn256_dev(a, b, 3, 1, c, None, None) == -1
    assert lib.hm_kzg_open_all_timed_bn256_dev(a, b, 24, 1, c, ms, None) == -1


def test_no_device_means_error_not_fallback():
    lib = _lib.load()
    if lib.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    a, b, c = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), ctypes.c_void_p(0x300000)      # never dereferenced
    assert lib.hm_kzg_open_table_bn256_dev(a, 3, b, None) == -2
    assert lib.hm_kzg_open_all_bn256_dev(a, b, 3, 1, c, None) == -2
    assert lib.hm_kzg_open_all_timed_bn256_dev(a, b, 3, 1, c, (ctypes.c_double * 7)(), None) == -2


class _Params:
    """what verify_opening reads of a ParamsKZG"""

    def __init__(self, s):
        self.g2, self.s_g2 = g2_bytes(G2_GENERATOR), g2_bytes(g2_mul(s))


def test_verify_opening_on_integer_made_proofs():
    n, k = 4, 2
    g = [g1_mul(pow(S, i, R), G1_GEN) for i in range(n)]
    f = _coeffs(n, salt=3)
    proofs = op.open_all_ints(g, f)
    w = op.domain_omega(k)
    ev = lambda z: sum(c * pow(z, j, R) for j, c in enumerate(f)) % R
    commitment = g1_mul(ev(S), G1_GEN)
    params = _Params(S)
    z1 = pow(w, 1, R)
    assert op.verify_opening(params, commitment, z1, ev(z1), proofs[1])
    assert not op.verify_opening(params, commitment, z1, (ev(z1) + 1) % R, proofs[1])            # another value
    assert not op.verify_opening(params, commitment, z1, ev(z1), proofs[2])                      # the proof of another index
    assert not op.verify_opening(params, commitment, z1, ev(z1), (proofs[1][0], (proofs[1][1] + 1) % P))   # a point off the curve
    assert op.verify_opening(params, g1_words(commitment), z1, ev(z1), g1_words(proofs[1]))      # the same from affine words
