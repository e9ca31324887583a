"""All KZG openings of a polynomial on its domain on the MI355X (hm_kzg_open_table_bn256_dev / hm_kzg_open_all_bn256_dev;
halo2_experiments_amd/openings.py).

open_all is compared word for word with the independent route open_at (eval_polynomial, kate_division, one MSM per point), at the small
sizes also with the closed form pi_i = [(f(s) - f(w^i)) / (s - w^i)]G in Python integers (the tests know s).  Sizes: sub-wave grids
(log_n 0 .. 3), the first size whose 2n transform runs a lane-uniform stage (log_n = 6), the first whose n transform does (7),
several 64-thread blocks (8, 10)."""
import ctypes
import random

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, openings as op
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, FR_MODULUS as R, fr_array, fr_ints, fr_words, g1_ints, g1_words
from halo2_experiments_amd.kzg import ParamsKZG
from halo2_experiments_amd.pairing import G1_GEN, g1_mul

pytestmark = pytest.mark.gpu

S = 0x2B5C1F0E3D4A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF % R
_PARAMS = {}


def params_for(k):
    """setup(k, S, keep_points=True), one per size for the whole module (k = 0 rides on the parameters of k = 1)"""
    kk = max(k, 1)
    if kk not in _PARAMS:
        _PARAMS[kk] = ParamsKZG.setup(kk, S, keep_points=True)
    return _PARAMS[kk]


def _to_dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to("cuda")


def _to_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _poly_ints(ints):
    return _to_dev(fr_array([int(v) % R for v in ints]))


def _by_open_at(params, poly, k):
    """(n, 8) words: every proof by the one-at-a-time route"""
    w = op.domain_omega(k)
    return np.stack([op.open_at(params, poly, pow(w, i, R))[1] for i in range(1 << k)])


def _closed_form(f, k):
    w = op.domain_omega(k)
    ev = lambda z: sum(c * pow(z, j, R) for j, c in enumerate(f)) % R
    fs = ev(S)
    return np.stack([g1_words(g1_mul((fs - ev(pow(w, i, R))) * pow(S - pow(w, i, R), -1, R) % R, G1_GEN)) for i in range(len(f))])


@pytest.mark.parametrize("log_n", [1, 3, 7])
def test_table_is_the_fft_of_the_arranged_points(log_n):
    params = params_for(log_n)
    table = op.OpeningTable(params, log_n)
    assert table is op.OpeningTable(params, log_n) and table.table.shape == (2 << log_n, 8)       # kept on the params object
    x = op.arrange_points(params.g_points, log_n)
    h.g1_fft(x, fr_words(op.domain_omega(log_n + 1)), log_n + 1)
    assert np.array_equal(_to_np(table.table), _to_np(x))


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6, 7, 8])
def test_every_proof_equals_the_one_at_a_time_route(log_n):
    n = 1 << log_n
    params = params_for(log_n)
    poly = h.random_fr(n, 100 + log_n, "cuda")
    got = _to_np(op.open_all(params, poly))
    assert got.shape == (n, 8)
    assert np.array_equal(got, _by_open_at(params, poly, log_n))
    if n <= 64:
        assert np.array_equal(got, _closed_form(fr_ints(_to_np(poly)), log_n))


def test_log_n_10_against_the_batched_quotients():
    k, n = 10, 1 << 10
    params = params_for(k)
    poly = h.random_fr(n, 77, "cuda")
    got = _to_np(op.open_all(params, poly))
    rng = random.Random(3)
    idx = sorted({0, 1, n // 2, n - 1} | set(rng.sample(range(n), 68)))
    assert len(idx) >= 64
    w = op.domain_omega(k)
    quotients = h.kate_division_batch([poly] * len(idx), [fr_words(pow(w, i, R)) for i in idx])
    exp = h.best_multiexp_batch(quotients, params.g_handle)
    assert exp[:, 8:].any(axis=1).all()                                       # no quotient of a random polynomial commits to the identity
    assert np.array_equal(got[idx], exp[:, :8])


@pytest.mark.parametrize("log_n", [3, 7])
def test_shaped_polynomials(log_n):
    n = 1 << log_n
    params = params_for(log_n)
    unit = lambda j, c=1: [c if i == j else 0 for i in range(n)]
    zeros = np.zeros((n, 8), dtype=np.uint64)
    assert np.array_equal(_to_np(op.open_all(params, _poly_ints([0] * n))), zeros)                # the zero polynomial
    assert np.array_equal(_to_np(op.open_all(params, _poly_ints(unit(0, 12345)))), zeros)         # a constant: f_0 never enters
    g0 = _to_np(params.g_points)[0]
    assert np.array_equal(g0, g1_words(G1_GEN))
    assert np.array_equal(_to_np(op.open_all(params, _poly_ints(unit(1)))), np.tile(g0, (n, 1)))  # f = X: every proof is g_0
    # X^(n-1): slot y_0 of the circulant and the identity in h_(n-1); X (above, vs open_at here) and X^(n-2): the two ends of the
    # wrapped tail; every coefficient r - 1: the scalar conversion at the top of the field
    for ints in (unit(n - 1), unit(1, 3), unit(n - 2), [R - 1] * n):
        poly = _poly_ints(ints)
        got = _to_np(op.open_all(params, poly))
        assert np.array_equal(got, _by_open_at(params, poly, log_n)), ints[:4]
        if n <= 64:
            assert np.array_equal(got, _closed_form(ints, log_n))
        assert got.any(axis=1).all()                                          # none of these proofs is the identity


def test_a_stack_equals_single_calls():
    import torch
    k, n = 6, 64
    params = params_for(k)
    stack = h.random_fr(3 * n, 9, "cuda", shape=(3, n, 4))
    got = op.open_all(params, stack)
    assert got.shape == (3, n, 8)
    for p in range(3):
        assert torch.equal(got[p], op.open_all(params, stack[p].contiguous()))
    assert not torch.equal(got[0], got[1])


def test_lagrange_form_equals_coefficient_form_and_keeps_its_input():
    import torch
    k, n = 7, 128
    params = params_for(k)
    coeffs = h.random_fr(n, 21, "cuda")
    evals = coeffs.clone()
    h.best_fft(evals, fr_words(op.domain_omega(k)), k)                       # the evaluations on the domain
    before = evals.clone()
    got = op.open_all(params, evals, form="lagrange")
    assert torch.equal(evals, before)
    assert torch.equal(got, op.open_all(params, coeffs))


@pytest.fixture(scope="module")
def opened():
    """log_n = 6: the polynomial, its commitment, evaluations and proofs"""
    k, n = 6, 64
    params = params_for(k)
    poly = h.random_fr(n, 55, "cuda")
    evals = poly.clone()
    h.best_fft(evals, fr_words(op.domain_omega(k)), k)
    return dict(k=k, n=n, params=params, poly=poly, commitment=params.commit(poly), values=fr_ints(_to_np(evals)),
                proofs=op.open_all(params, poly))


def test_verify_opening(opened):
    params, c, w = opened["params"], opened["commitment"], op.domain_omega(opened["k"])
    proofs = _to_np(opened["proofs"])
    for i in (0, 37):
        assert op.verify_opening(params, c, pow(w, i, R), opened["values"][i], proofs[i])
    assert not op.verify_opening(params, c, w, opened["values"][1], proofs[2])
    total, proof0 = op.open_at(params, opened["poly"], 0)                    # z = 0: n f(0) is the sum of the column
    assert total * opened["n"] % R == sum(opened["values"]) % R
    assert op.verify_opening(params, c, 0, total, proof0)


def test_verify_openings_with_one_pairing(opened):
    params, c, n = opened["params"], opened["commitment"], opened["n"]
    idx, values, proofs = list(range(n)), list(opened["values"]), opened["proofs"]
    assert op.verify_openings(params, c, idx, values, proofs, seed=b"openings")
    wrong = list(values)
    wrong[17] = (wrong[17] + 1) % R
    assert not op.verify_openings(params, c, idx, wrong, proofs, seed=b"openings")
    swapped = proofs.clone()
    swapped[[3, 40]] = proofs[[40, 3]]
    assert not op.verify_openings(params, c, idx, values, swapped, seed=b"openings")
    x, y = g1_ints(_to_np(proofs)[9])
    off = proofs.clone()
    off[9] = _to_dev(g1_words((x, (y + 1) % P))).reshape(8)
    assert not op.verify_openings(params, c, idx, values, off, seed=b"openings")                  # a point off the curve
    assert op.verify_openings(params, c, [5, 9], [values[5], values[9]], proofs[[5, 9]].contiguous())   # a subset, fresh weights


def test_errors():
    import torch
    params = params_for(3)
    bare = ParamsKZG.setup(3, S)
    with pytest.raises(ValueError, match="not kept"):
        op.open_all(bare, h.random_fr(8, 1, "cuda"))
    bare.release()
    with pytest.raises(ValueError, match="0 .. 23"):
        op.OpeningTable(params, 24)
    with pytest.raises(ValueError, match="longer"):
        op.open_all(params, h.random_fr(16, 1, "cuda"))
    with pytest.raises(ValueError, match="power of two"):
        op.open_all(params, h.random_fr(6, 1, "cuda"))
    with pytest.raises(ValueError, match="form"):
        op.open_all(params, h.random_fr(8, 1, "cuda"), form="extended")
    with pytest.raises(TypeError):
        op.open_all(params, np.zeros((8, 4), dtype=np.uint64))
    lib = _lib.load()
    t = torch.zeros((16, 8), dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    assert lib.hm_kzg_open_table_bn256_dev(vp(params.g_points), 24, vp(t), st) == -1 and b"log_n > 23" in lib.hm_last_error()
    assert lib.hm_kzg_open_all_bn256_dev(vp(t), vp(params.g_points), 24, 1, vp(t), st) == -1
    assert lib.hm_kzg_open_all_bn256_dev(vp(t), vp(params.g_points), 3, 1, vp(t), st) == -1 and b"overlap" in lib.hm_last_error()
