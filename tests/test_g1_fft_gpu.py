"""best_fft over BN256 G1 on the MI355X (hm_g1_fft_bn256_dev / hm_g1_fft_bn256; g_to_lagrange, ParamsKZG.from_monomial / downsize).

Small sizes are checked point by point against an EC-DFT written here from the oracle's affine group law; large sizes through known
discrete logs (fixed-base [d_j]G, so that the FFT of the points is the fixed-base image of the Fr NTT of d); the KZG identities through
the trapdoor setup, which derives g_lagrange from the scalars instead."""
import ctypes
import random

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib
from halo2_experiments_amd.arithmetic import FQ_ONE_MONT, G1_GENERATOR
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words
from oracle import bn256_ref as o

pytestmark = pytest.mark.gpu

P = o.P
G = (1, 2)
HM_ERR_BAD_ARG, HM_ERR_INTERNAL = -1, -5


def _to_dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to("cuda")


def _to_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _ec_fft(a, w):
    """Recursive radix-2 EC-DFT: out[i] = sum_j [w^(ij)] a[j] (None = identity)."""
    n = len(a)
    if n == 1:
        return list(a)
    ev, od = _ec_fft(a[0::2], w * w % R), _ec_fft(a[1::2], w * w % R)
    out = [None] * n
    t = 1
    for k in range(n // 2):
        m = o.g1_mul(t, od[k])
        out[k] = o.g1_add(ev[k], m)
        out[k + n // 2] = o.g1_add(ev[k], o.g1_neg(m))
        t = t * w % R
    return out


def _ec_dft_naive(a, w):
    n = len(a)
    out = []
    for i in range(n):
        acc = None
        for j in range(n):
            acc = o.g1_add(acc, o.g1_mul(pow(w, i * j, R), a[j]))
        out.append(acc)
    return out


def test_the_oracle_fft_is_the_dft():
    rng = random.Random(5)
    pts = [o.g1_mul(rng.randrange(R), G) for _ in range(8)]
    pts[3] = None
    for log_n in range(4):
        n = 1 << log_n
        w = o.fr_omega(log_n)
        assert _ec_fft(pts[:n], w) == _ec_dft_naive(pts[:n], w)


@pytest.mark.parametrize("variant", ["plain", "scaled"])
def test_small_sizes_against_the_oracle(variant):
    rng = random.Random(11 if variant == "plain" else 12)
    for log_n in range(8):
        n = 1 << log_n
        pts = [o.g1_mul(rng.randrange(1, R), G) for _ in range(n)]
        for j in rng.sample(range(n), max(1, n // 8)):
            pts[j] = None                                          # planted identities
        if n >= 4:
            pts[1] = pts[0]                                        # a repeated point
            pts[2] = o.g1_neg(pts[0])                              # and its negative
        # not the default root: its inverse (plain) or its cube (scaled), both of order exactly n
        w = pow(o.fr_omega(log_n), -1, R) if variant == "plain" else pow(o.fr_omega(log_n), 3, R)
        exp = _ec_fft(pts, w)
        scale = None
        if variant == "scaled":
            scale = rng.randrange(R)
            exp = [o.g1_mul(scale, p) for p in exp]
        t = _to_dev(o.g1_affine_array(pts))
        h.g1_fft(t, fr_words(w), log_n, None if scale is None else fr_words(scale))
        got = _to_np(t)
        assert np.array_equal(got, o.g1_affine_array(exp)), (variant, log_n)


def _fr_rows(t, rows):
    return o.fr_from_array(_to_np(t[rows]))


def _plant(d, k):
    """Exceptional cases in the scalars: zeros (identity points), and a duplicate and a negative across first-stage pairs (i, i + n/2:
    twiddle 1, so those butterflies double and cancel).  The last stage's doubling / cancelling pair is
    test_a_butterfly_that_doubles_and_one_that_cancels."""
    import torch
    n, half = 1 << k, 1 << (k - 1)
    a, b = _fr_rows(d, [0, 1])
    for idx, v in {3: 0, 4: 0, n - 1: 0, 5: a, half + 5: a, 6: b, half + 6: (R - b) % R, 7: a, 8: a}.items():
        d[idx] = torch.from_numpy(o.fr_array([v]).view(np.int64)[0]).to(d.device)


@pytest.mark.parametrize("k", [12, 16, 20, 24])
def test_known_discrete_logs(k):
    n = 1 << k
    d = h.random_fr(n, 1000 + k)
    w = o.fr_omega(k) if k != 16 else pow(o.fr_omega(k), -1, R)
    _plant(d, k)
    pts = h.g1_fixed_base_mul(d, G1_GENERATOR)
    dh = d.clone()
    h.best_fft(dh, fr_words(w), k)
    exp = h.g1_fixed_base_mul(dh, G1_GENERATOR)
    h.g1_fft(pts, fr_words(w), k)
    assert np.array_equal(_to_np(pts), _to_np(exp))


@pytest.mark.parametrize("k", [12, 16])
def test_a_butterfly_that_doubles_and_one_that_cancels(k):
    """d = (a, omega^-j a, 0, ...): output i is [a + omega^(i-j) a]G, so the last stage's butterfly j adds
    [a]G to itself (output j: doubling) and to its negative (output j + n/2: the identity)."""
    import torch
    n = 1 << k
    w = o.fr_omega(k)
    rng = random.Random(77 + k)
    a, j = rng.randrange(1, R), rng.randrange(1, n // 2)
    d = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d[:2] = _to_dev(o.fr_array([a, a * pow(w, n - j, R) % R]))
    pts = h.g1_fixed_base_mul(d, G1_GENERATOR)
    dh = d.clone()
    h.best_fft(dh, fr_words(w), k)
    exp = h.g1_fixed_base_mul(dh, G1_GENERATOR)
    h.g1_fft(pts, fr_words(w), k)
    got = _to_np(pts)
    assert np.array_equal(got, _to_np(exp))
    assert not got[j + n // 2].any() and got[j].any()


def test_round_trip_at_the_largest_size():
    k = 24
    n = 1 << k
    d = h.random_fr(n, 4242)
    pts = h.g1_fixed_base_mul(d, G1_GENERATOR)
    before = _to_np(pts).copy()
    w = o.fr_omega(k)
    h.g1_fft(pts, fr_words(w), k)
    h.g1_fft(pts, fr_words(pow(w, -1, R)), k, fr_words(pow(n, -1, R)))
    assert np.array_equal(_to_np(pts), before)


def _jacobian_host(aff, rng, zero_rows):
    """(n, 8) affine words -> (n, 12) Jacobian (lambda^2 x, lambda^3 y, lambda z) with random lambda; z = 0 rows are identities."""
    n = aff.shape[0]
    out = np.zeros((n, 12), dtype=np.uint64)
    mont, rinv = 1 << 256, pow(1 << 256, -1, P)
    for i in range(n):
        if i in zero_rows or not aff[i].any():
            out[i, 0:4] = o.to_limbs(rng.randrange(P) * mont % P)     # garbage x, y under z = 0
            out[i, 4:8] = o.to_limbs(rng.randrange(P) * mont % P)
            continue
        x = o.from_limbs(aff[i, :4]) * rinv % P
        y = o.from_limbs(aff[i, 4:]) * rinv % P
        lam = rng.randrange(2, P)
        out[i, 0:4] = o.to_limbs(x * lam * lam % P * mont % P)
        out[i, 4:8] = o.to_limbs(y * lam * lam * lam % P * mont % P)
        out[i, 8:12] = o.to_limbs(lam * mont % P)
    return out


def _expected_jacobian(aff):
    out = np.zeros((aff.shape[0], 12), dtype=np.uint64)
    live = aff.any(axis=1)
    out[live, :8] = aff[live]
    out[live, 8:] = FQ_ONE_MONT
    return out


def test_host_form_matches_the_device_form():
    k = 14
    n = 1 << k
    rng = random.Random(14)
    d = h.random_fr(n, 1400)
    aff = _to_np(h.g1_fixed_base_mul(d, G1_GENERATOR)).copy()
    zero_rows = set(rng.sample(range(n), 40))
    aff[sorted(zero_rows)] = 0
    xyz = _jacobian_host(aff, rng, zero_rows)
    w, sc = fr_words(o.fr_omega(k)), fr_words(rng.randrange(R))
    t = _to_dev(aff)
    h.g1_fft(t, w, k, sc)
    h.g1_fft_host(xyz, w, k, sc)
    assert np.array_equal(xyz, _expected_jacobian(_to_np(t)))


def test_host_form_leaves_the_array_untouched_on_an_early_fault():
    fi = _lib.load_fi()
    k = 8
    d = h.random_fr(1 << k, 88)
    aff = _to_np(h.g1_fixed_base_mul(d, G1_GENERATOR)).copy()
    xyz = _jacobian_host(aff, random.Random(8), set())
    want = xyz.copy()
    w = fr_words(o.fr_omega(k))
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    try:
        for point in (b"g1_fft_upload", b"g1_fft_download"):
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_g1_fft_bn256(p(xyz), p(w), k, None) == HM_ERR_INTERNAL
            assert point in fi.hm_last_error() and np.array_equal(xyz, want)
        fi.hm_test_arm_fault(None, 0)
        assert fi.hm_g1_fft_bn256(p(xyz), p(w), k, None) == 0
    finally:
        fi.hm_test_arm_fault(None, 0)
    t = _to_dev(aff)
    h.g1_fft(t, w, k)
    assert np.array_equal(xyz, _expected_jacobian(_to_np(t)))


def test_errors_then_a_valid_call():
    import torch
    lib = _lib.load()
    w = fr_words(o.fr_omega(3))
    t = _to_dev(o.g1_affine_array([o.g1_mul(i + 1, G) for i in range(8)]))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(t.data_ptr()), p(w), 25, None, st) == HM_ERR_BAD_ARG
    assert b"log_n > 24" in lib.hm_last_error()
    assert lib.hm_g1_fft_bn256_dev(None, p(w), 3, None, st) == HM_ERR_BAD_ARG and b"null" in lib.hm_last_error()
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(t.data_ptr()), None, 3, None, st) == HM_ERR_BAD_ARG
    assert lib.hm_g1_fft_bn256(None, p(w), 3, None) == HM_ERR_BAD_ARG
    exp = _ec_fft([o.g1_mul(i + 1, G) for i in range(8)], o.fr_omega(3))
    assert lib.hm_g1_fft_bn256_dev(ctypes.c_void_p(t.data_ptr()), p(w), 3, None, st) == 0
    assert np.array_equal(_to_np(t), o.g1_affine_array(exp))


# ---- the KZG parameters ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 18])
def test_g_to_lagrange_reproduces_the_trapdoor_setup(k):
    from halo2_experiments_amd.kzg import ParamsKZG
    s = random.Random(k).randrange(2, R)
    params = ParamsKZG.setup(k, s, keep_points=True)
    try:
        got = h.g_to_lagrange(params.g_points, k)
        assert np.array_equal(_to_np(got), _to_np(params.g_lagrange_points))
    finally:
        params.release()


def test_downsize_and_from_monomial():
    from halo2_experiments_amd.kzg import ParamsKZG
    s = 0x1234567890ABCDEF1234567890ABCDEF % R
    big = ParamsKZG.setup(20, s, keep_points=True)
    ref = ParamsKZG.setup(18, s, keep_points=True)
    mono = None
    try:
        big.downsize(18)
        assert big.k == 18 and big.n == 1 << 18 and len(big.g_lagrange_handle) == 1 << 18
        assert np.array_equal(_to_np(big.g_lagrange_points), _to_np(ref.g_lagrange_points))
        assert np.array_equal(_to_np(big.g_points), _to_np(ref.g_points))
        mono = ParamsKZG.from_monomial(18, ref.g_points, ref.g2, ref.s_g2)
        v = h.random_fr(1 << 18, 1818)
        want = ref.commit_lagrange(v)
        assert want.any() and np.array_equal(mono.commit_lagrange(v), want) and np.array_equal(big.commit_lagrange(v), want)
        assert np.array_equal(mono.commit(v), ref.commit(v))
    finally:
        for p in (big, ref, mono):
            if p is not None:
                p.release()


def _pcie_bytes():
    st = _lib.Stats()
    _lib.check(_lib.load().hm_get_stats(ctypes.byref(st)))
    return np.array([st.h2d_bytes, st.d2h_bytes], dtype=np.int64)


def test_host_form_counts_the_bytes_it_moves():
    """hm_get_stats' h2d_bytes / d2h_bytes of hm_g1_fft_bn256 at 2^2 points: 96 bytes per point each way."""
    rng = random.Random(22)
    aff = _to_np(h.g1_fixed_base_mul(h.random_fr(4, 22), G1_GENERATOR))
    xyz = _jacobian_host(aff, rng, ())
    dev = _to_dev(aff.copy())
    w = fr_words(o.fr_omega(2))
    h.g1_fft(dev, w, 2)
    b0 = _pcie_bytes()
    h.g1_fft_host(xyz, w, 2)
    assert (_pcie_bytes() - b0).tolist() == [4 * 96, 4 * 96]
    assert np.array_equal(xyz, _expected_jacobian(_to_np(dev)))
