"""GPU suite: the lockstep Montgomery products of csrc/ff29.h where they run -- g1x_madd_fast<true> inside accumulate_chain, in the
table MSM's bucket accumulation kernel -- against the C oracle, on ordinary and on adversarial inputs: every base equal, bases in
P / -P pairs (the equal-x exit into the general law), scalars 0, 1 and r - 1.  And the neighbours that share the header but keep
the single products: msm_small (the same accumulate_chain, single form), best_fft in one and in two passes, batch inversion.
Small sizes: the products are the same at every size, what varies is which kernel calls them."""
import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib
from conftest import g1_equal

pytestmark = pytest.mark.gpu

N_TABLE, N_PLAIN = 1 << 12, 1 << 10
KINDS = ["uniform", "equal_bases", "plus_minus_pairs", "edge_scalars"]


def rand_fr_gpu(n, seed):
    from halo2_experiments_amd.arithmetic import random_fr
    return random_fr(n, seed, "cuda")                 # uniform over the whole of [0, r)


def _negated(pyref, bases_host):
    """(n, 8) uint64 affine points in Montgomery words -> the same points with y -> p - y (also a Montgomery word)."""
    out = bases_host.copy()
    for i in range(out.shape[0]):
        y = pyref.from_limbs(out[i, 4:8])
        out[i, 4:8] = pyref.to_limbs((pyref.P - y) % pyref.P)
    return out


@pytest.fixture(scope="module")
def cases(cref, pyref):
    """{(kind, n): (scalars on the GPU, bases on the GPU, the oracle's affine result)}, computed once."""
    import torch
    out = {}
    edge = cref.fr_to_mont(np.array([pyref.to_limbs(0), pyref.to_limbs(1), pyref.to_limbs(pyref.R - 1)], dtype=np.uint64))
    for n in (N_TABLE, N_PLAIN):
        pool = h.g1_fixed_base_mul(rand_fr_gpu(n, 7100 + n), cref.g1_generator())
        pool_host = pool.cpu().numpy().view(np.uint64)
        for kind in KINDS:
            s = rand_fr_gpu(n, 7200 + n + len(kind)).cpu().numpy().view(np.uint64)
            b = pool_host.copy()
            if kind == "equal_bases":
                b[:] = b[0]
            elif kind == "plus_minus_pairs":
                b[1::2] = _negated(pyref, b[0::2])
                s[1:n // 2:2] = s[0:n // 2:2]          # first half: P and -P under ONE scalar share every bucket
            elif kind == "edge_scalars":
                s = np.ascontiguousarray(edge[np.arange(n) % 3])
                b[n // 2:] = b[n // 2]                 # ... and half the bases equal as well
            want = cref.g1_to_affine(cref.best_multiexp(s, b, 4))[0]
            out[kind, n] = (torch.from_numpy(s.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda(), want)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_table_msm_drives_the_bucket_accumulation_kernel(cases, kind):
    """n = 2^12 on the fixed-base table (threshold lowered for the test): K3 and the row / column reduction."""
    lib = _lib.load()
    s, b, want = cases[kind, N_TABLE]
    _lib.check(lib.hm_set_fixed_base_threshold(12))
    try:
        hd = h.register_bases(b)
        try:
            assert h.bases_info(hd)["table_windows"] != 0
            assert g1_equal(h.best_multiexp(s, hd), want), kind
        finally:
            h.release_bases(hd)
    finally:
        _lib.check(lib.hm_set_fixed_base_threshold(17))


@pytest.mark.parametrize("kind", KINDS)
def test_plain_msm_reaches_the_same_chain_through_msm_small(cases, kind):
    """n = 2^10 on a plain base set: accumulate_chain instantiated with the single products."""
    s, b, want = cases[kind, N_PLAIN]
    assert g1_equal(h.best_multiexp(s, b), want), kind


@pytest.mark.parametrize("k", [11, 12])
def test_best_fft_one_and_two_passes(cref, pyref, k):
    """Forward against the oracle, then the inverse root and 1 / n bring the input back."""
    import torch
    x = rand_fr_gpu(1 << k, 7300 + k)
    x0 = x.cpu().numpy().view(np.uint64).copy()
    omega = pyref.fr_omega(k)
    w = pyref.fr_array([omega])[0]
    h.best_fft(x, w, k)
    torch.cuda.synchronize()
    fwd = x.cpu().numpy().view(np.uint64)
    assert np.array_equal(fwd, cref.best_fft(x0, w, k, 4)), k
    h.best_fft(x, pyref.fr_array([pow(omega, pyref.R - 2, pyref.R)])[0], k)
    torch.cuda.synchronize()
    ninv = np.tile(pyref.fr_array([pow(1 << k, pyref.R - 2, pyref.R)]), (1 << k, 1))
    assert np.array_equal(cref.fr_mul(x.cpu().numpy().view(np.uint64), ninv), x0), k


def test_batch_invert_multiplies_back_to_one(cref, pyref):
    n = 1 << 10
    x = rand_fr_gpu(n, 7400)
    x0 = x.cpu().numpy().view(np.uint64).copy()
    assert not (x0 == 0).all(axis=1).any()
    h.batch_invert(x)
    one = np.tile(pyref.fr_array([1]), (n, 1))
    assert np.array_equal(cref.fr_mul(x.cpu().numpy().view(np.uint64), x0), one)
