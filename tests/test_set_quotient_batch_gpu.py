"""hm_shplonk_set_quotient_batch_bn256_fr_dev and hm_fr_linear_combination_batch_dev on the GPU: a batch of
independent proofs in one launch chain equals the loop of the single entry, word for word.  n = 8 (one lane), 1000 (a ragged last chunk),
1028 (257 lanes: a second workgroup and the join); t = 1 .. 4; 1 and 3 proofs; m = 1 and 5 with one polynomial shared by all proofs;
both ``accumulate`` values.  At n = 8 also against the integers (``set_quotient_ints``).  An output may be one of its own proof's
inputs; an output that is another proof's input, a non-canonical point in proof 2 only and two equal points in proof 1 only are
HM_ERR_BAD_ARG with every output untouched."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, arithmetic as ar, poseidon as ps, shplonk as sh
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words

pytestmark = pytest.mark.gpu
_u64p = ctypes.POINTER(ctypes.c_uint64)


def ints(t):
    torch.cuda.synchronize()
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def batch(n, m, t, proofs, seed):
    """-> (polys[b][j], weights[b][j], points[b][l], scales[b], bases[b]): polynomial 0 is ONE tensor for all proofs"""
    rng = random.Random(seed)
    shared = h.random_fr(n, seed)
    polys = [[shared] + [h.random_fr(n, seed + 100 * b + j) for j in range(1, m)] for b in range(proofs)]
    weights = [[rng.randrange(R) for _ in range(m)] for _ in range(proofs)]
    points = [[rng.randrange(R) for _ in range(t)] for _ in range(proofs)]
    scales = [rng.randrange(1, R) for _ in range(proofs)]
    bases = [h.random_fr(n, seed + 7000 + b) for b in range(proofs)]
    return polys, weights, points, scales, bases


@pytest.mark.parametrize("proofs", [1, 3])
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("t", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [8, 1000, 1028])
def test_the_batch_equals_the_loop(n, t, m, proofs):
    polys, weights, points, scales, bases = batch(n, m, t, proofs, 13 * n + 5 * t + m + proofs)
    want = [sh.set_quotient(polys[b], weights[b], points[b], scales[b]) for b in range(proofs)]
    got = sh.set_quotient_batch(polys, weights, points, scales)
    for b in range(proofs):
        assert torch.equal(got[b], want[b]), b
        assert not bool(got[b][n - t:].any()) and bool(got[b][n - t - 1].any())
    # accumulate: on top of each proof's own base, against the loop on a copy
    want_acc = [sh.set_quotient(polys[b], weights[b], points[b], scales[b], out=bases[b].clone(), accumulate=True) for b in range(proofs)]
    outs = [x.clone() for x in bases]
    back = sh.set_quotient_batch(polys, weights, points, scales, outs=outs, accumulate=True)
    for b in range(proofs):
        assert back[b] is outs[b] and torch.equal(outs[b], want_acc[b]), b
    if n == 8:
        for b in range(proofs):
            assert ints(got[b]) == sh.set_quotient_ints([ints(p) for p in polys[b]], weights[b], points[b], scales[b]), b


def test_an_output_may_be_one_of_its_own_proofs_inputs():
    n, proofs = 1028, 3
    polys, weights, points, scales, _ = batch(n, 3, 2, proofs, 77)
    want = sh.set_quotient_batch(polys, weights, points, scales)
    keep = [polys[b][2].clone() for b in range(proofs)]
    outs = sh.set_quotient_batch(polys, weights, points, scales, outs=[polys[b][2] for b in range(proofs)])
    for b in range(proofs):
        assert outs[b] is polys[b][2] and torch.equal(outs[b], want[b]) and not torch.equal(keep[b], want[b])


def raw_call(polys, weights, points_words, scales, outs, m, n, t, accumulate=0):
    lib = _lib.load()
    proofs = len(outs)
    tab = (ctypes.c_void_p * (proofs * m))(*[p.data_ptr() for row in polys for p in row])
    out_tab = (ctypes.c_void_p * proofs)(*[o if isinstance(o, int) else o.data_ptr() for o in outs])
    w = np.stack([fr_words(v) for row in weights for v in row])
    s = np.stack([fr_words(v) for v in scales])
    pts = np.ascontiguousarray(points_words, dtype=np.uint64)
    return lib.hm_shplonk_set_quotient_batch_bn256_fr_dev(tab, w.ctypes.data_as(_u64p), m, n, pts.ctypes.data_as(_u64p), t, s.ctypes.data_as(_u64p),
                                                          out_tab, accumulate, proofs, None)


def test_refusals_leave_every_output_untouched():
    n, m, t, proofs = 64, 2, 2, 3
    polys, weights, points, scales, bases = batch(n, m, t, proofs, 91)
    outs = [x.clone() for x in bases]
    words = lambda pts: np.stack([fr_words(v) for row in pts for v in row])
    good = words(points)
    BAD = _lib.HM_ERR_BAD_ARG

    def untouched(what):
        torch.cuda.synchronize()
        for b in range(proofs):
            assert torch.equal(outs[b], bases[b]), (what, b)
        for b in range(proofs):
            assert torch.equal(polys[b][1], kept[b]), (what, b)

    kept = [polys[b][1].clone() for b in range(proofs)]
    # d_outs[0] is proof 1's input
    assert raw_call(polys, weights, good, scales, [polys[1][1], outs[1], outs[2]], m, n, t) == BAD
    untouched("an output that is another proof's input")
    assert raw_call(polys, weights, good, scales, [outs[0], outs[1], outs[1]], m, n, t) == BAD
    untouched("two proofs with one output")
    # the shared polynomial as proof 0's output: it is proof 1's input too
    assert raw_call(polys, weights, good, scales, [polys[0][0], outs[1], outs[2]], m, n, t) == BAD
    untouched("the shared polynomial as an output")
    not_canonical = good.copy()
    not_canonical[2 * t] = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert raw_call(polys, weights, not_canonical, scales, outs, m, n, t) == BAD
    untouched("a point not below r in proof 2 only")
    equal = good.copy()
    equal[1 * t + 1] = equal[1 * t]
    assert raw_call(polys, weights, equal, scales, outs, m, n, t) == BAD
    untouched("two equal points in proof 1 only")
    assert raw_call(polys, weights, good, scales, [outs[0], 0, outs[2]], m, n, t) == BAD
    assert raw_call(polys, weights, good, scales, [outs[0], outs[1].data_ptr() + 8, outs[2]], m, n - 1, t) == BAD
    assert raw_call(polys, weights, good, scales, outs, m, 2, t) == BAD                                  # n < t + 1
    assert raw_call(polys, weights, good[:proofs * 5], scales, outs, m, n, 0) == BAD
    assert _lib.load().hm_shplonk_set_quotient_batch_bn256_fr_dev(None, None, m, n, None, t, None, None, 0, 0, None) == BAD
    untouched("null, misaligned, short")
    with pytest.raises(ValueError):
        sh.set_quotient_batch(polys, weights, [[5, 5]] * proofs, scales)
    with pytest.raises(ValueError):
        sh.set_quotient_batch(polys, weights, points[:2], scales)
    with pytest.raises(ValueError):
        sh.set_quotient_batch(polys, [w[:1] for w in weights], points, scales)
    # and the same call with good arguments runs
    assert raw_call(polys, weights, good, scales, outs, m, n, t) == _lib.HM_OK
    for b in range(proofs):
        assert ints(outs[b]) == sh.set_quotient_ints([ints(p) for p in polys[b]], weights[b], points[b], scales[b])


@pytest.mark.parametrize("proofs", [1, 3])
@pytest.mark.parametrize("count", [0, 1, 5, 24, 25, 60])
@pytest.mark.parametrize("n", [8, 1000])
def test_the_batched_linear_combination_equals_the_loop(n, count, proofs):
    rng = random.Random(n + count + proofs)
    shared = h.random_fr(n, 3)
    polys = [([shared] if count else []) + [h.random_fr(n, 10 + 100 * b + j) for j in range(1, count)] for b in range(proofs)]
    coeffs = [[rng.randrange(R) for _ in range(count)] for _ in range(proofs)]
    outs = [h.random_fr(n, 900 + b) for b in range(proofs)]
    want = [h.linear_combination(polys[b], np.stack([fr_words(c) for c in coeffs[b]]) if count else np.zeros((0, 4), dtype=np.uint64),
                                 out=outs[b].clone()) for b in range(proofs)]
    got = ar.linear_combination_batch(polys, coeffs, outs=outs)
    for b in range(proofs):
        assert got[b] is outs[b] and torch.equal(got[b], want[b]), b
        if count == 0:
            assert not bool(got[b].any())
    if count:
        fresh = ar.linear_combination_batch(polys, coeffs)
        assert all(torch.equal(fresh[b], want[b]) for b in range(proofs))


def test_the_linear_combination_may_write_one_of_its_own_inputs_only():
    n, proofs, count = 1000, 3, 30
    polys = [[h.random_fr(n, 40 + 100 * b + j) for j in range(count)] for b in range(proofs)]
    coeffs = [[b + j + 2 for j in range(count)] for b in range(proofs)]
    want = ar.linear_combination_batch(polys, coeffs)
    outs = ar.linear_combination_batch(polys, coeffs, outs=[polys[b][count - 1] for b in range(proofs)])     # the LAST term is the output
    assert all(torch.equal(outs[b], want[b]) for b in range(proofs))
    polys = [[h.random_fr(n, 40 + 100 * b + j) for j in range(count)] for b in range(proofs)]
    kept = polys[1][0].clone()
    with pytest.raises(_lib.Halo2Mi355xError):
        ar.linear_combination_batch(polys, coeffs, outs=[polys[1][0], polys[1][1], polys[2][2]])
    torch.cuda.synchronize()
    assert torch.equal(polys[1][0], kept)
