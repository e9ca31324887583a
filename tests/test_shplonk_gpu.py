"""hm_shplonk_set_quotient_bn256_fr_dev on the GPU, word for word: against shplonk.set_quotient_ints (interpolate, subtract, divide point by
point on integers) for n <= 2^10, and above that against the same chain composed from the kernels that existed before it
(linear_combination, eval_polynomial, host interpolation, kate_division once per point).

The shapes come from the kernel's own plan (shplonk.set_quotient_plan: a lane owns B = 4 rows up to n = 2^18, a workgroup 256 lanes):
  n = t + 1    the smallest the entry accepts: one output row, t rows of zeros
  n = 4        a single lane's chunk                  n = 5      the smallest n with a ragged last chunk (lanes of 4 + 1 rows)
  n = 64       sixteen lanes of one workgroup         n = 1024   the largest n of one workgroup (256 full lanes)
  n = 1025     the smallest n with a second workgroup (its only lane holds one row), and n = 1026
  n = 2^14     sixteen workgroups through the joining kernel
with t in {1, 2, 3, 4 = HM_SHPLONK_MAX_POINTS} and m in {1, LC_MAX = 24, 25, 60} (one, exactly one full, two, and three launches of the
combination)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, poseidon as ps, shplonk as sh
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words

pytestmark = pytest.mark.gpu
LC_MAX = 24
_u64p = ctypes.POINTER(ctypes.c_uint64)


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def test_the_shapes_are_the_plans():
    assert sh.set_quotient_plan(4) == (4, 1, 1) and sh.set_quotient_plan(5) == (4, 1, 2) and sh.set_quotient_plan(64) == (4, 1, 16)
    assert sh.set_quotient_plan(1024) == (4, 1, 256) and sh.set_quotient_plan(1025) == (4, 2, 257) and sh.set_quotient_plan(1 << 14)[1] == 16
    assert sh.MAX_POINTS == 4


def case(n, m, t, seed):
    rng = random.Random(seed)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    weights = [rng.randrange(R) for _ in range(m)]
    points = [rng.randrange(R) for _ in range(t)]
    return polys, weights, points, rng.randrange(1, R), [rng.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("t", [1, 2, 3, 4])
@pytest.mark.parametrize("n,m", [(0, 1), (0, 60), (4, 25), (5, 1), (5, 24), (64, 60), (64, 25), (1024, 1), (1024, 25)])
def test_against_the_integer_twin(n, m, t):
    n = n or t + 1
    if n < t + 1:
        n = t + 2                                   # n = 4 is below t + 1 for t = 4: six rows, two lanes, the second ragged
    polys, weights, points, scale, base = case(n, m, t, 7 * n + 100 * m + t)
    want = sh.set_quotient_ints(polys, weights, points, scale)
    assert want[n - t:] == [0] * t
    cols = [d(p) for p in polys]
    got = sh.set_quotient(cols, weights, points, scale)
    assert ints(got) == want
    out = d(base)
    assert sh.set_quotient(cols, weights, points, scale, out=out, accumulate=True) is out
    assert ints(out) == [(b + w) % R for b, w in zip(base, want)]          # the top t rows: base + 0, untouched
    assert ints(cols[0]) == polys[0]                                       # the inputs are only read


def composed(cols, weights, points, scale):
    """the route of the kernels before this one: combine, evaluate, interpolate on the host, subtract, divide once per point, scale"""
    n, t = cols[0].shape[0], len(points)
    num = h.linear_combination(cols, np.stack([fr_words(w) for w in weights]))
    evals = ps.words_to_ints(h.eval_polynomial(num.reshape(1, n, 4), np.stack([fr_words(p) for p in points]),
                                               poly_index=np.zeros(t, dtype=np.uint32)))
    r = d(sh.lagrange_interpolate_ints(points, evals) + [0] * (n - t))
    q = h.linear_combination([num, r], np.stack([fr_words(1), fr_words(R - 1)]))
    for p in points:
        q = h.kate_division(q, fr_words(p))
    q = h.linear_combination([q], np.stack([fr_words(scale)]))
    return torch.cat([q, torch.zeros((t, 4), dtype=torch.int64, device="cuda")])


@pytest.mark.parametrize("t", [1, 2, 3, 4])
@pytest.mark.parametrize("n,m", [(1025, 25), (1026, 1), (1 << 14, 60)])
def test_against_the_composed_route(n, m, t):
    rng = random.Random(n + m + t)
    cols = [h.random_fr(n, 1000 * m + j) for j in range(m)]
    weights = [rng.randrange(R) for _ in range(m)]
    points = [rng.randrange(R) for _ in range(t)]
    scale = rng.randrange(1, R)
    want = composed(cols, weights, points, scale)
    assert not bool(want[n - t:].any()) and bool(want[n - t - 1].any())
    got = sh.set_quotient(cols, weights, points, scale)
    assert torch.equal(got, want)
    # accumulate, on a stream of its own: twice the quotient on top of a copy of it is three times it
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = got.clone()
        sh.set_quotient(cols, weights, points, 2 * scale % R, out=acc, accumulate=True)
        three = h.linear_combination([want], np.stack([fr_words(3)]))
    side.synchronize()
    assert torch.equal(acc, three)


def test_the_output_may_be_an_input():
    n = 1025
    cols = [h.random_fr(n, 5), h.random_fr(n, 6)]
    want = sh.set_quotient(cols, [3, 4], [9, 10, 11])
    keep = cols[1].clone()
    assert sh.set_quotient(cols, [3, 4], [9, 10, 11], out=cols[1]) is cols[1]
    assert torch.equal(cols[1], want) and not torch.equal(keep, want)


def test_refusals_leave_the_output_untouched():
    lib = _lib.load()
    n = 64
    cols = [h.random_fr(n, 1), h.random_fr(n, 2)]
    out = h.random_fr(n, 3)
    before = out.clone()
    p = lambda values: np.stack([fr_words(v) for v in values]).ctypes.data_as(_u64p)
    tab = (ctypes.c_void_p * 2)(cols[0].data_ptr(), cols[1].data_ptr())
    f = lib.hm_shplonk_set_quotient_bn256_fr_dev
    o = ctypes.c_void_p(out.data_ptr())
    one = p([1])
    calls = {
        "t = 0": lambda: f(tab, p([1, 2]), 2, n, p([5, 6]), 0, one, o, 0, None),
        "t above the cap": lambda: f(tab, p([1, 2]), 2, n, p([5, 6, 7, 8, 9]), 5, one, o, 0, None),
        "two equal points": lambda: f(tab, p([1, 2]), 2, n, p([5, 6, 5]), 3, one, o, 0, None),
        "m = 0": lambda: f(tab, p([1, 2]), 0, n, p([5, 6]), 2, one, o, 0, None),
        "n < t + 1": lambda: f(tab, p([1, 2]), 2, 2, p([5, 6]), 2, one, o, 0, None),
        "null table": lambda: f(None, p([1, 2]), 2, n, p([5, 6]), 2, one, o, 0, None),
        "null polynomial": lambda: f((ctypes.c_void_p * 2)(cols[0].data_ptr(), None), p([1, 2]), 2, n, p([5, 6]), 2, one, o, 0, None),
        "misaligned polynomial": lambda: f((ctypes.c_void_p * 2)(cols[0].data_ptr(), cols[1].data_ptr() + 8), p([1, 2]), 2, n - 1, p([5, 6]), 2,
                                           one, o, 0, None),
        "misaligned output": lambda: f(tab, p([1, 2]), 2, n - 1, p([5, 6]), 2, one, ctypes.c_void_p(out.data_ptr() + 8), 0, None),
        "null output": lambda: f(tab, p([1, 2]), 2, n, p([5, 6]), 2, one, None, 0, None),
        "null weights": lambda: f(tab, None, 2, n, p([5, 6]), 2, one, o, 0, None),
        "a point not below r": lambda: f(tab, p([1, 2]), 2, n, np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).ctypes.data_as(_u64p), 1, one, o,
                                         1, None),
    }
    for name, call in calls.items():
        assert call() == -1, name                                          # HM_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert torch.equal(out, before), name
    with pytest.raises(ValueError):
        sh.set_quotient(cols, [1, 2], [5, 5])
    with pytest.raises(ValueError):
        sh.set_quotient(cols, [1], [5])
    assert f(tab, p([1, 2]), 2, n, p([5, 6]), 2, one, o, 0, None) == 0     # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert ints(out) == sh.set_quotient_ints([ints(c) for c in cols], [1, 2], [5, 6])
