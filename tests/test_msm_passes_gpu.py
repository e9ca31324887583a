"""The passes of the table MSM around the bucket accumulation kernel, at the smallest shapes where they can go wrong:

* coarse-bin counts out of the digits pass (msm_digits_kernel<true>) instead of msm_part1_hist_kernel,
* the reduction reading one-task buckets straight from their partials (load_bucket_value) instead of a copy pass,
* the row / column sums with one wave per sum (msm_reduce_rowcol_wave_kernel) instead of workgroup-wide trees.

Every result is compared with the closed form [sum_i s_i (a + i b)]G, built as bench.py's known_answer builds it (the device
inner product and ONE fixed-base multiplication: nothing of the MSM's passes), and, byte for byte, with the same call made
with the three switches off.  2^20 points is the smallest table set with a first sort level (13 windows of 20 bits over one
bucket set, 2^16-point chunks) and the two-launch reduction; the counting digits pass and the one-wave form of the row / column
sums are the default only where they fill the chip (2^24 points, c = 22), so they are asked for by their switches here."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N = 1 << 20
EXTRA = 12345
SWITCHES_OFF = {"HALO2_MI355X_DIGITS_COUNT": "0", "HALO2_MI355X_K3B_COPY": "1", "HALO2_MI355X_K4_WAVE_SUMS": "0"}
# the defaults (at this size: only the direct bucket reads), then the counting digits pass and the one-wave sums at this size as well
ARMS = [{}, {"HALO2_MI355X_DIGITS_COUNT": "1"}, {"HALO2_MI355X_DIGITS_COUNT": "1", "HALO2_MI355X_K4_WAVE_SUMS": "1"}]


@contextlib.contextmanager
def switches(values):
    """The library reads these switches at every MSM call."""
    keys = set(SWITCHES_OFF)
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def sets():
    """One seeded input of 2^20 + 12 345 points, shared and never modified: scalars, bases P_i = [t_i]G with t_i = a + i b, and the
    base sets registered over it."""
    import torch
    import bench
    import halo2_experiments_amd as h
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    s, bases, t = bench.bench_inputs(N + EXTRA, 0, 0x7061737365730001, dev)
    flagged = torch.arange(0, N, 100, device=dev)                      # 1 % of the bases become the identity (all-zero words)
    bases_id = bases[:N].clone()
    bases_id[flagged] = 0
    t_id = t[:N].clone()
    t_id[flagged] = 0                                                  # ... and drop out of the closed form
    hs = dict(table=h.register_bases(bases[:N].contiguous()), ragged=h.register_bases(bases), flagged=h.register_bases(bases_id),
              plain=h.register_bases(bases[:N].contiguous(), plain=True))
    try:
        yield dict(s=s, t=t, t_id=t_id, dev=dev, **hs)
    finally:
        for x in hs.values():
            h.release_bases(x)


def fr_const(value, n, dev):
    import torch
    from oracle import bn256_ref as o
    return torch.from_numpy(o.fr_array([value]).view(np.int64)).to(dev).repeat(n, 1).contiguous()


def check(scalars, t, handle, dev, table=True):
    """Closed form == the MSM in every arm of the new passes == (byte for byte) the MSM with the switches off."""
    import bench
    import halo2_experiments_amd as h
    exp = bench.known_answer(scalars, t, dev)
    with switches(SWITCHES_OFF):
        off = h.best_multiexp(scalars, handle)
    st = h.msm_stats()
    if table and not st["window_bits"] > 17:
        pytest.skip(f"the registration did not build a fixed-base table with a shared bucket set: {st}")
    assert np.array_equal(off, exp)
    for arm in ARMS:
        with switches(arm):
            got = h.best_multiexp(scalars, handle)
        assert np.array_equal(got, exp), arm
        assert got.tobytes() == off.tobytes(), arm
    return exp


def test_uniform_scalars_on_the_table_set(sets):
    """Chunks of 2^16 points divide n: the digits pass counts the coarse bins; almost every bucket is one task."""
    exp = check(sets["s"][:N].contiguous(), sets["t"][:N].contiguous(), sets["table"], sets["dev"])
    assert exp[8:].any()


def test_chunks_that_straddle_windows_keep_the_histogram_pass(sets):
    """n = 2^20 + 12 345 is no multiple of the chunk: msm_part1_hist_kernel is the one that runs."""
    check(sets["s"], sets["t"], sets["ragged"], sets["dev"])


def test_every_scalar_equal(sets):
    """All points of a window in one bucket: the hot-bucket queue, the slices and big kernels, the >= 2 partials read path, and
    lds_inc's wave-uniform guard inside the digits kernel."""
    dev = sets["dev"]
    k = 0x1d3f5b7a9c2e4f60718293a4b5c6d7e8f90123456789abcdef0123456789abcd   # 253 bits (< r): a non-zero digit in every window
    exp = check(fr_const(k, N, dev), sets["t"][:N].contiguous(), sets["table"], dev)
    assert exp[8:].any()


def test_zero_one_scalars_and_flagged_bases(sets):
    """Scalars in {0, 1} and 1 % of the bases the identity: most buckets are empty (the identity path of the bucket read)."""
    import torch
    dev = sets["dev"]
    bits = (torch.arange(N, device=dev) * 2654435761 >> 7) & 1
    s01 = fr_const(1, N, dev) * bits.view(N, 1)
    check(s01.contiguous(), sets["t_id"], sets["flagged"], dev)


def test_all_zero_scalars_give_the_identity(sets):
    import torch
    dev = sets["dev"]
    exp = check(torch.zeros((N, 4), dtype=torch.int64, device=dev), sets["t"][:N].contiguous(), sets["table"], dev)
    assert not exp.any()


def test_a_group_of_three_columns(sets):
    """best_multiexp_batch of three dense columns over the table: one launch chain, a bucket set per column (blockIdx.y)."""
    import bench
    import halo2_experiments_amd as h
    dev = sets["dev"]
    s, t = sets["s"], sets["t"][:N].contiguous()
    cols = [s[:N].contiguous(), s[EXTRA: EXTRA + N].contiguous(), s[:N].flip(0).contiguous()]
    exp = np.stack([bench.known_answer(c, t, dev) for c in cols])
    with switches(SWITCHES_OFF):
        off = h.best_multiexp_batch(cols, sets["table"])
    assert np.array_equal(off, exp)
    for arm in ARMS:
        with switches(arm):
            got = h.best_multiexp_batch(cols, sets["table"])
        assert np.array_equal(got, exp), arm
        assert got.tobytes() == off.tobytes(), arm


def test_the_plain_layout_is_untouched(sets):
    """One bucket set per window: none of the three passes applies; guards the kernels they share with it."""
    import halo2_experiments_amd as h
    check(sets["s"][:N].contiguous(), sets["t"][:N].contiguous(), sets["plain"], sets["dev"], table=False)
    assert h.msm_stats()["window_bits"] <= 17
