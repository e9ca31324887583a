"""The exception barrier of the C ABI (include/halo2_mi355x.h: "never aborts or throws across the boundary").

libhalo2_mi355x_fi.so is the same sources built with -DHM_FAULT_INJECTION: hm_test_arm_fault(point, after) makes the
(after + 1)-th passage through a named fault point throw std::runtime_error.  A throw under an extern "C" entry must come
back as HM_ERR_INTERNAL with a message -- not std::terminate -- must release the device lock (the next call works), and a
helper thread that cannot be started must degrade to the calling thread, never to a joinable std::thread being destroyed.
The reference side would at worst see a Rust panic here (/root/reference/src/circuits/utils.rs:48: `.expect(...)`)."""
import ctypes
import threading

import numpy as np
import pytest

from halo2_experiments_amd import _lib

HM_ERR_INTERNAL = -5


@pytest.fixture()
def fi():
    lib = _lib.load_fi()
    yield lib
    lib.hm_test_arm_fault(None, 0)


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def test_fi_build_exports_the_same_abi():
    lib = _lib.load_fi()
    assert b"gfx950" in lib.hm_version()
    for name in _lib._SIGNATURES:
        assert hasattr(lib, name)
    assert not hasattr(_lib.load(), "hm_test_arm_fault"), "the product library must not carry the fault hook"


def test_a_throw_inside_a_host_entry_is_an_error_code(fi, golden):
    """hm_g1_sum needs no device: the fault point at its top throws on CPU-only boxes too."""
    pts = np.zeros((2, 12), dtype=np.uint64)
    out = np.zeros(12, dtype=np.uint64)
    assert fi.hm_g1_sum(_u64(pts), 2, _u64(out)) == 0
    fi.hm_test_arm_fault(b"g1_sum", 1)                    # the second passage throws
    assert fi.hm_g1_sum(_u64(pts), 2, _u64(out)) == 0
    assert fi.hm_g1_sum(_u64(pts), 2, _u64(out)) == HM_ERR_INTERNAL
    msg = fi.hm_last_error()
    assert b"hm_g1_sum" in msg and b"injected fault at g1_sum" in msg
    assert fi.hm_g1_sum(_u64(pts), 2, _u64(out)) == 0     # disarmed by firing; the library is still usable


def test_a_throw_on_another_thread_stays_on_that_thread(fi):
    """hm_last_error is per thread: the message of a guarded failure does not leak to the caller's thread."""
    pts, out = np.zeros((1, 12), dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    assert fi.hm_set_msm_devices(None, 0) == 0
    seen = {}

    def work():
        fi.hm_test_arm_fault(b"g1_sum", 0)
        seen["rc"] = fi.hm_g1_sum(_u64(pts), 1, _u64(out))
        seen["msg"] = fi.hm_last_error()

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert seen["rc"] == HM_ERR_INTERNAL and b"injected" in seen["msg"]
    assert fi.hm_g1_sum(_u64(pts), 1, _u64(out)) == 0


# ---- with a device: faults under the device lock, in helper-thread creation and inside helper threads ---------------------

def _rand_fr(n, seed):
    from halo2_experiments_amd.arithmetic import random_fr
    return random_fr(n, seed, "cuda")                 # uniform over the whole of [0, r)


def _fi_bases(fi, n, seed, cref):
    """n affine points [t_i]G as host words, made by the FI library's own fixed-base kernel."""
    import torch
    t = _rand_fr(n, seed)
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    gen = cref.g1_generator()
    assert fi.hm_g1_fixed_base_mul_dev(ctypes.c_void_p(t.data_ptr()), n, _u64(gen), ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).copy()


def _msm_host(lib, s, b):
    out, ident = np.zeros(8, dtype=np.uint64), ctypes.c_int(0)
    rc = lib.hm_msm_bn256_g1(_u64(s), _u64(b), s.shape[0], _u64(out), ctypes.byref(ident))
    return rc, out, ident.value


@pytest.mark.gpu
def test_faults_in_the_drop_in_call(fi, cref):
    """hm_msm_bn256_g1 on an array large enough for the four-thread digest (>= 8 MiB): a digest thread that cannot be
    started is replaced by the calling thread (same result); a throw inside the call, under the device lock, is an error
    code and the lock is free afterwards."""
    n = 1 << 17                                            # 8 MiB of bases
    b = _fi_bases(fi, n, 9101, cref)
    s = _rand_fr(n, 9102).cpu().numpy().view(np.uint64).copy()
    rc, want, _ = _msm_host(fi, s, b)
    assert rc == 0
    exp = cref.g1_to_affine(cref.best_multiexp(s, b, 8))[0]
    assert np.array_equal(want, exp)
    fi.hm_test_arm_fault(b"digest_spawn", 1)               # the second of three helper threads cannot be had
    rc, got, _ = _msm_host(fi, s, b)
    assert rc == 0 and np.array_equal(got, want)
    fi.hm_test_arm_fault(b"digest", 0)                     # a throw under ctx->mu
    rc, got, _ = _msm_host(fi, s, b)
    assert rc == HM_ERR_INTERNAL and b"hm_msm_bn256_g1" in fi.hm_last_error()
    rc, got, _ = _msm_host(fi, s, b)                       # the lock was released by the unwinding
    assert rc == 0 and np.array_equal(got, want)


@pytest.mark.gpu
def test_the_copy_lanes_are_optional(fi, cref):
    """The host-pointer forms move their arrays through four (at most eight) pinned staging lanes, a helper thread each (csrc/xfer.hip): lanes
    whose thread cannot be started are run by the calling thread -- same result, no error; in place on the allocation the coefficients
    live in the contents are kept."""
    from halo2_experiments_amd.domain import EvaluationDomain, fr_words
    d = EvaluationDomain(7, 15)                            # 1 MiB up, 8 MiB down: every lane
    n, en = d.n, d.extended_len()
    coeffs = _rand_fr(n, 9150).cpu().numpy().view(np.uint64).copy()
    coset = np.concatenate([fr_words(1), fr_words(d.g_coset), fr_words(d.g_coset * d.g_coset)])
    def run():
        out = np.empty((en, 4), dtype=np.uint64)           # fresh pages
        rc = fi.hm_coeff_to_extended_bn256_fr(_u64(coeffs), _u64(out), _u64(fr_words(d.extended_omega)), d.k, d.extended_k, _u64(coset))
        return rc, out
    assert fi.hm_set_host_copies(1) == 0                   # lanes always (the default policy too, for ranges the caller has not registered)
    rc, want = run()
    assert rc == 0
    pad = np.zeros((en, 4), dtype=np.uint64)
    pad[:n] = cref.fr_mul(coeffs, np.stack([fr_words([1, d.g_coset, d.g_coset * d.g_coset][i % 3]) for i in range(n)]))
    assert np.array_equal(want, cref.best_fft(pad, fr_words(d.extended_omega), d.extended_k))
    for after in (0, 2, 9):                                # not even the first helper / the third / one of the second transfer's
        fi.hm_test_arm_fault(b"xfer_spawn", after)
        rc, got = run()
        assert rc == 0 and np.array_equal(got, want), after
    fi.hm_test_arm_fault(None, 0)
    buf = np.zeros((en, 4), dtype=np.uint64)               # in place on the allocation the coefficients live in
    buf[:n] = coeffs
    assert fi.hm_coeff_to_extended_bn256_fr(_u64(buf), _u64(buf), _u64(fr_words(d.extended_omega)), d.k, d.extended_k, _u64(coset)) == 0
    assert np.array_equal(buf, want)
    a = want.copy()                                        # hm_ntt_bn256_fr through the same lanes, odd sizes of transfer included
    exp = cref.best_fft(want, fr_words(d.extended_omega), d.extended_k)
    fi.hm_test_arm_fault(b"xfer_spawn", 3)
    assert fi.hm_ntt_bn256_fr(_u64(a), _u64(fr_words(d.extended_omega)), d.extended_k) == 0 and np.array_equal(a, exp)
    fi.hm_test_arm_fault(None, 0)
    assert fi.hm_set_host_copies(2) == 0                   # direct always: the prefault helpers are optional too
    fi.hm_test_arm_fault(b"prefault", 1)
    rc, got = run()
    assert rc == 0 and np.array_equal(got, want)
    fi.hm_test_arm_fault(None, 0)
    assert fi.hm_set_host_copies(3) == -1 and fi.hm_set_host_copies(0) == 0


@pytest.mark.gpu
def test_faults_in_the_multi_device_workers(fi, cref):
    """hm_set_msm_devices((0, 0, 0)): a worker thread that cannot be started hands its part to the calling thread; a throw
    inside a worker comes back as an error code from the caller's call (and the other workers are joined, not abandoned)."""
    n = 3 * (1 << 14) + 5
    b = _fi_bases(fi, n, 9201, cref)
    s = _rand_fr(n, 9202).cpu().numpy().view(np.uint64).copy()
    rc, want, _ = _msm_host(fi, s, b)
    assert rc == 0
    devs = (ctypes.c_int * 3)(0, 0, 0)
    assert fi.hm_set_msm_devices(devs, 3) == 0
    try:
        rc, got, _ = _msm_host(fi, s, b)
        assert rc == 0 and np.array_equal(got, want)
        fi.hm_test_arm_fault(b"worker_spawn", 0)
        rc, got, _ = _msm_host(fi, s, b)
        assert rc == 0 and np.array_equal(got, want)
        fi.hm_test_arm_fault(b"worker_body", 1)
        rc, got, _ = _msm_host(fi, s, b)
        assert rc == HM_ERR_INTERNAL and b"injected fault at worker_body" in fi.hm_last_error()
        rc, got, _ = _msm_host(fi, s, b)
        assert rc == 0 and np.array_equal(got, want)
    finally:
        assert fi.hm_set_msm_devices(None, 0) == 0


@pytest.mark.gpu
def test_faults_in_the_batch_waiter(fi, cref):
    """hm_msm_batch_bn256_g1_h: without its waiter thread the call awaits between submissions (same results); a throw
    inside the waiter is an error code, every ticket of the call is still awaited (the next batch finds all slots free)."""
    n, count = 1 << 12, 19
    b = _fi_bases(fi, n, 9301, cref)
    hd = ctypes.c_uint64(0)
    assert fi.hm_register_bases(_u64(b), n, ctypes.byref(hd)) == 0
    try:
        cols = [_rand_fr(n, 9310 + i).cpu().numpy().view(np.uint64).copy() for i in range(count)]
        ptrs = (ctypes.c_void_p * count)(*[c.ctypes.data for c in cols])
        want = np.zeros((count, 12), dtype=np.uint64)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(want)) == 0
        exp = cref.g1_to_affine(cref.best_multiexp(cols[3], b, 4))[0]
        assert np.array_equal(want[3][:8], exp)
        got = np.zeros_like(want)
        fi.hm_test_arm_fault(b"batch_waiter_spawn", 0)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) == 0
        assert np.array_equal(got, want)
        fi.hm_test_arm_fault(b"batch_await", 1)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) < 0
        got[:] = 0
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) == 0
        assert np.array_equal(got, want)
        # a throw IN THE SUBMIT LOOP with chains already in flight (19 columns of 2^12 = four grouped chains,
        # no waiter started yet: the calling thread awaits what it issued).  The call reports an error; every ticket it
        # issued is awaited or abandoned before the staging lock goes back (the next batch finds every slot free and its
        # staging buffers its own), and results are right again.
        for after in (1, 3):
            fi.hm_test_arm_fault(b"batch_submit", after)
            assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) < 0
            assert b"batch_submit" in fi.hm_last_error()
            fi.hm_test_arm_fault(None, 0)
            got[:] = 0
            assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) == 0
            assert np.array_equal(got, want)
    finally:
        assert fi.hm_release_bases(hd) == 0
    # the same with the waiters RUNNING: 12 dense columns of 2^17 against a SLICE of the set (offset 1: no table, so every
    # column keeps a chain of its own) are 12 chains on 8 lanes, the waiters start at the ninth
    n, count = 1 << 17, 12
    b = _fi_bases(fi, n + 1, 9302, cref)
    assert fi.hm_register_bases(_u64(b), n + 1, ctypes.byref(hd)) == 0
    try:
        cols = [_rand_fr(n, 9340 + i).cpu().numpy().view(np.uint64).copy() for i in range(count)]
        ptrs = (ctypes.c_void_p * count)(*[c.ctypes.data for c in cols])
        want, got = np.zeros((count, 12), dtype=np.uint64), np.zeros((count, 12), dtype=np.uint64)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 1, ptrs, n, count, _u64(want)) == 0
        assert np.array_equal(want[11][:8], cref.g1_to_affine(cref.best_multiexp(cols[11], b[1:], 8))[0])
        fi.hm_test_arm_fault(b"batch_submit", 10)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 1, ptrs, n, count, _u64(got)) < 0
        fi.hm_test_arm_fault(None, 0)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 1, ptrs, n, count, _u64(got)) == 0
        assert np.array_equal(got, want)
        # ... and on the whole set: the dense columns share chains of the general pipeline on the table (three chains of four):
        # a throw before the third one leaves two grouped chains in flight
        whole = np.zeros((count, 12), dtype=np.uint64)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n + 1, 0, _u64(whole)) == 0          # (an empty phase is fine)
    finally:
        assert fi.hm_release_bases(hd) == 0
    b = b[: n].copy()
    assert fi.hm_register_bases(_u64(b), n, ctypes.byref(hd)) == 0
    try:
        want, got = np.zeros((count, 12), dtype=np.uint64), np.zeros((count, 12), dtype=np.uint64)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(want)) == 0
        for i in (0, 5, 11):
            assert np.array_equal(want[i][:8], cref.g1_to_affine(cref.best_multiexp(cols[i], b, 8))[0]), i
        fi.hm_test_arm_fault(b"batch_submit", 2)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) < 0
        fi.hm_test_arm_fault(None, 0)
        assert fi.hm_msm_batch_bn256_g1_h(hd, 0, ptrs, n, count, _u64(got)) == 0
        assert np.array_equal(got, want)
    finally:
        assert fi.hm_release_bases(hd) == 0


@pytest.mark.gpu
def test_an_exhausted_device_gets_the_librarys_caches_back(fi):
    """hm_device_malloc's retry freed parked base sets only, while the library may hold 1 GiB of twiddle sets and 2 GiB of
    coset power tables.  Test build: an armed "device_malloc_oom" fails the first attempt like an exhausted device; the call must
    succeed on the retry, after every cached table has gone (hm_get_stats), and the transforms rebuild theirs on demand."""
    from halo2_experiments_amd.domain import EvaluationDomain, fr_words
    d = EvaluationDomain(7, 12)
    a = _rand_fr(d.n, 9300).cpu().numpy().view(np.uint64).copy()
    want = a.copy()
    assert fi.hm_ntt_bn256_fr(_u64(want), _u64(fr_words(d.omega)), d.k) == 0                  # builds a twiddle set
    ext = np.empty((d.extended_len(), 4), dtype=np.uint64)
    coset = np.concatenate([fr_words(1), fr_words(d.g_coset), fr_words(d.g_coset * d.g_coset)])
    assert fi.hm_coeff_to_extended_bn256_fr(_u64(a), _u64(ext), _u64(fr_words(d.extended_omega)), d.k, d.extended_k, _u64(coset)) == 0
    st = _lib.Stats()
    assert fi.hm_get_stats(ctypes.byref(st)) == 0 and st.ntt_tables >= 2 and st.ntt_table_bytes > 0
    # parked base sets (left by other tests of this process) go first and may satisfy the retry by themselves: the second "exhausted"
    # call finds none and takes the tables
    for _ in range(2):
        fi.hm_test_arm_fault(b"device_malloc_oom", 0)
        p = ctypes.c_void_p()
        assert fi.hm_device_malloc(1 << 20, ctypes.byref(p)) == 0 and p.value                  # the retry, after the caches gave back
        fi.hm_test_arm_fault(None, 0)
        assert fi.hm_device_free(p) == 0
    assert fi.hm_get_stats(ctypes.byref(st)) == 0 and st.ntt_tables == 0 and st.ntt_table_bytes == 0 and st.coset_tables == 0
    again = a.copy()
    assert fi.hm_ntt_bn256_fr(_u64(again), _u64(fr_words(d.omega)), d.k) == 0 and np.array_equal(again, want)      # rebuilt on demand
    assert fi.hm_get_stats(ctypes.byref(st)) == 0 and st.ntt_tables == 1


# ---- per-call device scratch: every request can fail, and the call after it is right -----------------------------------------------------
# The drivers get their scratch in two ways only (csrc/hm_internal.h): a buffer of the stream's slot inside aux_scope, or stream-ordered
# memory inside stream_scratch.  Both pass the fault point "scratch_alloc" on EVERY request, so arming it at after = 0, 1, ... until the
# call succeeds enumerates the requests of a call.  Each entry below states that number as a literal, and `clean`: for how many of the
# leading values of `after` the pattern-filled outputs must come back untouched.  It equals `requests` but for the permutation assembly,
# which writes the identity permutation before it asks for its keys (clean = 0): no other driver launches a kernel that writes an output
# before its last request (the set quotient's and logUp's second requests follow launches that write scratch only).
HM_ERR_HIP = -3
HM_AUX_SLOTS = 4                                          # csrc/hm_internal.h
PO_COLS_MAX, EV_MAX_Q = 16, 48                            # csrc/polyops.hip, csrc/poly.hip
PATTERN = 0x5A5A5A5A5A5A5A5A
u32p = ctypes.POINTER(ctypes.c_uint32)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sp(stream):
    return ctypes.c_void_p(stream.cuda_stream if stream is not None else None)


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _fr(values):
    from halo2_experiments_amd.bn256 import fr_array
    return fr_array(values)


class _Entry:
    """One call of the test build: ``call(stream)`` -> return code; ``outs``: the device tensors and host arrays it writes, filled with
    ``fill`` (a tensor or array each; None: the pattern) before every call."""

    def __init__(self, name, requests, call, outs, fill=None, clean=None):
        self.name, self.requests, self.clean, self.call, self.outs = name, requests, requests if clean is None else clean, call, outs
        self.fill = fill or [None] * len(outs)

    def reset(self):
        for o, f in zip(self.outs, self.fill):
            if isinstance(o, np.ndarray):
                o[...] = PATTERN if f is None else f
            elif f is None:
                o.fill_(PATTERN if o.element_size() == 8 else 0x5A5A5A5A)
            else:
                o.copy_(f)

    def read(self):
        return [o.copy() if isinstance(o, np.ndarray) else o.cpu().numpy().copy() for o in self.outs]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _run(fi, e, stream=None, arm=None):
    import torch
    e.reset()
    torch.cuda.synchronize()
    if arm is not None:
        fi.hm_test_arm_fault(b"scratch_alloc", arm)
    try:
        rc = e.call(stream)
    finally:
        fi.hm_test_arm_fault(None, 0)
    msg = fi.hm_last_error()
    torch.cuda.synchronize()
    return rc, msg, e.read()


def _sweep(fi, e, second):
    import torch
    e.reset()
    torch.cuda.synchronize()
    blank = e.read()
    rc, msg, want = _run(fi, e)
    assert rc == 0, (e.name, msg)
    assert not _same(want, blank) or not e.outs, e.name          # the call does write what the pattern check looks at
    k = 0
    while True:
        rc, msg, got = _run(fi, e, arm=k)
        if rc == 0:                                                # the armed passage was not reached: k requests in all
            assert _same(got, want), (e.name, k)
            break
        assert rc == HM_ERR_HIP and b"scratch allocation failed" in msg, (e.name, k, rc, msg)
        if k < e.clean:
            assert _same(got, blank), (e.name, k)
        for stream in (None, second):
            rc, msg, got = _run(fi, e, stream)
            assert rc == 0 and _same(got, want), (e.name, k, stream, msg)
        k += 1
        assert k <= 8, e.name
    assert k == e.requests, (e.name, k)


def _code(fn, *args):
    """a wrapper of the Python layer as a return code"""
    try:
        fn(*args)
    except _lib.Halo2Mi355xError as err:
        return err.code
    return 0


def _poly_entries(fi):
    import torch
    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
    out = []
    for count in (1, PO_COLS_MAX + 1):                        # one column; a second group of the loop
        polys, z, qs = [_rand_fr(5, 9400 + i) for i in range(count)], _fr(list(range(3, 3 + count))), [new(5, 4) for _ in range(count)]
        out.append(_Entry(f"kate x{count}", 1, lambda s, a=(polys, z, qs, count): fi.hm_kate_division_batch_bn256_fr_dev(
            _ptrs(a[0]), 5, _u64(a[1]), _ptrs(a[2]), a[3], _sp(s)), qs))
    count = PO_COLS_MAX + 1
    fs, start, zs = [_rand_fr(5, 9420 + i) for i in range(count)], _fr(7), [new(5, 4) for _ in range(count)]
    out.append(_Entry("grand product, chained", 1, lambda s: fi.hm_fr_grand_product_batch_dev(_ptrs(fs), 5, _u64(start), 3, _ptrs(zs), count,
                                                                                             _sp(s)), zs))
    a, b, dot = _rand_fr(3, 9440), _rand_fr(3, 9441), np.zeros(4, dtype=np.uint64)
    out.append(_Entry("dot", 1, lambda s: fi.hm_fr_dot_bn256_dev(_vp(a), _vp(b), 3, _u64(dot), _sp(s)), [dot]))
    q = EV_MAX_Q + 1                                           # a second launch of the loop
    poly, idx, pts, evals = _rand_fr(17, 9442), np.zeros(q, dtype=np.uint32), _fr(list(range(2, 2 + q))), np.zeros((q, 4), dtype=np.uint64)
    out.append(_Entry("eval_polynomial", 1, lambda s: fi.hm_eval_polynomial_bn256_fr_dev(_vp(poly), 17, idx.ctypes.data_as(u32p), _u64(pts), q,
                                                                                        _u64(evals), _sp(s)), [evals]))
    # SHPLONK set quotient, t = 2 points, n = 8, two polynomials per proof: the single form, and the batch form with 2 proofs (its own
    # workspace, then the batched linear combination's table)
    ps_, w, x, sc = [_rand_fr(8, 9450 + i) for i in range(4)], _fr([1, 2, 3, 4]), _fr([5, 7, 11, 13]), _fr([3, 9])
    h1, h2 = new(8, 4), [new(8, 4), new(8, 4)]
    out.append(_Entry("set quotient", 1, lambda s: fi.hm_shplonk_set_quotient_bn256_fr_dev(_ptrs(ps_[:2]), _u64(w), 2, 8, _u64(x), 2, _u64(sc),
                                                                                          _vp(h1), 0, _sp(s)), [h1]))
    out.append(_Entry("set quotient batch", 2, lambda s: fi.hm_shplonk_set_quotient_batch_bn256_fr_dev(_ptrs(ps_), _u64(w), 2, 8, _u64(x), 2,
                                                                                                      _u64(sc), _ptrs(h2), 0, 2, _sp(s)), h2))
    terms, c6, lc = [_rand_fr(8, 9460 + i) for i in range(6)], _fr(list(range(21, 27))), [new(8, 4), new(8, 4)]
    out.append(_Entry("linear combination batch", 1, lambda s: fi.hm_fr_linear_combination_batch_dev(_ptrs(terms), _u64(c6), 3, 8, _ptrs(lc), 2,
                                                                                                    _sp(s)), lc))
    cells = torch.tensor([5, 0, 15, 2, 9, 1, 7, 3, 8, 4, 10, 6, 12, 14, 13, 11], dtype=torch.int32, device="cuda")
    om, de, sigma = _fr(_omega(3)), _fr(7), new(16, 4)
    out.append(_Entry("permutation columns", 1, lambda s: fi.hm_permutation_columns_bn256_fr_dev(ctypes.cast(_vp(cells), u32p), 2, 3, _u64(om),
                                                                                                _u64(de), _vp(sigma), _sp(s)), [sigma]))
    return out


def _omega(k):
    from oracle import bn256_ref
    return bn256_ref.fr_omega(k)


def _lookup_entries(fi):
    import torch
    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
    out = []
    table = _rand_fr(5, 9500)
    inp = table[torch.tensor([0, 0, 2, 4, 4], device="cuda")].contiguous()
    pi, pt, miss = new(5, 4), new(5, 4), (ctypes.c_int * 1)()
    out.append(_Entry("lookup permute", 1, lambda s: fi.hm_lookup_permute_batch_bn256_fr_dev(_ptrs([inp]), _ptrs([table]), 1, 5, _ptrs([pi]),
                                                                                            _ptrs([pt]), miss, _sp(s)), [pi, pt]))
    pick = torch.tensor([7, 7, 0, 3, 3, 3, 1, 6], device="cuda")
    for name, tab in (("small keys", _dev(_fr(list(range(10, 18))))), ("general keys", _rand_fr(8, 9510))):   # value bins / sorted records
        col, m, miss2, counts = tab[pick].contiguous(), new(8, 4), (ctypes.c_int * 1)(), (ctypes.c_uint32 * 1)(1)
        out.append(_Entry(f"logup multiplicities, {name}", 2, lambda s, a=(tab, col, m, miss2, counts): fi.hm_logup_multiplicities_bn256_fr_dev(
            _ptrs([a[0]]), _ptrs([a[1]]), a[4], 1, 8, _ptrs([a[2]]), a[3], _sp(s)), [m]))
    terms, sums = _rand_fr(8, 9520), new(8, 4)
    out.append(_Entry("grand sum", 1, lambda s: fi.hm_fr_grand_sum_batch_dev(_ptrs([terms]), 8, _ptrs([sums]), 1, _sp(s)), [sums]))
    return out


def _g1_entries(fi):
    import torch
    from halo2_experiments_amd.bn256 import g1_words
    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
    out = []
    gen, t3, p3 = g1_words((1, 2)), _rand_fr(3, 9600), new(3, 8)
    mul = lambda s, t=t3, p=p3, n=3: fi.hm_g1_fixed_base_mul_dev(_vp(t), n, _u64(gen), _vp(p), _sp(s))
    out.append(_Entry("fixed-base mul", 1, mul, [p3]))
    t4, p4 = _rand_fr(4, 9601), new(4, 8)
    assert mul(None, t4, p4, 4) == 0 and mul(None) == 0
    torch.cuda.synchronize()
    points, pts3, om = p4.clone(), p3.clone(), _fr(_omega(2))
    out.append(_Entry("g1 fft", 1, lambda s: fi.hm_g1_fft_bn256_dev(_vp(p4), _u64(om), 2, None, _sp(s)), [p4], [points]))      # in place
    table, coeffs, proofs = new(8, 8), _rand_fr(4, 9602), new(4, 8)
    assert fi.hm_kzg_open_table_bn256_dev(_vp(points), 2, _vp(table), None) == 0
    out.append(_Entry("open_all", 1, lambda s: fi.hm_kzg_open_all_bn256_dev(_vp(table), _vp(coeffs), 2, 1, _vp(proofs), _sp(s)), [proofs]))
    packed, back, first = new(3, 4), new(3, 8), np.zeros(1, dtype=np.uint64)
    assert fi.hm_g1_compress_bn256_dev(_vp(pts3), 3, _vp(packed), None) == 0
    torch.cuda.synchronize()
    # (*out_first_invalid is set to n before anything else, so it is no pattern-checked output: a success must leave n there)
    def verdict(rc):
        assert rc != 0 or first[0] == 3
        return rc
    out.append(_Entry("decompress", 1, lambda s: verdict(fi.hm_g1_decompress_bn256_dev(_vp(packed), 3, _vp(back), _u64(first), _sp(s))), [back]))
    out.append(_Entry("check", 1, lambda s: verdict(fi.hm_g1_check_bn256_dev(_vp(pts3), 3, _u64(first), _sp(s))), []))
    return out


def _hash_entries(fi, spec_handle):
    import torch
    from halo2_experiments_amd._marshal import _dev_ptr
    new = lambda *shape, dtype=torch.int64: torch.empty(shape, dtype=dtype, device="cuda")
    out = []
    values, perm = _rand_fr(5, 9700), new(5)
    out.append(_Entry("argsort", 1, lambda s: fi.hm_fr_argsort_bn256_dev(_vp(values), 5, _dev_ptr(perm), _sp(s)), [perm]))
    copies = torch.tensor([[0, 9], [9, 3], [4, 12], [15, 1]], dtype=torch.int32, device="cuda")      # cells of 2 columns of 2^3 rows
    cells = new(16, dtype=torch.int32)
    out.append(_Entry("permutation assembly", 1, lambda s: fi.hm_permutation_assemble_dev(_dev_ptr(copies, u32p), 4, 2, 3, _dev_ptr(cells, u32p),
                                                                                         None, _sp(s)), [cells], clean=0))
    # SafeAccumulator: one user, 4 rows, 4 limbs of 4 bits at k = 5 (the shape of smoke())
    vals, init = _dev(_fr([1, 3, 2, 5])), torch.tensor([[0, 0, 14, 13]], dtype=torch.int64, device="cuda")
    adv, fin, over = new(10, 32, 4), new(1, 4), new(1, dtype=torch.int32)
    out.append(_Entry("accumulator witness", 1, lambda s: fi.hm_accumulator_witness_bn256_fr_dev(
        4, 4, 5, 1, 4, _vp(vals), _dev_ptr(init), _vp(adv), _dev_ptr(fin), _dev_ptr(over, u32p), _sp(s)), [adv, fin, over]))
    # a Merkle sum tree of depth 2: 4 leaves of (hash, balance), 7 nodes
    leaves, nodes = _rand_fr(8, 9710), new(7, 2, 4)
    assert fi.hm_merkle_sum_tree_build_dev(spec_handle, _vp(leaves), 2, _vp(nodes), None) == 0
    torch.cuda.synchronize()
    built, idx, leaf = nodes.clone(), torch.tensor([1], dtype=torch.int64, device="cuda"), _rand_fr(2, 9711)
    out.append(_Entry("merkle update", 1, lambda s: fi.hm_merkle_sum_tree_update_dev(spec_handle, 2, _vp(nodes), _dev_ptr(idx), _vp(leaf), 1, None,
                                                                                    _sp(s)), [nodes], [built]))           # in place
    sibs, roots = new(2, 2, 4), new(1, 2, 4)
    assert fi.hm_merkle_paths_dev(_vp(built), 2, 2, _dev_ptr(idx), 1, _vp(sibs), None) == 0
    torch.cuda.synchronize()
    out.append(_Entry("merkle roots", 0, lambda s: fi.hm_merkle_roots_bn256_dev(spec_handle, 2, 1, _vp(leaves[2:4]), _vp(sibs), _dev_ptr(idx),
                                                                               _vp(roots), _sp(s)), [roots]))           # no scratch of its own
    return out


def _verifier_entries(fi, keep):
    """The Blake2b and the Keccak transcript and one terms call, on the recorded SHPLONK proofs of the Poseidon system (tests/golden/
    gwc_proofs_poseidon.npz, the smallest recorded).  The caller has routed the Python layer to the test build."""
    import torch
    import halo2_experiments_amd as h
    from halo2_experiments_amd import device_transcript
    import gwc_cases as gc
    rec = gc.recorded("poseidon")
    out = []
    for enc in gc.ENCODINGS:
        bv = h.BatchVerifier(None, rec["vk"], seed=5, transcript="device", encoding=enc)
        keep.append(bv)
        bv.add_proof(rec["instance"], rec["proofs"][("shplonk", enc)])
        st = bv._prepare()
        assert st["bad"] == [False]
        n_ch = st["d_records"].shape[1] - 1
        fresh = st["d_records"].clone()
        fresh[:, :n_ch] = PATTERN                               # the challenges; r_b behind them stays
        records, flags = fresh.clone(), torch.zeros(1, dtype=torch.int32, device="cuda")

        def transcript(s, bv=bv, st=st, records=records, flags=flags):
            with torch.cuda.stream(s):
                return _code(device_transcript.challenges, bv.layout, bv._digest, bv._preamble_instances(), st["d_proofs"], st["d_ybytes"], flags,
                             records, st["preamble"], st["d_table"])
        out.append(_Entry(f"transcript, {enc}", 1, transcript, [records, flags], [fresh, torch.zeros_like(flags)]))
        if enc == "halo2":
            outs = [torch.empty_like(st[key]) for key in ("d_own", "d_shared", "d_h2_r", "d_h2_l")]
            flags2 = torch.zeros(1, dtype=torch.int32, device="cuda")
            terms = lambda s, bv=bv, st=st: _code(bv._queue_terms, st["plan"], 1, st["d_records"], st["d_scalars"], st["d_inst"], flags2, *outs,
                                                  _sp(s))
            out.append(_Entry("terms", 2, terms, outs))
    return out


@pytest.fixture()
def fi_spec(fi):
    """a width-5 Poseidon spec of the test build (its own contexts and handles)"""
    from halo2_experiments_amd import poseidon as P
    import poseidon_checker as chk
    rc, mds, _ = P.default_spec(5).constants()
    rcw, mdsw = chk.to_words([v for r in rc for v in r]), chk.to_words([v for r in mds for v in r])
    handle = ctypes.c_uint64(0)
    assert fi.hm_poseidon_create(5, 4, 8, 56, _u64(rcw), _u64(mdsw), ctypes.byref(handle)) == 0
    yield handle
    assert fi.hm_poseidon_destroy(handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["poly", "lookup", "g1", "hash", "verifier"])
def test_every_scratch_request_can_fail_and_the_next_call_is_right(fi, fi_spec, group, monkeypatch):
    import torch
    second = torch.cuda.Stream()
    keep = []
    if group == "verifier":
        monkeypatch.setattr(_lib, "_lib", fi)                  # BatchVerifier and the transcripts' wrapper call the test build
    try:
        entries = {"poly": _poly_entries, "lookup": _lookup_entries, "g1": _g1_entries}[group](fi) if group in ("poly", "lookup", "g1") \
            else _hash_entries(fi, fi_spec) if group == "hash" else _verifier_entries(fi, keep)
        torch.cuda.synchronize()
        for e in entries:
            _sweep(fi, e, second)
    finally:
        for bv in keep:
            bv.close()


@pytest.mark.gpu
def test_slot_pressure_after_a_failure(fi):
    """A failed call leaves its slot with a recorded event: more streams than slots, back to back, each get buffers nobody is writing.
    n = 1025 gives two workgroups per column, so the join reads what another workgroup left in the slot's buffer."""
    import torch
    n = 1025
    factors, start = _rand_fr(n, 9800), _fr(1)
    product = lambda s, out: fi.hm_fr_grand_product_dev(_vp(factors), n, _u64(start), _vp(out), _sp(s))
    new = lambda: torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    want = new()
    assert product(None, want) == 0
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(HM_AUX_SLOTS + 1)]
    torch.cuda.synchronize()
    fi.hm_test_arm_fault(b"scratch_alloc", 0)
    try:
        assert product(streams[0], new()) == HM_ERR_HIP and b"scratch allocation failed" in fi.hm_last_error()
    finally:
        fi.hm_test_arm_fault(None, 0)
    outs = [new() for _ in streams]
    torch.cuda.synchronize()
    for s, out in zip(streams, outs):                          # no wait between them
        assert product(s, out) == 0
    torch.cuda.synchronize()
    for out in outs:
        assert torch.equal(out, want)
