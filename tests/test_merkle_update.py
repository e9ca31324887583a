"""Updating a built Merkle (sum) tree in place and the roots of many paths, the parts that need no GPU: the exports, the C ABI's argument
checks, ``update_plan`` against brute force, and the planning arithmetic of the update kernels (poseidon.inc's ``merkle_update_key`` /
``_owned`` / ``_count``) built for the host against ``update_plan``.  Every comparison is exact."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import poseidon_checker as chk
from halo2_experiments_amd import _lib
from halo2_experiments_amd import poseidon as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = chk.R
NO_SPEC = ctypes.c_uint64(1 << 40)          # a handle no spec has: with a device present nothing can be launched on these host buffers
HM_ERR_BAD_ARG, HM_ERR_NO_DEVICE = -1, -2
NEW_ENTRIES = ("hm_merkle_sum_tree_update_dev", "hm_merkle_tree_update_dev", "hm_merkle_roots_bn256_dev", "hm_merkle_roots_bn256")


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _vp(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def test_package_exports_the_feature():
    import halo2_experiments_amd as h
    assert hasattr(h, "update_plan") and "update_plan" in h.__all__ and h.update_plan is P.update_plan
    for cls in (h.MerkleSumTree, h.MerkleTree):
        assert callable(getattr(cls, "update")) and callable(getattr(cls, "path_roots"))
    header = open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib._SIGNATURES and hasattr(_lib.load(), name) and hasattr(_lib.load_fi(), name)
        assert f"int {name}(" in header


def _aligned(nbytes):
    """a zeroed host buffer whose address is a multiple of 64 (the checks look at alignment and overlap only; nothing is read)"""
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + nbytes]


def test_bad_arguments_are_reported_before_anything_else():
    lib = _lib.load()
    nodes, leaves, idx, counts = _aligned(7 * 64), _aligned(4 * 64), _aligned(64), _aligned(64)
    for fn, elem in ((lib.hm_merkle_sum_tree_update_dev, 64), (lib.hm_merkle_tree_update_dev, 32)):
        ok = dict(depth=2, nodes=_vp(nodes), idx=_u64(idx), leaves=_vp(leaves), m=2, counts=_u32(counts))

        def call(**kw):
            a = dict(ok, **kw)
            return fn(NO_SPEC, a["depth"], a["nodes"], a["idx"], a["leaves"], a["m"], a["counts"], None)
        assert call(nodes=None) == HM_ERR_BAD_ARG                                    # NULL with m > 0
        assert call(idx=None) == HM_ERR_BAD_ARG
        assert call(leaves=None) == HM_ERR_BAD_ARG
        assert call(depth=0) == HM_ERR_BAD_ARG and call(depth=31) == HM_ERR_BAD_ARG
        assert call(m=(1 << 31) + 1) == HM_ERR_BAD_ARG
        assert b"2^31" in lib.hm_last_error()
        assert call(nodes=_vp(nodes, 8)) == HM_ERR_BAD_ARG                           # not 16-byte aligned
        assert b"aligned" in lib.hm_last_error()
        assert call(leaves=_vp(leaves, 8)) == HM_ERR_BAD_ARG
        assert call(idx=ctypes.cast(_vp(idx, 4), ctypes.POINTER(ctypes.c_uint64))) == HM_ERR_BAD_ARG
        assert call(leaves=_vp(nodes)) == HM_ERR_BAD_ARG                             # the new leaves inside the nodes
        assert b"overlaps" in lib.hm_last_error()
        assert call(leaves=_vp(nodes, 6 * elem)) == HM_ERR_BAD_ARG                   # ... on the root, the last of the 2^(depth+1) - 1
        assert call(leaves=_vp(nodes, 7 * elem), m=1) != HM_ERR_BAD_ARG              # right behind the nodes is fine
    dev, host = lib.hm_merkle_roots_bn256_dev, lib.hm_merkle_roots_bn256
    buf = _aligned(16 * 64)
    v, u = _vp(buf), _u64(buf)
    for k in range(4):                                                               # NULL with m > 0
        args = [v, v, u, v]
        args[k] = None
        assert dev(NO_SPEC, 2, 1, *args, None) == HM_ERR_BAD_ARG
        args = [u, u, u, u]
        args[k] = None
        assert host(NO_SPEC, 2, 1, *args) == HM_ERR_BAD_ARG
    for depth in (0, 31):
        assert dev(NO_SPEC, depth, 1, v, v, u, v, None) == HM_ERR_BAD_ARG
        assert host(NO_SPEC, depth, 1, u, u, u, u) == HM_ERR_BAD_ARG
    assert dev(NO_SPEC, 2, (1 << 31) + 1, v, v, u, v, None) == HM_ERR_BAD_ARG
    assert host(NO_SPEC, 2, (1 << 31) + 1, u, u, u, u) == HM_ERR_BAD_ARG
    for k in (0, 1, 3):
        args = [v, v, u, v]
        args[k] = _vp(buf, 8)
        assert dev(NO_SPEC, 2, 1, *args, None) == HM_ERR_BAD_ARG
        assert b"aligned" in lib.hm_last_error()
    assert dev(NO_SPEC, 2, 1, v, v, ctypes.cast(_vp(buf, 4), ctypes.POINTER(ctypes.c_uint64)), v, None) == HM_ERR_BAD_ARG


def test_without_a_device_every_new_entry_says_so():
    lib = _lib.load()
    if lib.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    nodes, leaves, idx, counts = _aligned(7 * 64), _aligned(4 * 64), _aligned(64), _aligned(64)
    for fn in (lib.hm_merkle_sum_tree_update_dev, lib.hm_merkle_tree_update_dev):
        assert fn(1, 2, _vp(nodes), _u64(idx), _vp(leaves), 2, _u32(counts), None) == HM_ERR_NO_DEVICE
        assert fn(1, 2, None, None, None, 0, None, None) == HM_ERR_NO_DEVICE         # m = 0: after the argument checks all the same
        assert fn(1, 0, None, None, None, 0, None, None) == HM_ERR_BAD_ARG           # ... which come first
    assert lib.hm_merkle_roots_bn256_dev(NO_SPEC, 2, 1, _vp(nodes), _vp(nodes), _u64(idx), _vp(leaves), None) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_roots_bn256(1, 2, 1, _u64(nodes), _u64(nodes), _u64(idx), _u64(leaves)) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_roots_bn256(1, 2, 0, None, None, None, None) == HM_ERR_NO_DEVICE
    with pytest.raises(_lib.Halo2Mi355xError) as e:
        P.MerkleSumTree.path_roots(np.zeros((1, 2, 4), dtype=np.uint64), np.zeros((1, 3, 2, 4), dtype=np.uint64), [0])
    assert e.value.code == HM_ERR_NO_DEVICE


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def plan_cases():
    """(depth, indices) with seeded inputs: m = 1, all leaves, random with repeats, neighbours, the two halves, an index out of range"""
    rng = random.Random(1515)
    cases = []
    for depth in (1, 2, 5, 12):
        n = 1 << depth
        cases.append((depth, [rng.randrange(n)]))
        everyone = list(range(n))
        rng.shuffle(everyone)
        cases.append((depth, everyone))
        for m in (3, 40, 300):
            cases.append((depth, [rng.randrange(n) for _ in range(m)]))
        cases.append((depth, [0, 1]))                                        # differ in bit 0 only
        cases.append((depth, [n - 2, n - 1]))
        cases.append((depth, [n // 2 - 1, n - 1]))                           # differ in the top bit only
        cases.append((depth, [1 % n, 1 % n + n // 2][::-1]))
        cases.append((depth, [rng.randrange(n), n, rng.randrange(n), (1 << 40) + 1, n + 5]))   # out of range among valid ones
        cases.append((depth, [n, n + 1]))                                    # nothing but dropped entries
    cases.append((12, []))
    return cases


def _brute(depth, indices):
    live = [i for i in indices if i < (1 << depth)]
    return [len({i >> l for i in live}) for l in range(depth + 1)]


def test_update_plan_equals_brute_force():
    for depth, idx in plan_cases():
        got = P.update_plan(depth, idx)
        assert got == _brute(depth, idx), (depth, idx[:8])
        assert got == P.update_plan(depth, np.array(idx, dtype=np.uint64)) and len(got) == depth + 1
        if got[0]:
            assert got[depth] == 1 and all(a >= b for a, b in zip(got, got[1:]))
    assert P.update_plan(5, [0, 1]) == [2, 1, 1, 1, 1, 1]
    assert P.update_plan(5, [15, 31]) == [2, 2, 2, 2, 2, 1]
    assert P.update_plan(3, [7, 7, 7, 8]) == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        P.update_plan(0, [0])


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    assert hasattr(lib, "hc_merkle_update_plan") and hasattr(lib, "hc_merkle_roots")
    return lib


def test_the_kernels_planning_arithmetic_on_the_host_equals_update_plan(hc):
    rng = random.Random(99)
    cases = plan_cases() + [(30, [rng.randrange(1 << 30) for _ in range(500)] + [(1 << 30) - 1, 0, 1 << 30, (1 << 64) - 1]),
                            (24, [rng.randrange(1 << 10) << 14 for _ in range(2000)])]
    for depth, idx in cases:
        arr = np.array(idx, dtype=np.uint64)
        counts = np.full(depth + 2, 0xDEAD, dtype=np.uint32)
        assert hc.hc_merkle_update_plan(depth, _u64(arr), ctypes.c_size_t(len(idx)), _u32(counts)) == 0
        assert counts[:depth + 1].tolist() == P.update_plan(depth, idx), (depth, idx[:8])
        assert counts[depth + 1] == 0xDEAD
    assert hc.hc_merkle_update_plan(0, None, ctypes.c_size_t(0), None) != 0 and hc.hc_merkle_update_plan(31, None, ctypes.c_size_t(0), None) != 0


def _limbs9(v):
    x = v % R * (1 << 261) % R
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


@pytest.mark.parametrize("width", [3, 5])
def test_host_build_of_the_root_lane_equals_verify_path(hc, width):
    """the lane of the roots kernel with HM_BOUNDS armed, against the host integers; index bits above the depth are ignored"""
    rng = random.Random(40 + width)
    spec = P.default_spec(width)
    rc, mds, _ = spec.constants()
    flat = [v for row in rc for v in row] + [v for row in mds for v in row] + [(width - 1) << 64]
    consts = np.array([l for v in flat for l in _limbs9(v)], dtype=np.uint32)
    E, depth, m = (width - 1) // 2, 3, 5
    leaves = [[rng.randrange(R) for _ in range(E)] for _ in range(m)]
    sibs = [[[rng.randrange(R) for _ in range(E)] for _ in range(depth)] for _ in range(m)]
    sibs[0][1][-1] = R - 1                                                             # a balance sum that wraps
    idx = [rng.randrange(1 << depth) for _ in range(m)]
    lw = np.ascontiguousarray(chk.to_words([v for leaf in leaves for v in leaf])).view(np.uint32)
    sw = np.ascontiguousarray(chk.to_words([v for path in sibs for node in path for v in node])).view(np.uint32)
    iw = np.array([i | (rng.randrange(1 << 20) << depth) for i in idx], dtype=np.uint64)
    out = np.zeros((m * E, 8), dtype=np.uint32)
    assert hc.hc_merkle_roots(width, _vp(consts), 8, 56, depth, ctypes.c_size_t(m), _vp(lw), _vp(sw), _u64(iw), _vp(out)) == 0
    got = chk.from_words(out.view(np.uint64))
    for u in range(m):
        bits = [(idx[u] >> l) & 1 for l in range(depth)]
        if E == 2:
            exp = P.MerkleSumTree.verify_path(tuple(leaves[u]), ([s[0] for s in sibs[u]], [s[1] for s in sibs[u]], bits))
            assert tuple(got[2 * u:2 * u + 2]) == exp, u
        else:
            assert got[u] == P.MerkleTree.verify_path(leaves[u][0], ([s[0] for s in sibs[u]], bits)), u
