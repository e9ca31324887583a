"""Poseidon over BN256 Fr and the Merkle sum tree, the parts that need no GPU: the C ABI's argument checks, the kernels' per-hash code
built for the host with bound tracking (libhm_hostcheck.so, -DHM_BOUNDS) against the tests' own checker (tests/poseidon_checker.py),
the structure of the constant generator and of the permutation, verify_path on the reference's fixture, and the ISA of the kernels.
Every comparison is exact (integers mod r)."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import poseidon_checker as chk
from halo2_experiments_amd import _lib
from halo2_experiments_amd import poseidon as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = chk.R
HM_ERR_BAD_ARG, HM_ERR_NO_DEVICE = -1, -2


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _spec_words(spec):
    rc, mds, _ = spec.constants()
    return chk.to_words([v for row in rc for v in row]), chk.to_words([v for row in mds for v in row])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------

def test_package_exports_the_feature():
    import halo2_experiments_amd as h
    for name in ("Spec", "poseidon_hash", "poseidon_hash_host", "MerkleSumTree", "MerkleTree"):
        assert hasattr(h, name) and name in h.__all__
    for name in ("hm_poseidon_create", "hm_poseidon_destroy", "hm_poseidon_hash_bn256_fr_dev", "hm_poseidon_hash_bn256_fr",
                 "hm_merkle_sum_tree_build_dev", "hm_merkle_sum_tree_build", "hm_merkle_tree_build_dev", "hm_merkle_paths_dev"):
        assert name in _lib._SIGNATURES and hasattr(_lib.load(), name)


def test_bad_arguments_are_reported_before_anything_else():
    lib = _lib.load()
    rc5, mds5 = _spec_words(P.default_spec(5))
    rc3, mds3 = _spec_words(P.default_spec(3))
    out = ctypes.c_uint64(0)
    create = lib.hm_poseidon_create
    assert create(4, 3, 8, 56, _u64(rc5), _u64(mds5), ctypes.byref(out)) == HM_ERR_BAD_ARG          # width not 3 or 5
    assert create(2, 1, 8, 56, _u64(rc5), _u64(mds5), ctypes.byref(out)) == HM_ERR_BAD_ARG
    assert create(5, 3, 8, 56, _u64(rc5), _u64(mds5), ctypes.byref(out)) == HM_ERR_BAD_ARG          # rate != width - 1
    assert create(3, 3, 8, 56, _u64(rc3), _u64(mds3), ctypes.byref(out)) == HM_ERR_BAD_ARG
    assert create(5, 4, 7, 56, _u64(rc5), _u64(mds5), ctypes.byref(out)) == HM_ERR_BAD_ARG          # odd r_f
    assert create(5, 4, 8, 56, None, _u64(mds5), ctypes.byref(out)) == HM_ERR_BAD_ARG               # null pointers
    assert create(5, 4, 8, 56, _u64(rc5), None, ctypes.byref(out)) == HM_ERR_BAD_ARG
    assert create(5, 4, 8, 56, _u64(rc5), _u64(mds5), None) == HM_ERR_BAD_ARG
    r_words = np.array([(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
    for arr, pos in ((rc5, 0), (rc5, rc5.shape[0] - 1), (mds5, 7)):                                  # a constant >= r
        bad = arr.copy()
        bad[pos] = r_words
        args = (_u64(bad), _u64(mds5)) if arr is rc5 else (_u64(rc5), _u64(bad))
        assert create(5, 4, 8, 56, *args, ctypes.byref(out)) == HM_ERR_BAD_ARG
        assert b"modulus" in lib.hm_last_error()
    bad = mds3.copy()
    bad[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert create(3, 2, 8, 56, _u64(rc3), _u64(bad), ctypes.byref(out)) == HM_ERR_BAD_ARG
    buf = np.zeros((8, 4), dtype=np.uint64)
    assert lib.hm_poseidon_hash_bn256_fr_dev(1, None, 4, _vp(buf), None) == HM_ERR_BAD_ARG           # NULL with n > 0
    assert lib.hm_poseidon_hash_bn256_fr_dev(1, _vp(buf), 4, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_poseidon_hash_bn256_fr(1, None, 4, _u64(buf)) == HM_ERR_BAD_ARG
    assert lib.hm_poseidon_hash_bn256_fr(1, _u64(buf), 4, None) == HM_ERR_BAD_ARG
    for fn in (lib.hm_merkle_sum_tree_build_dev, lib.hm_merkle_tree_build_dev):
        assert fn(1, _vp(buf), 31, _vp(buf), None) == HM_ERR_BAD_ARG                                 # depth > 30
        assert fn(1, None, 2, _vp(buf), None) == HM_ERR_BAD_ARG
        assert fn(1, _vp(buf), 2, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_sum_tree_build(1, _u64(buf), 31, _u64(buf), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_sum_tree_build(1, None, 2, _u64(buf), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_sum_tree_build(1, _u64(buf), 2, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_paths_dev(_vp(buf), 31, 2, _u64(buf), 1, _vp(buf), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_paths_dev(_vp(buf), 2, 3, _u64(buf), 1, _vp(buf), None) == HM_ERR_BAD_ARG   # elements per node: 1 or 2
    assert lib.hm_merkle_paths_dev(None, 2, 2, _u64(buf), 1, _vp(buf), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_paths_dev(_vp(buf), 2, 2, None, 1, _vp(buf), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_paths_dev(_vp(buf), 2, 2, _u64(buf), 1, None, None) == HM_ERR_BAD_ARG


def test_without_a_device_every_entry_says_so():
    lib = _lib.load()
    if lib.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    rc5, mds5 = _spec_words(P.default_spec(5))
    out = ctypes.c_uint64(0)
    buf = np.zeros((16, 4), dtype=np.uint64)
    assert lib.hm_poseidon_create(5, 4, 8, 56, _u64(rc5), _u64(mds5), ctypes.byref(out)) == HM_ERR_NO_DEVICE
    assert lib.hm_poseidon_destroy(1) == HM_ERR_NO_DEVICE
    assert lib.hm_poseidon_hash_bn256_fr_dev(1, _vp(buf), 1, _vp(buf), None) == HM_ERR_NO_DEVICE
    assert lib.hm_poseidon_hash_bn256_fr(1, _u64(buf), 1, _u64(buf)) == HM_ERR_NO_DEVICE
    assert lib.hm_poseidon_hash_bn256_fr(1, None, 0, None) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_sum_tree_build_dev(1, _vp(buf), 1, _vp(buf), None) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_sum_tree_build(1, _u64(buf), 1, _u64(buf), None) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_tree_build_dev(1, _vp(buf), 1, _vp(buf), None) == HM_ERR_NO_DEVICE
    assert lib.hm_merkle_paths_dev(_vp(buf), 1, 2, _u64(buf), 1, _vp(buf), None) == HM_ERR_NO_DEVICE
    with pytest.raises(_lib.Halo2Mi355xError) as e:
        P.poseidon_hash_host(P.default_spec(3), np.zeros((1, 2, 4), dtype=np.uint64))
    assert e.value.code == HM_ERR_NO_DEVICE


# ---- the kernels' per-hash code on the host (libhm_hostcheck.so, -DHM_BOUNDS) ----------------------------------------------------

@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    assert hasattr(lib, "hc_poseidon")
    return lib


def _limbs9(v):
    """the library's internal form: v * 2^261 mod r in 9 limbs of 29 bits"""
    x = v % R * (1 << 261) % R
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


def _const_block(rc, mds, rate):
    flat = [v for row in rc for v in row] + [v for row in mds for v in row] + [rate << 64]
    return np.array([l for v in flat for l in _limbs9(v)], dtype=np.uint32)


def _hc_hash(hc, width, rc, mds, r_f, r_p, msgs, op=0):
    consts = _const_block(rc, mds, width - 1)
    words = np.ascontiguousarray(chk.to_words([v for m in msgs for v in m])).view(np.uint32)
    out = np.zeros((len(msgs), 2 if op else 1, 8), dtype=np.uint32)
    assert hc.hc_poseidon(op, width, _vp(consts), r_f, r_p, _vp(words), _vp(out), ctypes.c_size_t(len(msgs))) == 0
    return chk.from_words(out.view(np.uint64))


@pytest.mark.parametrize("width", [3, 5])
def test_host_build_of_the_per_hash_code_equals_the_checker(hc, width):
    """1 000 random messages and the all-(r-1) / all-zero messages, HM_BOUNDS armed (a violated bound aborts the process): the tracked
    bounds do not depend on the data, so this run proves the limb bounds of the 64-round chain for every input."""
    rng = random.Random(100 + width)
    spec = P.default_spec(width)
    rc, mds, _ = spec.constants()
    msgs = [[rng.randrange(R) for _ in range(width - 1)] for _ in range(1000)] + [[R - 1] * (width - 1), [0] * (width - 1)]
    got = _hc_hash(hc, width, rc, mds, 8, 56, msgs)
    assert got == [chk.digest(m, rc, mds, 8, 56) for m in msgs]


def test_host_build_of_the_sum_tree_node(hc):
    rng = random.Random(7)
    rc, mds, _ = P.default_spec(5).constants()
    kids = [[rng.randrange(R) for _ in range(4)] for _ in range(50)] + [[R - 1] * 4, [0] * 4, [1, R - 1, 2, 1], [1, R - 2, 2, 1]]
    got = _hc_hash(hc, 5, rc, mds, 8, 56, kids, op=1)
    exp = [v for k in kids for v in (chk.digest(k, rc, mds, 8, 56), (k[1] + k[3]) % R)]
    assert got == exp


def test_host_build_with_other_round_numbers_and_worst_case_constants(hc):
    """every constant r - 1 (the largest limbs a spec can hold) and a spec with no partial rounds / few full rounds"""
    for width in (3, 5):
        for r_f, r_p in ((2, 3), (4, 0), (8, 56)):
            rc = [[R - 1] * width for _ in range(r_f + r_p)]
            mds = [[R - 1] * width for _ in range(width)]
            msgs = [[R - 1] * (width - 1), [0] * (width - 1), list(range(1, width))]
            assert _hc_hash(hc, width, rc, mds, r_f, r_p, msgs) == [chk.digest(m, rc, mds, r_f, r_p) for m in msgs]


# ---- the constant generator ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [3, 5])
def test_generator_structure(width):
    rc, mds, mds_inv = P.generate_constants(width, 8, 56, 0)
    assert len(rc) == 64 and all(len(row) == width for row in rc)
    flat = [v for row in rc for v in row]
    assert all(0 <= v < R for v in flat) and len(set(flat)) == len(flat)
    assert all(0 <= v < R for row in mds + mds_inv for v in row)
    ident = [[int(i == j) for j in range(width)] for i in range(width)]
    assert [chk.matvec(mds, col) for col in zip(*mds_inv)] == [list(c) for c in zip(*ident)]        # MDS . MDS^-1 = I, column by column
    # the Cauchy structure: entry (i, j) = 1 / (x_i + y_j) with every sum non-zero  <=>  1/m_ij - 1/m_kj does not depend on j
    inv = [[pow(v, -1, R) for v in row] for row in mds]                                             # x_i + y_j, all invertible => non-zero
    for i in range(1, width):
        assert len({(inv[i][j] - inv[0][j]) % R for j in range(width)}) == 1
    assert P.generate_constants(width, 8, 56, 0) == (rc, mds, mds_inv)                              # a pure function of its arguments
    assert P.Spec(width, width - 1).constants() == (rc, mds, mds_inv)
    for other in ((width, 8, 57, 0), (width, 6, 56, 0), (width, 8, 56, 1)):
        assert P.generate_constants(*other)[1] != mds
    assert P.generate_constants(8 - width, 8, 56, 0)[0][0][0] != rc[0][0]                           # the width is part of the seed


# ---- the permutation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [3, 5])
def test_identity_mds_and_zero_round_constants_give_the_closed_form(width):
    """No hash code takes part in the expected values: word 0 passes all 64 S-boxes, the other words the 8 of the full rounds."""
    rng = random.Random(width)
    ident = [[int(i == j) for j in range(width)] for i in range(width)]
    zero = [[0] * width for _ in range(64)]
    spec = P.Spec.from_constants(width, width - 1, 8, 56, zero, ident)
    state = [rng.randrange(R) for _ in range(width)]
    exp = [pow(state[0], pow(5, 64, R - 1), R)] + [pow(v, pow(5, 8, R - 1), R) for v in state[1:]]
    assert P.permute(spec, state) == exp
    assert chk.permutation(state, zero, ident, 8, 56) == exp
    msg = state[:-1]
    assert P.hash_ints(spec, msg) == pow(msg[0], pow(5, 64, R - 1), R)


@pytest.mark.parametrize("width", [3, 5])
def test_the_inverse_permutation_undoes_the_forward_one(width):
    rng = random.Random(50 + width)
    spec = P.default_spec(width)
    rc, mds, mds_inv = spec.constants()
    for _ in range(3):
        state = [rng.randrange(R) for _ in range(width)]
        out = P.permute(spec, state)
        assert out == chk.permutation(state, rc, mds, 8, 56)
        assert chk.inverse_permutation(out, rc, mds_inv, 8, 56) == state


def test_from_constants_takes_the_constants_as_data():
    rng = random.Random(9)
    rc = [[rng.randrange(R) for _ in range(3)] for _ in range(10)]
    mds = [[rng.randrange(R) for _ in range(3)] for _ in range(3)]
    spec = P.Spec.from_constants(3, 2, 4, 6, rc, mds)
    assert P.hash_ints(spec, [5, 6]) == chk.digest([5, 6], rc, mds, 4, 6)
    with pytest.raises(ValueError):
        P.Spec.from_constants(3, 2, 4, 6, rc[:-1], mds)
    with pytest.raises(ValueError):
        P.Spec.from_constants(3, 2, 4, 6, rc, [[R, 1, 1]] * 3)
    with pytest.raises(ValueError):
        P.Spec(4, 3)
    with pytest.raises(ValueError):
        P.Spec(5, 4, r_f=7)


# ---- verify_path on the reference's fixture -----------------------------------------------------------------------------------

def _golden_case():
    with open(os.path.join(ROOT, "tests", "golden", "merkle_sum_tree_case.json")) as f:
        g = json.load(f)
    leaf = (g["leaf"]["hash"], g["leaf"]["balance"])
    path = ([e["hash"] for e in g["path_elements"]], [e["balance"] for e in g["path_elements"]], list(g["path_indices"]))
    return leaf, path


def test_verify_path_on_the_reference_fixture():
    leaf, path = _golden_case()
    spec = P.default_spec(5)
    rc, mds, _ = spec.constants()
    root = P.MerkleSumTree.verify_path(leaf, path)
    assert root[1] == 100 + 10 + 50 + 60 + 90 + 90
    h, b = leaf                                                         # the fold, by the checker
    for eh, eb in zip(path[0], path[1]):
        h, b = chk.digest([h, b, eh, eb], rc, mds, 8, 56), b + eb
    assert root == (h, b)
    swapped = (path[0], path[1], [1] * 5)                               # index 1: the sibling is hashed first
    h, b = leaf
    for eh, eb in zip(path[0], path[1]):
        h, b = chk.digest([eh, eb, h, b], rc, mds, 8, 56), b + eb
    got = P.MerkleSumTree.verify_path(leaf, swapped)
    assert got == (h, b) and got[0] != root[0] and got[1] == root[1]
    assert P.MerkleTree.verify_path(3, ([4, 5], [0, 1])) == chk.digest(
        [5, chk.digest([3, 4], *P.default_spec(3).constants()[:2], 8, 56)], *P.default_spec(3).constants()[:2], 8, 56)


def test_trees_refuse_leaf_counts_that_are_not_powers_of_two():
    for n in (0, 1, 3, 6):
        with pytest.raises(ValueError):
            P._depth_of(n, "MerkleSumTree")
    assert P._depth_of(2, "t") == 1 and P._depth_of(1 << 20, "t") == 20


# ---- what the compiler made of the kernels --------------------------------------------------------------------------------------

def test_the_poseidon_kernels_are_in_poseidon_o_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    if not os.path.exists(os.path.join(isa_check.CSRC, "poseidon.o")):
        _lib.build()
    rows = isa_check.summary("poseidon.o")
    for kernel in ("poseidon_hash_kernelILi3", "poseidon_hash_kernelILi5", "merkle_sum_level_kernel", "merkle_path_kernel"):
        hits = [r for name, r in rows.items() if kernel in name]
        assert len(hits) == 1, kernel
        assert hits[0]["scratch"] == 0 and hits[0]["mfma"] == 0 and hits[0]["kernarg_vector_accesses"] == [], kernel
