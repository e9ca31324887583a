"""Helper of tests/test_witness_v3.py: paths and messages through libhm_hostcheck.so's hc_merkle_witness / hc_poseidon_witness (the
lane functions of merkle_witness_kernel<1>, merkle_chain_kernel<1> and poseidon_witness_kernel compiled for the host with the limb-bound
checks on), as integer columns."""
import ctypes

import numpy as np

from halo2_experiments_amd import _lib, poseidon as ps
from halo2_experiments_amd.domain import FR_MODULUS as R

_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_p = lambda a: a.ctypes.data_as(_u32p)


def _limbs9(v):
    """the library's internal form: v * 2^261 mod r in 9 limbs of 29 bits"""
    x = v % R * (1 << 261) % R
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


def const_block(spec):
    rc, mds, _ = spec.constants()
    flat = [v for row in rc for v in row] + [v for row in mds for v in row] + [spec.rate << 64]
    return np.array([l for v in flat for l in _limbs9(v)], dtype=np.uint32)


def _columns(adv):
    return [ps.words_to_ints(col.view(np.uint64)) for col in adv]


def run_merkle(spec, lay, leaf, siblings, bits, nodes=None):
    """-> (advice columns, [leaf, root]); nodes: integers of a built tree, level by level (the chain is not run then)"""
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    consts, depth = const_block(spec), lay.depth
    leaves = ps.ints_to_words([leaf]).view(np.uint32)
    sib = ps.ints_to_words(list(siblings)).view(np.uint32)
    idx = np.array([sum(int(b) << l for l, b in enumerate(bits))], dtype=np.uint64)
    tree = ps.ints_to_words(list(nodes)).view(np.uint32) if nodes is not None else None
    run_buf = np.zeros(max(depth - 1, 1) * 8, dtype=np.uint32)
    adv = np.zeros((lay.N_ADVICE, lay.n, 8), dtype=np.uint32)
    inst = np.zeros((2, 8), dtype=np.uint32)
    lib.hc_merkle_witness.restype = ctypes.c_int
    lib.hc_merkle_witness.argtypes = [_u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, _u32p, _u32p,
                                      _u64p, _u32p, _u32p, _u32p, _u32p]
    rc = lib.hc_merkle_witness(_p(consts), spec.r_f, spec.r_p, depth, lay.k, 1, _p(leaves), _p(sib), idx.ctypes.data_as(_u64p),
                               _p(tree) if tree is not None else None, _p(run_buf), _p(adv), _p(inst))
    assert rc == 0
    return _columns(adv), ps.words_to_ints(inst.view(np.uint64))


def run_poseidon(spec, lay, message):
    """-> (advice columns, [digest])"""
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    consts = const_block(spec)
    msgs = ps.ints_to_words(list(message)).view(np.uint32)
    adv = np.zeros((lay.N_ADVICE, lay.n, 8), dtype=np.uint32)
    inst = np.zeros((1, 8), dtype=np.uint32)
    lib.hc_poseidon_witness.restype = ctypes.c_int
    lib.hc_poseidon_witness.argtypes = [_u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, _u32p, _u32p, _u32p]
    assert lib.hc_poseidon_witness(_p(consts), spec.r_f, spec.r_p, lay.k, 1, _p(msgs), _p(adv), _p(inst)) == 0
    return _columns(adv), ps.words_to_ints(inst.view(np.uint64))
