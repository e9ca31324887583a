"""Helper of tests/test_witness.py: one path through libhm_hostcheck.so's hc_merkle_sum_witness (the witness kernels' lane
functions compiled for the host with the limb-bound checks on), as integer columns."""
import ctypes

import numpy as np

from halo2_experiments_amd import poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R

from halo2_experiments_amd import _lib


def _limbs9(v):
    """the library's internal form: v * 2^261 mod r in 9 limbs of 29 bits"""
    x = v % R * (1 << 261) % R
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


def const_block(spec):
    rc, mds, _ = spec.constants()
    flat = [v for row in rc for v in row] + [v for row in mds for v in row] + [spec.rate << 64]
    return np.array([l for v in flat for l in _limbs9(v)], dtype=np.uint32)


def run(spec, lay, leaf, siblings, bits, assets):
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    consts = const_block(spec)
    depth, n = lay.depth, lay.n
    u32p = ctypes.POINTER(ctypes.c_uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    leaves = ps.ints_to_words(list(leaf)).view(np.uint32)
    sib = ps.ints_to_words([v for pair in siblings for v in pair]).view(np.uint32)
    idx = np.array([sum(int(b) << l for l, b in enumerate(bits))], dtype=np.uint64)
    a = ps.ints_to_words([assets % R]).view(np.uint32)
    run_buf = np.zeros(max(depth - 1, 1) * 16, dtype=np.uint32)
    adv = np.zeros((sy.N_ADVICE, n, 8), dtype=np.uint32)
    inst = np.zeros((4, 8), dtype=np.uint32)
    lib.hc_merkle_sum_witness.restype = ctypes.c_int
    lib.hc_merkle_sum_witness.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, u32p, u32p,
                                          ctypes.POINTER(ctypes.c_uint64), u32p, u32p, u32p, u32p, u32p]
    rc = lib.hc_merkle_sum_witness(p(consts), spec.r_f, spec.r_p, depth, lay.k, 1, p(leaves), p(sib),
                                   idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), p(a), None, p(run_buf), p(adv), p(inst))
    assert rc == 0
    return [ps.words_to_ints(col.view(np.uint64)) for col in adv], ps.words_to_ints(inst.view(np.uint64))
