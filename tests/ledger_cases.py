"""Shared by tests/test_ledger_host.py and tests/test_ledger_gpu.py: a tiny ledger on host integers through the trapdoor, the oracle of
one user's pairing operands, and the call of the host twin ``hc_ledger_pair`` (csrc/ledger.inc under bound tracking)."""
import ctypes
import random

import numpy as np

from halo2_experiments_amd import _lib, ledger as lg
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_words, g1_words
from halo2_experiments_amd.kzg import G2_GENERATOR, g2_bytes, g2_mul
from halo2_experiments_amd.openings import domain_omega
from halo2_experiments_amd.pairing import G1_GEN, g1_add, g1_mul, g1_neg

u32p = ctypes.POINTER(ctypes.c_uint32)
S = 0x1234567890ABCDEF1234567 % R                 # the trapdoor of tests/test_openings_host.py


class Params:
    """what the host verifiers read of a ParamsKZG"""

    def __init__(self, s, k):
        self.g2, self.s_g2, self.k, self.n = g2_bytes(G2_GENERATOR), g2_bytes(g2_mul(s)), k, 1 << k


def lagrange_at(k, s):
    """L_i(s) for the domain of size 2^k: (s^n - 1) omega^i / (n (s - omega^i))"""
    n, w = 1 << k, domain_omega(k)
    z = (pow(s, n, R) - 1) * pow(n, -1, R) % R
    return [z * pow(w, i, R) * pow(s - pow(w, i, R), -1, R) % R for i in range(n)]


def int_ledger(k, assets, seed, s=S, users=None):
    """ids, balances and every public and per-user value of a ledger of 2^k rows (the last 6 zero), by the definitions"""
    rng = random.Random(f"ledger {k} {assets} {seed}")
    n = 1 << k
    users = n - 6 if users is None else users
    ids = [rng.randrange(1, R) for _ in range(users)] + [0] * (n - users)
    bal = [[rng.randrange(1 << 16) for _ in range(users)] + [0] * (n - users) for _ in range(assets)]
    lag = lagrange_at(k, s)
    at_s = lambda col: sum(v * l for v, l in zip(col, lag)) % R
    c_id, cs = g1_mul(at_s(ids), G1_GEN), [g1_mul(at_s(col), G1_GEN) for col in bal]
    gamma = lg.ledger_gamma(k, c_id, cs)
    g = [lg.combined_value(gamma, ids[i], [col[i] for col in bal]) for i in range(n)]
    w = domain_omega(k)
    openings = [g1_mul((at_s(g) - g[i]) * pow(s - pow(w, i, R), -1, R) % R, G1_GEN) for i in range(n)]
    return dict(k=k, n=n, P=assets, ids=ids, bal=bal, c_id=c_id, cs=cs, gamma=gamma, g=g, openings=openings,
                c_gamma=lg.combined_commitment(gamma, c_id, cs), params=Params(s, k))


def expected_rows(k, gamma, c_gamma, index, user_id, balances, opening):
    """(pi, -R) as (2, 8) words, R = C_gamma + [r - y]G + [omega^i]pi on host integers"""
    y = lg.combined_value(gamma, user_id, balances)
    rhs = g1_add(g1_add(c_gamma, g1_mul((R - y) % R, G1_GEN)), g1_mul(pow(domain_omega(k), index, R), opening))
    return np.stack([g1_words(opening), g1_words(g1_neg(rhs))])


def load_twin():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_ledger_pair.restype = ctypes.c_int
    lib.hc_ledger_pair.argtypes = [u32p, u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p, u32p]
    return lib


def twin_rows(hc, k, gamma, c_gamma, index, id_words, balance_words, opening_words):
    """one user through ``hc_ledger_pair``: the words as the kernel reads them -> (flag, (2, 8) uint64 rows)"""
    keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in (fr_words(gamma), fr_words(domain_omega(k)), g1_words(c_gamma), opening_words,
                                                               id_words, np.asarray(balance_words, dtype=np.uint64).reshape(-1, 4))]
    ptr = lambda a: a.ctypes.data_as(u32p)
    rows = np.full(32, 0xFFFFFFFF, dtype=np.uint32)
    flag = hc.hc_ledger_pair(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), k, len(keep[5]), ptr(keep[3]), index, ptr(keep[4]), ptr(keep[5]),
                             rows.ctypes.data_as(u32p))
    return flag, rows.view(np.uint64).reshape(2, 8)


def raw_words(v):
    """the 4 words of the integer v itself (NOT its Montgomery form): for patterns at and above a modulus"""
    return np.array([(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)], dtype=np.uint64)
