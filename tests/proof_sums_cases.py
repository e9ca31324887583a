"""Synthetic inputs of the per-proof sums (csrc/verify_sums.inc) with a cheap oracle, shared by tests/test_proof_sums_host.py and
tests/test_verdicts_gpu.py.  Every base is k * G for a small k, built by repeated addition on host integers; 0 stands for the (0, 0)
base.  The expected rows are then L = (h2_l * k_tail mod r) * G and R = (sum_j s_j * k_j mod r) * G: one ``g1_mul`` each per proof.
A few scalars per proof are full width -- r - 1 and 1 among them --, the rest 16 bits, so that a term costs a few doublings."""
import random

import numpy as np

from halo2_experiments_amd.bn256 import fr_array, g1_words
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.pairing import G1_GEN, g1_add, g1_mul, g1_neg

T_LIST = [1, 2, 3, 63, 64, 65, 127, 128, 129, 300]       # terms of R: own + shared + 1; 300 runs the strided loop more than once
SPECIALS = ["double", "cancel", "zero scalar", "zero base", "all zero"]
# rows whose equal partial sums stand in lanes t and t + off when the fold's step off runs, so that vs_fold_step's g1_add doubles:
# name -> the (own, shared) it is built for (128 lanes; every lane holds at most one term)
FOLD_DOUBLINGS = {"fold double at 64": (100, 2), "fold double at 1": (2, 0), "fold double, other z": (2, 0)}
SHARED_K0, TAIL_K0 = 400, 801                            # shared base i is (400 + i) G, proof b's tail (801 + b) G; own bases lie below
_multiples = [None, G1_GEN]


def multiple(k: int):
    """k * G for a small k >= 0 by repeated addition (None for k = 0), remembered"""
    while len(_multiples) <= k:
        _multiples.append(g1_add(_multiples[-1], G1_GEN))
    return _multiples[k]


def splits(T: int):
    """(own, shared) with own + shared + 1 == T: all own, all shared, and both"""
    n = T - 1
    return sorted({(n, 0), (0, n), (n // 2, n - n // 2)})


def make_proof(rng, b: int, own: int, shared: int, special=None):
    """one proof's bases (as multiples of G) and scalars; ``special`` bends its first own terms, see SPECIALS"""
    own_k = [1 + j + 3 * (b % 16) for j in range(own)]                     # distinct within the proof
    scalars = [rng.randrange(1, 1 << 16) for _ in range(own + shared + 2)]  # own, shared, h2_r, h2_l
    wide = [R - 1, 1, rng.randrange(R), rng.randrange(R)]
    for at, v in zip(rng.sample(range(len(scalars)), min(len(wide), len(scalars))), wide):
        scalars[at] = v
    own_s, shared_s, h2r, h2l = scalars[:own], scalars[own:own + shared], scalars[-2], scalars[-1]
    if special == "double":                                              # equal terms 0, 1, 64, 128: lane 0 doubles in its own loop when it
        for j in (1, 64, 128):                                           # meets term 128; in the fold lane 0 has taken other terms in before
            if j < own:                                                  # it meets lane 1 or 64, so the FOLD doubles in FOLD_DOUBLINGS only
                own_k[j], own_s[j] = own_k[0], own_s[0]
    elif special == "fold double at 64":                                 # lanes 0 and 64 hold the same single term at the first step
        assert 65 <= own and own + shared + 1 <= 128
        own_k[64], own_s[64] = own_k[0], own_s[0]
    elif special == "fold double at 1":                                  # lanes 0 and 1 equal, lane 2 (h2_r) the identity: they meet at the last step
        assert (own, shared) == (2, 0)
        own_k[1], own_s[1], h2r = own_k[0], own_s[0], 0
    elif special == "fold double, other z":                              # 2s (k G) beside s (2k G): one point, two Jacobian forms
        assert (own, shared) == (2, 0)
        s = rng.randrange(1, 1 << 16)
        own_k[1], own_s[0], own_s[1], h2r = 2 * own_k[0], 2 * s, s, 0
    elif special == "cancel":                                            # s and r - s on one base; the other terms keep the sum alive
        own_k[1], own_s[1] = own_k[0], (R - own_s[0]) % R
    elif special == "zero scalar":
        own_s[0] = 0
        if own > 64:
            own_s[64] = 0
    elif special == "zero base":
        own_k[0] = 0
        if own > 65:
            own_k[65] = 0
    elif special == "all zero":
        own_s, shared_s, h2r, h2l = [0] * own, [0] * shared, 0, 0
    elif special is not None:
        raise ValueError(special)
    return dict(own_k=own_k, own_s=own_s, shared_s=shared_s, h2r=h2r, h2l=h2l)


def build(B: int, own: int, shared: int, seed, specials=None, bad=()):
    """A batch in the layout of ``hm_verify_proof_sums_dev``: bases (B own + shared + B, 8), own (B own, 4), shared (B, shared, 4),
    h2_r / h2_l (B, 4) uint64, bad (B,) uint32, and ``expect`` (B, 2, 8): the rows the kernel must write, bit for bit.
    ``specials``: {proof index: one of SPECIALS}; ``bad``: the proofs flagged on entry (zero rows whatever they hold)."""
    rng = random.Random(f"proof-sums {B} {own} {shared} {seed}")
    specials = specials or {}
    proofs = [make_proof(rng, b, own, shared, specials.get(b)) for b in range(B)]
    shared_k = [SHARED_K0 + i for i in range(shared)]
    tail_k = [TAIL_K0 + b for b in range(B)]
    ks = [k for p in proofs for k in p["own_k"]] + shared_k + tail_k
    bases = np.stack([g1_words(multiple(k)) for k in ks]) if ks else np.zeros((0, 8), dtype=np.uint64)
    expect = np.zeros((B, 2, 8), dtype=np.uint64)
    for b, p in enumerate(proofs):
        if b in bad:
            continue
        total = sum(s * k for s, k in zip(p["own_s"], p["own_k"])) + sum(s * k for s, k in zip(p["shared_s"], shared_k)) + p["h2r"] * tail_k[b]
        expect[b, 0] = g1_words(g1_mul(p["h2l"] * tail_k[b] % R))
        expect[b, 1] = g1_words(g1_neg(g1_mul(total % R)))
    words = lambda values, shape: fr_array(values).reshape(shape) if values else np.zeros(shape, dtype=np.uint64)
    flags = np.zeros(B, dtype=np.uint32)
    flags[list(bad)] = 1
    return dict(B=B, own=own, shared=shared, bases=np.ascontiguousarray(bases),
                own_s=words([s for p in proofs for s in p["own_s"]], (B * own, 4)),
                shared_s=words([s for p in proofs for s in p["shared_s"]], (B, shared, 4)),
                h2r=words([p["h2r"] for p in proofs], (B, 4)), h2l=words([p["h2l"] for p in proofs], (B, 4)), bad=flags, expect=expect)
