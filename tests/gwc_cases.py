"""What the tests of the GWC multiopen share (tests/test_gwc_host.py, tests/test_gwc_gpu.py, tests/golden/gen_golden_gwc_proofs.py): the
four systems at the smallest shapes the suite uses (tests/mutation_cases.py builds them: Poseidon k = 6, MerkleTreeV3 depth 2 / k = 7,
MerkleSumTree depth 2 / k = 9 -- lookups, hence rotation -1 --, OverflowCheckV2<4, 4> k = 5), the recorded proofs, random records for
the terms kernel with what the integer twin answers, and the host twin ``hc_verify_terms_gwc``.  This file imports no torch."""
import ctypes
import os
import random

import numpy as np

from halo2_experiments_amd import _lib, poseidon as ps, proof_layout as pl
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array, fr_ints
from halo2_experiments_amd.domain import EvaluationDomain
from halo2_experiments_amd.keygen import VerifyingKey

import mutation_cases as mc

SYSTEMS = list(mc.NAMES)                        # poseidon, merkle_v3, merkle_sum_tree, overflow_check_v2
ENCODINGS = ("halo2", "evm")
GOLDEN_SEED = 20230202
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
u32p = ctypes.POINTER(ctypes.c_uint32)


def golden_path(name: str) -> str:
    return os.path.join(GOLDEN, f"gwc_proofs_{name}.npz")


def instance_of(words) -> list:
    """the instance in the form ``create_proof`` takes, from the recorded words: [[]] for a system whose instance column is empty"""
    values = ps.words_to_ints(np.asarray(words, dtype=np.uint64).reshape(-1, 4))
    return values if values else [[]]


def recorded(name: str) -> dict:
    """the recorded proofs of one system: vk (host only), instance, seed, and proof bytes by (multiopen, encoding)"""
    c = mc.case(name)
    meta = np.load(golden_path(name))
    vk = VerifyingKey(EvaluationDomain(c.cs.degree(), c.k), c.cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proofs = {(mo, enc): meta[f"{mo}_{enc}"].tobytes() for mo in ("gwc", "shplonk") for enc in ENCODINGS}
    return dict(case=c, vk=vk, instance=instance_of(meta["instance"]), seed=int(meta["seed"]), proofs=proofs)


def layout(name: str, encoding: str = "halo2") -> pl.ProofLayout:
    c = mc.case(name)
    return pl.ProofLayout(c.cs, c.k, encoding, multiopen="gwc")


def plan_of(name: str, rows: int = None):
    """(layout, GwcTermsPlan, omega) of a system, every instance column ``rows`` long (the rows the circuit uses when None)"""
    c = mc.case(name)
    lay = layout(name)
    omega = EvaluationDomain(c.cs.degree(), c.k).omega
    return lay, pl.GwcTermsPlan(lay, omega, [c.inst_rows if rows is None else rows] * c.cs.num_instance), omega


# ---- records no transcript produces ------------------------------------------------------------------------------------------------------
def record(lay: pl.ProofLayout, rows: int, rng: random.Random, **change):
    """(ch, r_b, evals, inst_cols): uniform below r but for ``change`` (a challenge by name, or rb)"""
    ch = {name: rng.randrange(R) for name in pl.GWC_RECORD}
    rb = change.pop("rb", rng.randrange(1, R))
    ch.update(change)
    return ch, rb, [rng.randrange(R) for _ in range(lay.n_scalars)], [[rng.randrange(R) for _ in range(rows)] for _ in range(lay.cs.num_instance)]


def expected(lay: pl.ProofLayout, omega: int, case):
    """-> ((own, shared, w_left) as the kernel must write them, or None where the twin raises ``MalformedProof``, numerator or None)"""
    ch, rb, evals, inst_cols = case
    details = {}
    try:
        own, shared, left = pl.terms_from_challenges(lay, omega, inst_cols, evals, ch, details)
    except pl.MalformedProof:
        return None, details.get("numerator")
    scale = lambda values: [rb * v % R for v in values]
    return (scale(own), scale(shared), scale(left)), details["numerator"]


# ---- the host twin (libhm_hostcheck.so, bound tracking on) --------------------------------------------------------------------------------
def hostcheck():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_verify_terms_gwc.restype = ctypes.c_int
    lib.hc_verify_terms_gwc.argtypes = [u32p, ctypes.c_size_t, ctypes.c_size_t] + [u32p] * 8 + [ctypes.POINTER(ctypes.c_char_p)]
    return lib


def terms_on_the_host(hc, words, n_columns, n_vals, lay, rec, evals, inst_row, numerator):
    """``hc_verify_terms_gwc`` on one record -> (rc, why, own, shared, w_left) as integers"""
    w = lambda values: np.ascontiguousarray(fr_array(values)).view(np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rec_w, ev_w, iw, num = w(rec), w(evals), w(inst_row), w([numerator])
    vals, own = np.zeros((max(n_vals, 1), 8), dtype=np.uint32), np.zeros((lay.own_points, 8), dtype=np.uint32)
    shared, left = np.zeros((len(lay.shared_keys), 8), dtype=np.uint32), np.zeros((len(lay.groups), 8), dtype=np.uint32)
    why = ctypes.c_char_p()
    rc = hc.hc_verify_terms_gwc(p(words), len(words), n_columns, p(rec_w), p(ev_w), p(iw), p(num), p(vals), p(own), p(shared), p(left),
                                ctypes.byref(why))
    ints = lambda a: fr_ints(a.view(np.uint64))
    return rc, why.value, ints(own), ints(shared), ints(left)
