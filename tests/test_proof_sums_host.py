"""The per-proof sums without a GPU: the kernel's lane, fold and finish functions (csrc/verify_sums.inc) built on the host with bound
tracking (``hc_verify_proof_sums``: a violated bound aborts the process) against the oracle of tests/proof_sums_cases.py, bit for bit --
every term count around the workgroup's 128 lanes, split into own and shared points every way, the rows that meet a doubling (in a
lane, and -- counted by the twin -- in the fold), a cancellation, a zero scalar, a (0, 0) base, and flagged proofs; the two
double-and-add loops of csrc/g1_mul.h against each other; ``proof_sums_ints`` on the golden proofs through the trapdoor; and the
refusals of ``hm_verify_proof_sums_dev``, which come before a device is needed."""
import ctypes
import os
import random

import numpy as np
import pytest

from halo2_experiments_amd import _lib, batch_verifier as bvm, poseidon as ps
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.bn256 import g1_words
from halo2_experiments_amd.pairing import g1_mul

import proof_sums_cases as sc
import prover_cases as pc
from conftest import GOLDEN

u32p = ctypes.POINTER(ctypes.c_uint32)
HM_ERR_BAD_ARG = -1
LANES = 128                                                                  # VS_THREADS of csrc/verify_sums.inc


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_verify_proof_sums.restype = ctypes.c_int
    lib.hc_verify_proof_sums.argtypes = [u32p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p, u32p, ctypes.c_size_t,
                                         ctypes.c_uint32, u32p, u32p]
    lib.hc_g1_mul_words_pair.restype = ctypes.c_int
    lib.hc_g1_mul_words_pair.argtypes = [u32p, u32p, u32p]
    return lib


def host_rows(hc, case, lanes=LANES, doublings=None):
    """every proof of the batch through the host twin -> (B, 2, 8) uint64; ``doublings``: a list that receives, per proof, how many
    steps of the fold added two equal points"""
    ptr = lambda a: np.ascontiguousarray(a).ctypes.data_as(u32p)
    keep = [np.ascontiguousarray(case[key]) for key in ("bases", "own_s", "shared_s", "h2r", "h2l", "bad")]
    out = np.zeros((case["B"], 2, 8), dtype=np.uint64)
    for b in range(case["B"]):
        row, count = np.full(32, 0xFFFFFFFF, dtype=np.uint32), ctypes.c_uint32(0)
        rc = hc.hc_verify_proof_sums(ptr(keep[0]), case["B"], case["own"], case["shared"], ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                     ptr(keep[5]), b, lanes, row.ctypes.data_as(u32p), ctypes.byref(count))
        assert rc == 0
        if doublings is not None:
            doublings.append(count.value)
        out[b] = row.view(np.uint64).reshape(2, 8)
    return out


@pytest.mark.parametrize("T", sc.T_LIST)
def test_synthetic_sums_equal_the_oracle(hc, T):
    for own, shared in sc.splits(T):
        case = sc.build(2, own, shared, seed=T)
        assert np.array_equal(host_rows(hc, case), case["expect"]), (own, shared)


def test_the_result_does_not_depend_on_the_fold(hc):
    case = sc.build(1, 40, 30, seed="fold")
    for lanes in (2, 8, 64, 256):
        assert np.array_equal(host_rows(hc, case, lanes), case["expect"]), lanes


@pytest.mark.parametrize("special", sc.SPECIALS)
@pytest.mark.parametrize("own,shared", [(2, 0), (5, 3), (130, 2)])
def test_rows_with_special_terms(hc, special, own, shared):
    case = sc.build(2, own, shared, seed=special, specials={0: special})
    got = host_rows(hc, case)
    assert np.array_equal(got, case["expect"])
    if special == "all zero":
        assert not got[0].any() and got[1].any()
    else:
        assert got[0, 1].any()                                                # the partner terms keep the sum off the identity


@pytest.mark.parametrize("special", sorted(sc.FOLD_DOUBLINGS))
def test_the_fold_meets_a_doubling(hc, special):
    """equal partial sums in lanes t and t + off when step off runs: the twin counts the steps that took g1_add's doubling branch, so
    the rows are known to reach it (the rows of "double" do not: there lane 0 has taken other terms in before it meets its equal)"""
    own, shared = sc.FOLD_DOUBLINGS[special]
    case = sc.build(3, own, shared, seed=special, specials={0: special, 2: special})
    counts = []
    got = host_rows(hc, case, doublings=counts)
    assert np.array_equal(got, case["expect"]) and got[0, 1].any() and got[2, 1].any()
    assert counts == [1, 0, 1]
    plain = []
    host_rows(hc, sc.build(1, 130, 2, seed="double", specials={0: "double"}), doublings=plain)
    assert plain == [0]


def test_the_two_double_and_add_loops_agree(hc):
    """g1_mul_words and its field-by-field twin (csrc/g1_mul.h) on the same bases and integers: the same limbs, and the oracle's point"""
    rng = random.Random("g1_mul_words")
    scalars = [0, 1, 2, 3, R - 1, R, R + 1, 2 ** 256 - 1, 1 << 255, 0xFFFF] + [rng.randrange(2 ** 256) for _ in range(6)] + \
        [rng.randrange(1 << 16) for _ in range(4)]
    for i, e in enumerate(scalars):
        k = 1 + i % 5
        base = np.ascontiguousarray(g1_words(sc.multiple(k))).view(np.uint32)
        words = np.frombuffer(e.to_bytes(32, "little"), dtype=np.uint32).copy()
        row = np.zeros(16, dtype=np.uint32)
        assert hc.hc_g1_mul_words_pair(base.ctypes.data_as(u32p), words.ctypes.data_as(u32p), row.ctypes.data_as(u32p)) == 1, e
        assert np.array_equal(row.view(np.uint64), g1_words(g1_mul(e * k % R))), e


def test_a_cancelling_pair_alone_gives_the_identity(hc):
    case = sc.build(1, 2, 0, seed="cancel alone", specials={0: "cancel"})
    case["h2r"][:] = 0                                                       # no partner: R = s P - s P
    case["expect"][0, 1] = 0
    got = host_rows(hc, case)
    assert np.array_equal(got, case["expect"]) and got[0, 0].any() and not got[0, 1].any()


def test_flagged_proofs_get_zero_rows(hc):
    case = sc.build(3, 5, 2, seed="bad", bad=(1,))
    got = host_rows(hc, case)
    assert np.array_equal(got, case["expect"]) and not got[1].any() and got[0].any() and got[2].any()


# ---- the integer twin on the golden proofs ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("poseidon_k6", "poseidon_k6"), ("merkle_sum_d5_k9", "merkle_sum_k9")], ids=lambda p: p[1])
def golden_proof(request):
    name, short = request.param
    cs, k = pc.constraint_system(name)
    meta = np.load(os.path.join(GOLDEN, f"proof_{short}.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, f"proof_{short}.bin"), "rb").read()
    return vk, ps.words_to_ints(meta["instance"]), proof, bvm.ProofLayout(cs, k)


def holds(vk, instance, proof, lay, weight=1):
    left, right = bvm.proof_sums_ints(vk, instance, proof, lay, weight)
    return g1_mul(pc.SRS_S, left) == right


def test_integer_twin_through_the_trapdoor(golden_proof):
    vk, instance, proof, lay = golden_proof
    assert holds(vk, instance, proof, lay)
    assert bvm.proof_sums_ints(vk, instance, proof) == bvm.proof_sums_ints(vk, instance, proof, lay)      # the layout is optional
    at = 32 * lay.points_before_evals + 32 * 3 + 1
    flipped = proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:]
    assert not holds(vk, instance, flipped, lay)
    wrong = list(instance)
    wrong[-1] = (wrong[-1] + 1) % R
    assert not holds(vk, wrong, proof, lay)
    weight = random.Random(17).randrange(1, R)
    assert holds(vk, instance, proof, lay, weight) and not holds(vk, instance, flipped, lay, weight)
    one, weighted = bvm.proof_sums_ints(vk, instance, proof, lay), bvm.proof_sums_ints(vk, instance, proof, lay, weight)
    assert weighted == (g1_mul(weight, one[0]), g1_mul(weight, one[1]))


def test_an_empty_batch_and_an_unknown_method_need_no_device(golden_proof):
    import halo2_experiments_amd as h

    vk = golden_proof[0]
    bv = h.BatchVerifier(None, vk)
    assert bv.verdicts() == [] and bv.failing(method="each") == [] and bv.failing() == [] and bv.sums_calls == 0
    assert tuple(bv.proof_sums().shape) == (0, 2, 8) and bv.sums_calls == 0
    assert h.verify_each(None, vk, [], []) == []
    with pytest.raises(ValueError):
        bv.failing(method="all")
    with pytest.raises(ValueError):
        h.verify_each(None, vk, [[1]], [])


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    lib = _lib.load()
    assert "hm_verify_proof_sums_dev" in _lib._SIGNATURES
    vp = ctypes.c_void_p
    p16, p4 = vp(0x1000), ctypes.cast(vp(0x2000), u32p)
    base = dict(bases=p16, n=2, own=3, shared=2, own_s=p16, shared_s=p16, h2r=p16, h2l=p16, bad=p4, pairs=p16, stream=None)
    order = ("bases", "n", "own", "shared", "own_s", "shared_s", "h2r", "h2l", "bad", "pairs", "stream")
    call = lambda **kw: lib.hm_verify_proof_sums_dev(*[dict(base, **kw)[key] for key in order])
    cases = [(dict([(key, None)]), b"null") for key in ("bases", "own_s", "shared_s", "h2r", "h2l", "bad", "pairs")]
    cases += [(dict(n=0), b"n_proofs"), (dict(n=(1 << 20) + 1), b"n_proofs"), (dict(own=0, shared=0), b"own_points + shared_points"),
              (dict(own=1 << 16, shared=1), b"own_points + shared_points"), (dict(own=0xFFFFFFFF, shared=1), b"own_points + shared_points")]
    cases += [(dict([(key, vp(0x1008))]), b"16-byte") for key in ("bases", "own_s", "shared_s", "h2r", "h2l", "pairs")]
    cases += [(dict(bad=ctypes.cast(vp(0x2002), u32p)), b"4-byte")]
    for kw, why in cases:
        assert call(**kw) == HM_ERR_BAD_ARG and why in lib.hm_last_error(), kw
