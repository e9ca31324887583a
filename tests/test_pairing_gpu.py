"""GPU suite of the device pairing (``device_pairing``, csrc/pairing.inc).  The Python oracle costs tens of milliseconds per pairing,
so fewer than 40 pairs are compared with it; the rest is covered by properties whose outcome is known without it."""
import ctypes

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, device_pairing as dp, openings as op
from halo2_experiments_amd import pairing as pr
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fq_array, fr_ints, fr_words
from halo2_experiments_amd.kzg import ParamsKZG, g2_mul

import prover_cases as pc

pytestmark = pytest.mark.gpu
P = pr.P
G1, G2 = pr.G1_GEN, pr.G2_GENERATOR
SCALARS = [(3, 5), (0x1234567, 0x89ABCDEF0123), (R - 2, 7), (11, R - 3), (2 ** 200 + 9, 2 ** 100 + 1)]


@pytest.fixture(scope="module")
def points():
    """a few ([a]G1, [b]G2, [-ab]G1, [-ab + 1]G1): computed once, shared by every test"""
    out = []
    for a, b in SCALARS:
        out.append(dict(a=a, b=b, pa=pr.g1_mul(a), qb=g2_mul(b), cancel=pr.g1_mul(-a * b % R), near=pr.g1_mul((-a * b + 1) % R)))
    return out


def oracle_value(pairs):
    f = pr.F12_ONE
    for a, b in pairs:
        f = pr.f12_mul(f, pr.miller_loop(a, b))
    return pr.final_exponentiation(f)


def test_one_check_of_one_pair_equals_the_oracle(points):
    pt = points[1]
    assert dp.pairing_values([[(pt["pa"], pt["qb"])]]) == [pr.pairing(pt["pa"], pt["qb"])]
    assert dp.pairing_check([(pt["pa"], pt["qb"])]) is False


def test_a_kzg_relation_of_two_pairs():
    """a tiny trapdoor SRS: f(s), the quotient's q(s) and z chosen, y = f(s) - q(s)(s - z); e(pi, [s]G2) e(-(C - [y]G + [z]pi), G2) = 1"""
    s, fs, qs, z = 0xC0FFEE, 123456789, 987654321, 42
    y = (fs - qs * (s - z)) % R
    c, pi, s_g2 = pr.g1_mul(fs), pr.g1_mul(qs), g2_mul(s)
    rhs = pr.g1_add(pr.g1_add(c, pr.g1_neg(pr.g1_mul(y))), pr.g1_mul(z, pi))
    good = [(pi, s_g2), (pr.g1_neg(rhs), G2)]
    assert dp.run([good]) == ([1], None) and pr.pairing_check(good)
    assert dp.pairing_check(good) is True
    wrong = [(pr.g1_add(pi, G1), s_g2), (pr.g1_neg(rhs), G2)]           # one point moved
    assert dp.pairing_checks([good, wrong, good]) == [True, False, True]


def test_bilinearity_on_the_device_alone(points):
    pt = points[4]
    ab = pr.g1_mul(pt["a"] * pt["b"] % R)
    both, one_side, twice = dp.pairing_values([[(pt["pa"], pt["qb"])], [(ab, G2)], [(G1, G2), (G1, G2)]])
    assert both == one_side and both != pr.F12_ONE
    assert twice != pr.F12_ONE and twice != both


def segmented_checks(points):
    """130 checks whose pair counts cycle through 0, 1, 2, 3 (193 pairs: both cross a 64-lane block and leave a ragged tail), each
    with its known status"""
    checks, want = [], []
    off_g1 = (points[0]["pa"][0], (points[0]["pa"][1] + 1) % P)
    qb0 = points[0]["qb"]
    off_g2 = (qb0[0], ((qb0[1][0] + 1) % P, qb0[1][1]))
    for c in range(130):
        pt = points[c % len(points)]
        count = c % 4
        fails, malformed = c % 7 == 3, c in (5, 63, 64, 66, 129)
        pairs = [(pt["pa"], pt["qb"]), (pt["near"] if fails else pt["cancel"], G2), (None, pt["qb"]) if c % 8 == 3 else (pt["pa"], None)][:count]
        status = 1 if count == 0 else 0 if count == 1 or fails else 1
        if malformed and count:
            where = c % count
            pairs[where] = (off_g1, pairs[where][1]) if c % 2 else (pairs[where][0], off_g2)
            status = 2
        checks.append(pairs)
        want.append(status)
    return checks, want


def test_segmentation_over_130_checks(points):
    checks, want = segmented_checks(points)
    assert [len(c) for c in checks[:5]] == [0, 1, 2, 3, 0] and sum(len(c) for c in checks) == 193
    assert {0, 1, 2} == set(want) and want.count(2) == 4
    status, gt = dp.run(checks, want_gt=True)
    assert status == want
    one = np.ascontiguousarray(fq_array([1] + [0] * 11).reshape(-1))
    for c, s in enumerate(status):
        assert np.array_equal(gt[c], one) == (s == 1) and gt[c].any() == (s != 2)
    with pytest.raises(ValueError):
        dp.pairing_checks(checks)
    picked = [1, 2, 3, 70, 127]                                          # 1 + 2 + 3 + 2 + 3 = 11 pairs through the oracle
    assert all(want[c] != 2 for c in picked)
    assert dp.pairing_values([checks[c] for c in picked]) == [oracle_value(checks[c]) for c in picked]
    for c, v in zip(picked, dp.pairing_values([checks[c] for c in picked])):
        assert fq_array([x for six in v for two in six for x in two]).reshape(-1).tolist() == gt[c].tolist()


def test_identity_pairs_in_every_position(points):
    pt = points[2]
    live = [(pt["pa"], pt["qb"]), (pt["cancel"], G2)]
    checks = [[(None, G2)] + live, [live[0], (G1, None), live[1]], live + [(None, None)], [live[0], (None, pt["qb"])], [(None, G2)]]
    assert dp.pairing_checks(checks) == [True, True, True, False, True]
    values = dp.pairing_values(checks)
    assert values[0] == values[1] == values[2] == values[4] == pr.F12_ONE
    assert values[3] == dp.pairing_values([[live[0]]])[0]


def test_every_bad_argument_returns_without_launching():
    lib = _lib.load()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    f32, odd32 = ctypes.cast(fake, u32p), ctypes.cast(ctypes.c_void_p(0x1002), u32p)
    need = lib.hm_pairing_work_bytes(2, 1)
    assert need == 4 * (3 * 96 * 2 + 2 + 11 * 96) and lib.hm_pairing_work_bytes(0, 1) == 4 * 11 * 96
    assert lib.hm_pairing_work_bytes(1, 0) == 0 and lib.hm_pairing_work_bytes(1, (1 << 20) + 1) == 0 and lib.hm_pairing_work_bytes((1 << 24) + 1, 1) == 0
    call = lambda g1=fake, g2=fake, n_pairs=2, off=f32, n_checks=1, gt=None, status=f32, work=fake, work_bytes=need: \
        lib.hm_pairing_check_bn256_dev(g1, g2, n_pairs, off, n_checks, gt, status, work, work_bytes, None)
    for bad in (dict(g1=None), dict(g2=None), dict(off=None), dict(status=None), dict(work=None), dict(n_checks=0),
                dict(n_checks=(1 << 20) + 1, work_bytes=1 << 40), dict(n_pairs=(1 << 24) + 1, work_bytes=1 << 40), dict(work_bytes=need - 1),
                dict(g1=odd), dict(g2=odd), dict(gt=odd), dict(work=odd), dict(off=odd32), dict(status=odd32)):
        assert call(**bad) == _lib.HM_ERR_BAD_ARG and b"hm_pairing_check_bn256_dev" in lib.hm_last_error(), bad


# ---- the opt-in keyword of the verifiers -----------------------------------------------------------------------------------------
def test_batch_verifier_with_the_pairing_on_the_device():
    """Poseidon k = 6 proofs, as tests/test_batch_verifier_gpu.py makes them: accept and reject agree with the host pairing"""
    cs, lay, advice, instance, _ = pc.build("poseidon_k6")
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    try:
        vk = h.keygen_vk(params, cs, lay)
        pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
        proofs = [(instance, h.create_proof(params, pk, advice, instance, seed)) for seed in (7, 8)]
        assert h.verify_proofs(params, vk, [i for i, _ in proofs], [p for _, p in proofs], seed=5, pairing="device")
        from halo2_experiments_amd.batch_verifier import ProofLayout

        tampered = bytearray(proofs[1][1])
        tampered[32 * ProofLayout(cs, lay.k).points_before_evals + 32 * 3 + 1] ^= 1      # an evaluation: still a scalar below r
        members = [proofs[0], (instance, bytes(tampered))]
        results = {}
        for mode in ("host", "device"):
            bv = h.BatchVerifier(params, vk, seed=5, pairing=mode)
            for inst, proof in members:
                bv.add_proof(inst, proof)
            results[mode] = (bv.finalize(), bv.failing())
            assert bv.timings["pairing"] > 0
        assert results["device"] == results["host"] and results["host"][0] is False
        with pytest.raises(ValueError):
            h.BatchVerifier(params, vk, pairing="gpu")
    finally:
        params.release()


def test_verify_openings_with_the_pairing_on_the_device():
    """open_all at k = 4: accept, a wrong value, and a single opening"""
    k, n = 4, 16
    params = ParamsKZG.setup(k, pc.SRS_S, keep_points=True)
    try:
        poly = h.random_fr(n, 55, "cuda")
        evals = poly.clone()
        h.best_fft(evals, fr_words(op.domain_omega(k)), k)
        values = fr_ints(evals.cpu().numpy().view(np.uint64))
        c, proofs = params.commit(poly), op.open_all(params, poly)
        idx = list(range(n))
        wrong = list(values)
        wrong[5] = (wrong[5] + 1) % R
        for vals in (values, wrong):
            got = {mode: op.verify_openings(params, c, idx, vals, proofs, seed=b"openings", pairing=mode) for mode in ("host", "device")}
            assert got["device"] == got["host"] == (vals is values)
        w = op.domain_omega(k)
        one = proofs.cpu().numpy().view(np.uint64)[3]
        assert op.verify_opening(params, c, pow(w, 3, R), values[3], one, pairing="device")
        assert not op.verify_opening(params, c, pow(w, 3, R), values[4], one, pairing="device")
        with pytest.raises(ValueError):
            op.verify_opening(params, c, pow(w, 3, R), values[3], one, pairing="gpu")
    finally:
        params.release()
