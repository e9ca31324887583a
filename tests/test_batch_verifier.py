"""The batch verifier without a GPU, on the golden proofs (tests/golden/gen_golden_proofs.py): the integer twin of the per-proof part gives
the R and the L of ``verify_opening``; the rotation sets taken symbolically on rotations are those of ``construct_intermediate_sets`` on
the real points; the per-slot functions of the read kernel and the step / join / finish of the column-sum kernel, built on the host with
bound tracking (a violated bound aborts the process), give the twins' words, and so do the two phases of the terms kernel around the
interpreter's run, which also flag every zero they would invert; the plan builder and the plan check refuse an instance column of 65
rows, 257 value slots and indices outside their arrays; the randomizers; and the host-side pre-checks report every structural kind of
malformed proof."""
import ctypes
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

from halo2_experiments_amd import _lib, batch_verifier as bvm, poseidon as ps, shplonk, verifier
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, fq_ints, fr_array, fr_ints
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.kzg import G2_GENERATOR, g2_bytes, g2_mul
from halo2_experiments_amd.pairing import g1_msm
from halo2_experiments_amd.transcript import g1_decompress_int

import prover_cases as pc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def params():
    return SimpleNamespace(g2=g2_bytes(G2_GENERATOR), s_g2=g2_bytes(g2_mul(pc.SRS_S)))


@pytest.fixture(scope="module", params=[("poseidon_k6", "poseidon_k6"), ("merkle_sum_d5_k9", "merkle_sum_k9")], ids=lambda p: p[1])
def golden_proof(request):
    name, short = request.param
    cs, k = pc.constraint_system(name)
    meta = np.load(os.path.join(GOLDEN, f"proof_{short}.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, f"proof_{short}.bin"), "rb").read()
    return cs, vk, ps.words_to_ints(meta["instance"]), proof, bvm.ProofLayout(cs, k)


@pytest.fixture(scope="module")
def opening(golden_proof):
    """what verify_proof hands to verify_opening for the golden proof, and what comes back"""
    cs, vk, instance, proof, _ = golden_proof
    seen = {}
    real = verifier.verify_opening

    def spy(transcript, queries, commitments):
        seen["queries"], seen["commitments"] = list(queries), dict(commitments)
        seen["left"], seen["right"] = real(transcript, queries, commitments)
        return seen["left"], seen["right"]

    verifier.verify_opening = spy
    try:
        assert verifier.verify_proof(None, vk, instance, proof, trapdoor=pc.SRS_S)
    finally:
        verifier.verify_opening = real
    return seen


def test_the_twins_terms_sum_to_the_r_of_verify_opening(golden_proof, opening):
    cs, vk, instance, proof, lay = golden_proof
    ch, own, shared, points = bvm.proof_terms_ints(vk, instance, proof, lay)
    assert len(own) == len(points) == lay.n_points and len(shared) == len(lay.shared_keys)
    assert points[-1] == opening["left"]                                     # L is [h']
    assert g1_msm(own + shared, points + bvm.shared_points(vk, lay)) == opening["right"]
    assert all(0 < c < R for c in ch.values())


def test_symbolic_rotation_sets_are_those_of_the_real_points(golden_proof, opening):
    cs, vk, instance, proof, lay = golden_proof
    ch = bvm.proof_terms_ints(vk, instance, proof, lay)[0]
    sets, super_points = shplonk.construct_intermediate_sets(opening["queries"])
    point = lambda rot: ch["x"] * pow(vk.domain.omega, rot, R) % R
    assert len(sets) == len(lay.sets) and super_points == sorted(point(r) for r in lay.super_rotations)
    for (pts, members), (rots, keys) in zip(sets, lay.sets):
        assert pts == sorted(point(r) for r in rots)
        assert [key[:2] if len(key) == 3 else key for key, _ in members] == keys        # verify_proof's keys carry the circuit: (kind, index, 0)


# ---- the kernels' lane functions on the host, under bound tracking -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.hc_verify_read.restype = None
    lib.hc_verify_read.argtypes = [ctypes.c_char_p, u32p, u32p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t]
    lib.hc_verify_column_sum.restype = ctypes.c_int
    lib.hc_verify_column_sum.argtypes = [u32p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, u32p]
    return lib


def hc_read(hc, kinds, slots):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    raw = np.frombuffer(b"".join(slots), dtype=np.uint32).copy()
    out = np.zeros(24 * len(slots), dtype=np.uint32)
    valid = np.zeros(len(slots), dtype=np.int32)
    hc.hc_verify_read(bytes(kinds), raw.ctypes.data_as(u32p), out.ctypes.data_as(u32p), valid.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                      len(slots))
    return out.reshape(len(slots), 3, 8), valid


def test_read_lane_functions_give_the_twins_words(hc, golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    slots = [proof[32 * s:32 * s + 32] for s in range(lay.slots)]
    kinds = [1 if e & bvm.VR_POINT else 0 for e in lay.slot_table]
    out, valid = hc_read(hc, kinds, slots)
    assert valid.all()
    points, scalars = bvm.read_proof_ints(lay, proof)
    got_points = [(fq_ints(out[s, 0].view(np.uint64))[0], fq_ints(out[s, 1].view(np.uint64))[0]) for s in lay.point_slots]
    assert got_points == points
    assert [int.from_bytes(out[s, 2].tobytes(), "little") for s in lay.point_slots] == [y for _, y in points]
    assert [fr_ints(out[s, 0].view(np.uint64))[0] for s in lay.scalar_slots] == scalars


def test_read_lane_functions_refuse_what_the_transcript_refuses(hc):
    le = lambda v: v.to_bytes(32, "little")
    non_residue = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) != 1)
    on_curve = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) == 1)
    cases = [(1, le(P)), (1, le(P + 1)), (1, le(non_residue)), (1, bytes(32)), (1, le(on_curve)), (1, le(on_curve | 1 << 255)),
             (1, le(P - 1 | 1 << 255)), (0, le(R)), (0, le(2 ** 256 - 1)), (0, le(R - 1)), (0, le(0))]
    out, valid = hc_read(hc, [k for k, _ in cases], [s for _, s in cases])
    expected = []
    for kind, data in cases:
        if kind:
            try:
                expected.append(g1_decompress_int(data) is not None)
            except ValueError:
                expected.append(False)
        else:
            expected.append(int.from_bytes(data, "little") < R)
    assert [bool(v) for v in valid] == expected and expected[:4] == [False] * 4 and expected[7:9] == [False, False]
    assert not out[~valid.astype(bool)].any()                               # a refused slot leaves zeros
    for i in (4, 5):
        x, y = g1_decompress_int(cases[i][1])
        assert (fq_ints(out[i, 0].view(np.uint64))[0], fq_ints(out[i, 1].view(np.uint64))[0]) == (x, y)
        assert int.from_bytes(out[i, 2].tobytes(), "little") == y
    assert fr_ints(out[9, 0].view(np.uint64)) == [R - 1]


@pytest.mark.parametrize("rows,cols,lo,hi,lanes", [(1, 1, 0, 1, 256), (65, 3, 1, 65, 256), (300, 2, 0, 300, 256), (300, 2, 64, 257, 4), (5, 2, 3, 3, 256)])
def test_column_sum_lane_functions(hc, rows, cols, lo, hi, lanes):
    rng = random.Random(rows * 31 + lo)
    values = [[rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(cols)] for _ in range(rows)]
    words = np.ascontiguousarray(fr_array(values)).view(np.uint32)
    out = np.zeros((cols, 8), dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert hc.hc_verify_column_sum(words.ctypes.data_as(u32p), rows, cols, lo, hi, lanes, out.ctypes.data_as(u32p)) == 0
    assert fr_ints(out.view(np.uint64)) == [sum(values[r][c] for r in range(lo, hi)) % R for c in range(cols)]


def test_column_sum_at_the_class_maximum(hc):
    """every word all ones -- no Fr element, the largest input the step can meet: the tracked bounds hold and the sum is the integers'"""
    rows, cols = 600, 1
    words = np.full((rows, cols, 8), 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros((cols, 8), dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert hc.hc_verify_column_sum(words.ctypes.data_as(u32p), rows, cols, 0, rows, 256, out.ctypes.data_as(u32p)) == 0
    assert int.from_bytes(out.tobytes(), "little") == rows * (2 ** 256 - 1) % R


# ---- randomizers -----------------------------------------------------------------------------------------------------------------------
def test_randomizers(params, golden_proof):
    cs, vk, instance, proof, _ = golden_proof
    make = lambda seed: bvm.BatchVerifier(params, vk, seed=seed)
    a, b, c, d, e = make(11), make(11), make(12), make(None), make(None)
    for bv in (a, b, c, d, e):
        assert [bv.add_proof(instance, proof) for _ in range(3)] == [0, 1, 2]
        assert all(0 < r < R for r in bv.randomizers) and len(set(bv.randomizers)) == 3
    assert a.randomizers == b.randomizers != c.randomizers
    assert d.randomizers != e.randomizers
    with pytest.raises(AttributeError):
        a.randomizers = ()


def test_empty_batch_is_true(params, golden_proof):
    cs, vk, instance, proof, _ = golden_proof
    assert bvm.BatchVerifier(params, vk).finalize() and bvm.verify_proofs(params, vk, [], []) and bvm.BatchVerifier(params, vk).failing() == []


# ---- the host-side pre-checks ----------------------------------------------------------------------------------------------------------
def test_host_prechecks_report_every_structural_kind(params, golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    first_eval = 32 * lay.points_before_evals
    put = lambda at, data: proof[:at] + data + proof[at + 32:]
    non_residue = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) != 1)
    kinds = {"short": proof[:-32], "long": proof + b"\0", "empty": b"", "scalar = r": put(first_eval, R.to_bytes(32, "little")),
             "x >= p": put(0, P.to_bytes(32, "little")), "off the curve": put(32, non_residue.to_bytes(32, "little")),
             "zero point": put(len(proof) - 32, bytes(32))}
    bv = bvm.BatchVerifier(params, vk, seed=1)
    bv.add_proof(instance, proof)
    for data in kinds.values():
        bv.add_proof(instance, data)
        assert not verifier.verify_proof(params, vk, instance, data, trapdoor=pc.SRS_S)
    bv.add_proof(instance, proof)
    assert bv.malformed() == list(range(1, len(kinds) + 1))                   # the golden proof at both ends is well-formed
    for name, data in kinds.items():
        with pytest.raises(bvm.MalformedProof):
            bvm.proof_terms_ints(vk, instance, data, lay)


def test_x_to_the_n_equal_to_one_is_malformed(golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    ch, own, shared, _ = bvm.proof_terms_ints(vk, instance, proof, lay)
    evals = bvm.read_proof_ints(lay, proof)[1]
    inst_cols = verifier._instance_columns(cs, instance)
    assert bvm.terms_from_challenges(lay, vk.domain.omega, inst_cols, evals, ch) == (own, shared)
    for x in (1, vk.domain.omega, pow(vk.domain.omega, lay.n - 3, R)):
        with pytest.raises(bvm.MalformedProof, match="x\\^n = 1"):
            bvm.terms_from_challenges(lay, vk.domain.omega, inst_cols, evals, dict(ch, x=x))


def test_verify_opening_is_opening_terms_summed(golden_proof, opening):
    """the refactoring of shplonk.verify_opening: the helper's lists, summed, are the R the function returned"""
    cs, vk, instance, proof, lay = golden_proof
    ch, _, _, points = bvm.proof_terms_ints(vk, instance, proof, lay)
    scalars, pts = shplonk.opening_terms(opening["queries"], opening["commitments"], ch["y2"], ch["v"], ch["u"], points[-2], points[-1])
    assert len(scalars) == len(pts) == sum(len(keys) for _, keys in lay.sets) + 3
    assert g1_msm(scalars, pts) == opening["right"]


# ---- the terms kernel's plan and its two phases on the host -----------------------------------------------------------------------------
def terms_on_the_host(hc, plan, lay, record, evals, inst_row, numerator):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    hc.hc_verify_terms.restype = ctypes.c_int
    hc.hc_verify_terms.argtypes = [u32p, ctypes.c_size_t, ctypes.c_size_t] + [u32p] * 9 + [ctypes.POINTER(ctypes.c_char_p)]
    w = lambda values: np.ascontiguousarray(fr_array(values)).view(np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    rec, ev_, iw, num = w(record), w(evals), w(inst_row), w([numerator])
    vals, own = np.zeros((plan.n_vals, 8), dtype=np.uint32), np.zeros((lay.own_points, 8), dtype=np.uint32)
    shared, h2r, h2l = np.zeros((len(lay.shared_keys), 8), dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    why = ctypes.c_char_p()
    rc = hc.hc_verify_terms(p(plan.words), len(plan.words), plan.n_columns, p(rec), p(ev_), p(iw), p(num), p(vals), p(own), p(shared), p(h2r),
                            p(h2l), ctypes.byref(why))
    ints = lambda a: fr_ints(a.view(np.uint64))
    return rc, why.value, ints(vals), ints(own), ints(shared), ints(h2r)[0], ints(h2l)[0]


def test_terms_phases_give_the_twins_words_under_bound_tracking(hc, golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    inst_cols = verifier._instance_columns(cs, instance)
    plan = bvm.TermsPlan(lay, vk.domain.omega, [len(c) for c in inst_cols])
    ch, own, shared, _ = bvm.proof_terms_ints(vk, instance, proof, lay)
    evals, det = bvm.read_proof_ints(lay, proof)[1], {}
    bvm.terms_from_challenges(lay, vk.domain.omega, inst_cols, evals, ch, det)
    for rb in (1, R - 1, 0x1234567890ABCDEF1234567):
        record = [ch[name] for name in bvm.RECORD] + [rb]
        rc, why, vals, got_own, got_shared, h2r, h2l = terms_on_the_host(hc, plan, lay, record, evals, plan.instance_row(inst_cols), det["numerator"])
        assert (rc, why) == (1, None)
        assert vals[:lay.n_scalars] == evals
        assert vals[plan.s_l0:plan.s_l0 + 4] == [det["l0"], det["l_last"], det["l_active"], ch["x"]] and vals[plan.s_hx] == det["hx"]
        assert [vals[plan.s_inst + i] for i in range(len(plan.inst_queries))] == [det["instance"][q] for q in plan.inst_queries]
        assert got_own == [rb * c % R for c in own[:-1]] and got_shared == [rb * c % R for c in shared]
        assert (h2r, h2l) == (rb * own[-1] % R, rb)


def test_terms_phases_flag_a_zero_they_would_invert(hc, golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    inst_cols = verifier._instance_columns(cs, instance)
    plan = bvm.TermsPlan(lay, vk.domain.omega, [len(c) for c in inst_cols])
    ch = bvm.proof_terms_ints(vk, instance, proof, lay)[0]
    evals = bvm.read_proof_ints(lay, proof)[1]
    first_set_complement = next(r for r in lay.super_rotations if r not in lay.sets[0][0])
    for change in (dict(x=1), dict(x=vk.domain.omega), dict(x=0), dict(u=ch["x"] * pow(vk.domain.omega, first_set_complement, R) % R)):
        record = [dict(ch, **change)[name] for name in bvm.RECORD] + [7]
        rc, why = terms_on_the_host(hc, plan, lay, record, evals, plan.instance_row(inst_cols), 5)[:2]
        assert (rc, why) == (0, None), change                               # flagged, and no bound violated on the way


def test_plan_builder_and_plan_check_refusals(hc, golden_proof):
    cs, vk, instance, proof, lay = golden_proof
    with pytest.raises(ValueError, match="longer than 64 rows"):
        bvm.TermsPlan(lay, vk.domain.omega, [65] * cs.num_instance)
    with pytest.raises(ValueError, match="instance column"):
        bvm.TermsPlan(lay, vk.domain.omega, [1] * (cs.num_instance + 1))
    plan = bvm.TermsPlan(lay, vk.domain.omega, [64] * cs.num_instance)
    assert plan.words[15] == 64 * cs.num_instance and plan.n_vals <= 256
    inst_cols = verifier._instance_columns(cs, instance)
    ch = bvm.proof_terms_ints(vk, instance, proof, lay)[0]
    evals = bvm.read_proof_ints(lay, proof)[1]
    record = [ch[name] for name in bvm.RECORD] + [1]

    def refused(words, n_columns=plan.n_columns):
        broken = SimpleNamespace(words=np.array(words, dtype=np.uint32), n_vals=plan.n_vals, n_columns=n_columns)
        rc, why = terms_on_the_host(hc, broken, lay, record, evals, plan.instance_row(inst_cols), 5)[:2]
        assert rc == -1
        return why.decode()

    good = plan.words.tolist()
    poke = lambda at, value: good[:at] + [value] + good[at + 1:]
    off_inst, off_sets, off_colmap = good[13], good[14], good[12]
    assert "64 rows" in refused(poke(off_inst + 1, 65))
    assert "256 value slots" in refused(poke(2, 257))
    assert "another number of columns" in refused(good, plan.n_columns + 1)
    assert "shorter" in refused(good[:10])
    assert "slot outside" in refused(poke(off_colmap + good[off_colmap:off_colmap + 4000].index(0), plan.n_vals))
    assert "out of range" in refused(poke(off_sets + 3, 32)) and "1 .. 8 points" in refused(poke(off_sets, 9))
    assert "constants lie outside" in refused(poke(22, 1 << 15)) and "lie outside" in refused(good[:-1])
    # the C entry refuses the same plans, and null arguments, before it looks for a device
    lib = _lib.load()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    fake = ctypes.c_void_p(0x1000)
    call = lambda words, cols=plan.n_columns, proofs=1: lib.hm_verify_terms_dev(
        ctypes.c_uint64(1), np.array(words, dtype=np.uint32).ctypes.data_as(u32p), len(words), cols, 4, proofs, fake, fake, fake,
        ctypes.cast(fake, u32p), fake, fake, fake, fake, None)
    assert call(poke(off_inst + 1, 65)) == -1 and b"64 rows" in lib.hm_last_error()
    assert call(poke(2, 257)) == -1 and b"256 value slots" in lib.hm_last_error()
    assert call(good, proofs=0) == -1 and call(good, cols=0) == -1
    assert lib.hm_verify_terms_dev(ctypes.c_uint64(1), None, 0, 1, 4, 1, fake, fake, fake, ctypes.cast(fake, u32p), fake, fake, fake, fake, None) == -1
    assert lib.hm_verify_read_proofs_dev(None, 1, None, 1, 0, 1, 0, None, None, None, None, None, None) == -1
    assert lib.hm_verify_read_proofs_dev(fake, 1, ctypes.cast(fake, u32p), 5, 3, 2, 2, fake, fake, fake, fake, ctypes.cast(fake, u32p), None) == -1
    assert lib.hm_verify_column_sum_dev(fake, 4, 2, 3, 2, fake, None) == -1 and lib.hm_verify_column_sum_dev(fake, 4, 2, 0, 5, fake, None) == -1
    if lib.hm_device_count() == 0:
        assert call(good) == -2 and lib.hm_verify_column_sum_dev(fake, 4, 2, 0, 4, fake, None) == -2
