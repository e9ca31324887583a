"""``verify_terms_kernel`` (csrc/verify.hip over verify_terms.inc) on the GPU against its integer twin, on records no transcript produces
(tests/verify_terms_cases.py): the program is made with ``evaluation.CompiledGraph(**plan.lowered)`` and ``hm_verify_terms_dev`` is
called directly, as ``BatchVerifier._prepare`` calls it -- no SRS, key or proof.

Every parametrised case is ONE call of B = 513 lanes: three workgroups of 256 (T = 768), the last holding one lane.  Classes A - D are
shuffled over the lanes, so flagged and unflagged lanes share waves; lanes 63 / 64 / 65 and 255 / 256 / 257 hold an unflagged, a
flagged and an unflagged record; eight lanes, 0 and 512 among them, are flagged by the caller before the call and hold all-ones words.
Asserted: the lanes with d_bad = 1 are exactly the caller's and the twin's; each of them holds all-zero rows; every other lane equals
the twin word for word; one canary row behind each output and the inputs are untouched.

Further: small calls after a large one (the workspace keeps data laid out for another T), a call on a stream of its own, and the rule
that a flag of the terms kernel rejects the proof in ``BatchVerifier`` and names it."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, evaluation as ev
from halo2_experiments_amd.bn256 import FR_MODULUS as R, fr_array
from halo2_experiments_amd.kzg import ParamsKZG

import prover_cases as pc
import verify_terms_cases as vt

pytestmark = pytest.mark.gpu
SEED, B = 20242, 513
PRE_FLAGGED = (0, 31, 32, 127, 128, 300, 511, 512)
FIXED = {63: False, 64: True, 65: False, 255: False, 256: True, 257: False}     # lane -> flagged by the kernel
FILL = -0x5A5A5A5A5A5A5A5B                                                     # 0xA5A5...A5 as int64: what an unwritten output word holds
BAD_CANARY = 0x5A5A5A5A
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_cache = {}


def prepared(config):
    """the 513 lanes of ``config`` as host arrays, with what the twin expects of each; computed once"""
    if config in _cache:
        return _cache[config]
    s = vt.setup(config)
    lay, plan = s.layout, s.plan
    judged = list(vt.judged(config, SEED, B - len(PRE_FLAGGED)))               # asserts: A, B, D never flagged, C always
    rng = random.Random(SEED)
    rng.shuffle(judged)
    lanes = [None] * B
    for lane, want_flag in FIXED.items():
        at = next(i for i, (_, scalars, _) in enumerate(judged) if (scalars is None) == want_flag)
        lanes[lane] = judged.pop(at)
    free = [b for b in range(B) if b not in PRE_FLAGGED and b not in FIXED]
    assert len(free) == len(judged)
    for lane, entry in zip(free, judged):
        lanes[lane] = entry
    n_own, n_shared = lay.own_points, len(lay.shared_keys)
    records = np.full((B, len(bvm.RECORD) + 1, 4), ONES, dtype=np.uint64)
    evals = np.full((B, lay.n_scalars, 4), ONES, dtype=np.uint64)
    inst = np.full((B, plan.inst_elems, 4), ONES, dtype=np.uint64)
    own, shared = np.zeros((B, n_own, 4), dtype=np.uint64), np.zeros((B, n_shared, 4), dtype=np.uint64)
    h2r, h2l, bad_in, bad_out = np.zeros((B, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    labels = []
    for b, entry in enumerate(lanes):
        if entry is None:
            bad_in[b] = bad_out[b] = 1
            labels.append("pre-flagged")
            continue
        (label, ch, rb, ev_, inst_cols), scalars, _ = entry
        labels.append(label)
        records[b] = fr_array([ch[name] for name in bvm.RECORD] + [rb])
        evals[b] = fr_array(ev_)
        inst[b] = fr_array(plan.instance_row(inst_cols))
        if scalars is None:
            bad_out[b] = 1
        else:
            own[b], shared[b], h2r[b], h2l[b] = fr_array(scalars[0]), fr_array(scalars[1]), fr_array([scalars[2]])[0], fr_array([scalars[3]])[0]
    out = dict(setup=s, labels=labels, records=records, evals=evals, inst=inst, bad_in=bad_in, bad_out=bad_out, own=own, shared=shared,
               h2r=h2r, h2l=h2l)
    _cache[config] = out
    return out


@pytest.fixture(scope="module")
def programs():
    made = {}

    def program(config):
        if config not in made:
            made[config] = ev.CompiledGraph(**vt.setup(config).plan.lowered)
        return made[config]

    yield program
    for g in made.values():
        g.destroy()


def run_terms(program, s, records, evals, inst, bad_in):
    """one call on the current stream, on copies of the host arrays; the outputs hold one canary row behind the last lane.
    -> (inputs on the device, their clones made before the call, outputs as host arrays)"""
    lay, plan, n = s.layout, s.plan, len(bad_in)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    d_in = [up(records), up(evals), up(inst)]
    kept = [t.clone() for t in d_in]
    d_bad = torch.from_numpy(np.concatenate([bad_in, np.array([BAD_CANARY], dtype=np.int32)])).to(dev)
    d_own = torch.full(((n + 1) * lay.own_points, 4), FILL, dtype=torch.int64, device=dev)
    d_shared = torch.full((n + 1, len(lay.shared_keys), 4), FILL, dtype=torch.int64, device=dev)
    d_h2r, d_h2l = torch.full((n + 1, 4), FILL, dtype=torch.int64, device=dev), torch.full((n + 1, 4), FILL, dtype=torch.int64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().hm_verify_terms_dev(ctypes.c_uint64(program.handle), plan.words.ctypes.data_as(_u32p), len(plan.words), plan.n_columns,
                                               4, n, vp(d_in[0]), vp(d_in[1]), vp(d_in[2]), ctypes.cast(vp(d_bad), _u32p), vp(d_own),
                                               vp(d_shared), vp(d_h2r), vp(d_h2l), stream))
    torch.cuda.current_stream(dev).synchronize()
    host = lambda t: t.cpu().numpy().view(np.uint64)
    got = dict(bad=d_bad.cpu().numpy(), own=host(d_own).reshape(n + 1, lay.own_points, 4), shared=host(d_shared), h2r=host(d_h2r), h2l=host(d_h2l))
    return d_in, kept, got


def check_call(p, got, lo=0, hi=B):
    """the outputs of a call on lanes [lo, hi) of ``p``, against the twin"""
    n, labels = hi - lo, p["labels"][lo:hi]
    named = lambda lanes: [(lo + int(b), labels[int(b)]) for b in lanes[:8]]
    # the flags: exactly the caller's and the twin's
    wrong = np.nonzero(got["bad"][:n] != p["bad_out"][lo:hi])[0]
    assert wrong.size == 0, f"d_bad differs from the twin's flags at {named(wrong)}"
    assert set(np.unique(got["bad"][:n]).tolist()) <= {0, 1}
    flagged = p["bad_out"][lo:hi] == 1
    for name in ("own", "shared", "h2r", "h2l"):
        rows, want = got[name][:n].reshape(n, -1), p[name][lo:hi].reshape(n, -1)
        dirty = np.nonzero(rows[flagged].any(axis=1))[0]
        assert dirty.size == 0, f"{name}: a flagged lane holds a non-zero row at {named(np.nonzero(flagged)[0][dirty])}"
        wrong = np.nonzero((rows != want).any(axis=1))[0]
        assert wrong.size == 0, f"{name} differs from the twin at {named(wrong)}"
        assert (got[name][n].view(np.int64) == FILL).all(), f"{name}: the row behind the last lane was written"
    assert got["bad"][n] == BAD_CANARY, "d_bad: the word behind the last lane was written"


def unchanged(d_in, kept):
    return all(torch.equal(a, b) for a, b in zip(d_in, kept))


def test_the_lanes_are_laid_out_as_promised():
    p = prepared("poseidon_k6_rows0")
    kernel_flags = (p["bad_out"] == 1) & (p["bad_in"] == 0)
    assert [b for b in range(B) if p["bad_in"][b]] == list(PRE_FLAGGED) and {0, 512} <= set(PRE_FLAGGED)
    for lane, want_flag in FIXED.items():
        assert bool(kernel_flags[lane]) == want_flag and not p["bad_in"][lane]
    assert (p["records"][list(PRE_FLAGGED)] == ONES).all() and (p["evals"][list(PRE_FLAGGED)] == ONES).all()
    waves = {b // 64 for b in np.nonzero(kernel_flags)[0]}
    assert len(waves) >= 6                                                      # flagged lanes in most of the nine waves, each beside unflagged ones
    assert {label[0] for label in p["labels"] if label != "pre-flagged"} == set("ABCD")


@pytest.mark.parametrize("config", list(vt.CONFIGS))
def test_one_call_of_513_lanes_equals_the_twin(programs, config):
    p = prepared(config)
    s = p["setup"]
    kernel_flags = int(((p["bad_out"] == 1) & (p["bad_in"] == 0)).sum())
    assert kernel_flags >= 8 and int((p["bad_out"] == 0).sum()) >= 300          # lanes the kernel flags; lanes compared exactly
    d_in, kept, got = run_terms(programs(config), s, p["records"], p["evals"], p["inst"], p["bad_in"])
    check_call(p, got)
    assert unchanged(d_in, kept), "the call wrote to its records, evaluations or instance values"
    zero_unflagged = p["labels"].index("D:rb=0")                                # zero rows and NO flag: not the same thing as flagged
    assert got["bad"][zero_unflagged] == 0 and not got["own"][zero_unflagged].any() and not got["shared"][zero_unflagged].any()


@pytest.mark.parametrize("config", ["poseidon_k6_rows64", "merkle_sum_k9_rows1"])
def test_small_calls_after_a_large_one_give_its_rows(programs, config):
    """the aux slot's scratch is reused: after T = 768 it holds data laid out for another T when T = 256 runs"""
    p = prepared(config)
    s = p["setup"]
    _, _, big = run_terms(programs(config), s, p["records"], p["evals"], p["inst"], p["bad_in"])
    check_call(p, big)
    # B = 1, B = 1 on a lane the kernel flags, B = 65 with two lanes flagged on entry, B = 65 around lanes 255 / 256 / 257
    for lo, hi in [(200, 201), (256, 257), (120, 185), (229, 294)]:
        cut = lambda a: a[lo:hi].copy()
        d_in, kept, got = run_terms(programs(config), s, cut(p["records"]), cut(p["evals"]), cut(p["inst"]), cut(p["bad_in"]))
        check_call(p, got, lo, hi)
        for name in ("own", "shared", "h2r", "h2l"):
            assert np.array_equal(got[name][:hi - lo].reshape(hi - lo, -1), big[name][lo:hi].reshape(hi - lo, -1))
        assert np.array_equal(got["bad"][:hi - lo], big["bad"][lo:hi]) and unchanged(d_in, kept)


def test_on_a_stream_of_its_own(programs):
    config = "merkle_v3_k8_rows5"
    p = prepared(config)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in, kept, got = run_terms(programs(config), p["setup"], p["records"], p["evals"], p["inst"], p["bad_in"])
    side.synchronize()
    check_call(p, got)
    assert unchanged(d_in, kept)


# ---- a flag of the terms kernel rejects the proof, and names it -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poseidon_proofs():
    cs, lay, advice, instance, _ = pc.build("poseidon_k6")
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    proofs = [(instance, h.create_proof(params, pk, advice, instance, seed)) for seed in (11, 12, 13, 14, 15)]
    assert len({proof for _, proof in proofs}) == 5
    yield dict(params=params, vk=vk, proofs=proofs)
    params.release()


@pytest.mark.parametrize("what", ["x = omega", "u on a point outside the first set"])
def test_a_flag_of_the_terms_kernel_rejects_the_proof_and_names_it(poseidon_proofs, monkeypatch, what):
    c = poseidon_proofs
    victim, omega = c["proofs"][2][1], c["vk"].domain.omega
    real = bvm.transcript_challenges

    def forged(layout, vk_digest, inst_cols, proof, y_bytes):
        ch = real(layout, vk_digest, inst_cols, proof, y_bytes)
        if proof == victim:
            if what == "x = omega":
                ch["x"] = omega
            else:
                rot = next(r for r in layout.super_rotations if r not in layout.sets[0][0])
                ch["u"] = ch["x"] * pow(omega, rot, R) % R
        return ch

    monkeypatch.setattr(bvm, "transcript_challenges", forged)

    def batch(members):
        bv = h.BatchVerifier(c["params"], c["vk"], seed=5, transcript="host")
        for inst, proof in members:
            bv.add_proof(inst, proof)
        return bv

    bv = batch(c["proofs"])
    assert bv._prepare()["bad"] == [False, False, True, False, False]
    assert bv.finalize(trapdoor=pc.SRS_S) is False and bv.finalize() is False
    assert bv.failing(trapdoor=pc.SRS_S) == [2]
    bv.close()
    others = batch(c["proofs"][:2] + c["proofs"][3:])
    assert others.finalize(trapdoor=pc.SRS_S) and others.finalize() and others.failing(trapdoor=pc.SRS_S) == []
    others.close()
