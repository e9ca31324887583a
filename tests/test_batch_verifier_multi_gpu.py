"""Multi-circuit proofs through the batch verifier on the GPU (``BatchVerifier(..., circuits=m)``, ``hm_verify_terms_multi_dev``: one
wavefront per proof, one lane per circuit).  The proofs are made here by ``create_proof_multi`` at the mutation
sweep's small shapes; ``proof_terms_ints`` on a multi-circuit ``ProofLayout`` is the oracle, word for word.  m = 2 is the first real
fold, 3 is odd (and the recorded proof's), 33 is one lane past half a wave, 64 leaves no idle lane; B = 5 puts several waves into a
workgroup and leaves the last workgroup ragged."""
import ctypes
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, batch_verifier as bvm, circuits, evaluation as ev, poseidon as ps, synthesis as sy
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, FR_MODULUS as R, fr_array, fr_ints
from halo2_experiments_amd.domain import EvaluationDomain
from halo2_experiments_amd.keygen import VerifyingKey
from halo2_experiments_amd.kzg import G2_GENERATOR, ParamsKZG, g2_bytes, g2_mul

import mutation_cases as mc
import prover_cases as pc
import prover_multi_cases as pmc
import verify_terms_cases as vt
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FILL = -0x5A5A5A5A5A5A5A5B                                                     # what an unwritten output word holds
BAD_CANARY = 0x5A5A5A5A
_u32p = ctypes.POINTER(ctypes.c_uint32)
MODES = [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device")]     # (pairing, transcript)


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


# ---- keys and proofs, made once ------------------------------------------------------------------------------------------------------------
class Stack:
    """one constraint system with its keys; ``proof(m, seed)`` is a ``create_proof_multi`` proof of m circuits, made once"""

    def __init__(self, name):
        self.name = name
        if name == "poseidon":
            self.cs, self.lay = mc.case("poseidon").cs, mc.case("poseidon").lay
        elif name == "safe_accumulator_4x4":
            self.cs, self.lay = circuits.safe_accumulator(4, 4), sy.SafeAccumulatorLayout(6, 4, 4, 3)
            self.lay.check_constraint_system(self.cs)
        else:
            self.cs, self.lay = mc.case(name).cs, mc.case(name).lay
        self.k = self.lay.k
        self.params = ParamsKZG.setup(self.k, pc.SRS_S)
        self.vk = h.keygen_vk(self.params, self.cs, self.lay)
        self.pk = h.keygen_pk(self.params, self.vk, self.cs, self.lay, cosets=False)
        self._proofs, self._terms, self._layouts = {}, {}, {}

    def layout(self, m):
        if m not in self._layouts:
            self._layouts[m] = bvm.ProofLayout(self.cs, self.k, circuits=m)
        return self._layouts[m]

    def witness(self, m, seed):
        """-> ((m, num_advice, n, 4) advice, [the instance of circuit c])"""
        if self.name == "poseidon":                                            # m different users, written on the device
            _, _, adv, instances = pmc.build_multi("poseidon_k6", m, seed)
            return adv, instances
        if self.name == "safe_accumulator_4x4":                                # degree 17: sixteen h pieces; a different first value per circuit
            advs, instances = [], []
            for c in range(m):
                initial, values = [0, 1, 2, 3], [(5 + c + seed) % 16, 9, 15]
                advs.append([v for col in self.lay.assign_ints(initial, values) for v in col])
                instances.append(list(self.lay.instance(initial, values)[0]))
            return d([v for a in advs for v in a]).reshape(m, self.cs.num_advice, self.lay.n, 4).contiguous(), instances
        c = mc.case(self.name)                                                 # the sweep's satisfied witness in every circuit: the blinding differs
        one = d([v for col in c.advice for v in col]).reshape(1, self.cs.num_advice, c.n, 4)
        return one.repeat(m, 1, 1, 1).contiguous(), [c.proof_instance] * m

    def proof(self, m, seed):
        if (m, seed) not in self._proofs:
            adv, instances = self.witness(m, seed)
            self._proofs[(m, seed)] = (instances, h.create_proof_multi(self.params, self.pk, adv, instances, seed))
        return self._proofs[(m, seed)]

    def terms(self, m, seed):
        """``proof_terms_ints`` of that proof: computed once, shared by the tests"""
        if (m, seed) not in self._terms:
            instances, proof = self.proof(m, seed)
            self._terms[(m, seed)] = bvm.proof_terms_ints(self.vk, instances, proof, self.layout(m))
        return self._terms[(m, seed)]


_STACKS = {}


@pytest.fixture(scope="module")
def stacks():
    def get(name):
        if name not in _STACKS:
            _STACKS[name] = Stack(name)
        return _STACKS[name]

    yield get
    for s in _STACKS.values():
        s.params.release()
    _STACKS.clear()


def batch(s, m, members, seed=5, **modes):
    bv = h.BatchVerifier(s.params, s.vk, seed=seed, circuits=m, **modes)
    for instances, proof in members:
        bv.add_proof(instances, proof)
    return bv


def assert_terms_equal_the_twin(s, m, bv, seeds):
    st = bv._prepare()
    lay = s.layout(m)
    own, n_shared = lay.own_points, len(lay.shared_keys)
    assert st["bad"] == [False] * len(seeds)
    ints = lambda t: fr_ints(t.cpu().numpy().view(np.uint64))
    got_own, got_shared, got_r, got_l = ints(st["d_own"]), ints(st["d_shared"]), ints(st["d_h2_r"]), ints(st["d_h2_l"])
    for b, seed in enumerate(seeds):
        _, o, sh, _ = s.terms(m, seed)
        rb = bv.randomizers[b]
        assert got_own[b * own:(b + 1) * own] == [rb * v % R for v in o[:own]], (b, "own")
        assert got_shared[b * n_shared:(b + 1) * n_shared] == [rb * v % R for v in sh], (b, "shared")
        assert (got_r[b], got_l[b]) == (rb * o[own] % R, rb), (b, "h2")


# ---- the kernel against proof_terms_ints, word for word ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("m", [2, 3, 33, 64])
def test_the_kernel_writes_the_twins_words(stacks, m, B):
    s = stacks("poseidon")
    seeds = [21, 22, 21, 22, 21][:B]
    bv = batch(s, m, [s.proof(m, seed) for seed in seeds])
    assert_terms_equal_the_twin(s, m, bv, seeds)
    assert bv.finalize(trapdoor=pc.SRS_S) and bv.verdicts(trapdoor=pc.SRS_S) == [True] * B
    bv.close()


@pytest.mark.parametrize("name,m", [("overflow_check_v2", 3), ("merkle_sum_tree", 2), ("safe_accumulator_4x4", 3)])
def test_other_constraint_systems(stacks, name, m):
    """lookups and an empty instance column; several permutation sets, lookups and an instance column; degree 17, sixteen h pieces"""
    s = stacks(name)
    seeds = [31, 32]
    bv = batch(s, m, [s.proof(m, seed) for seed in seeds], transcript="device", pairing="device")
    assert_terms_equal_the_twin(s, m, bv, seeds)
    assert bv.finalize(trapdoor=pc.SRS_S) and bv.finalize() and bv.verdicts() == [True, True]
    if name == "safe_accumulator_4x4":
        assert s.layout(m).pieces == 16
    for seed in seeds:
        instances, proof = s.proof(m, seed)
        assert h.verify_proof_multi(s.params, s.vk, instances, proof, trapdoor=pc.SRS_S)
    bv.close()


# ---- the two entries at one circuit -----------------------------------------------------------------------------------------------------------
def call_entry(program, plan, lay, m, records, evals, inst, bad_in):
    """``hm_verify_terms_dev`` (m = None) or ``hm_verify_terms_multi_dev`` on copies of the host arrays, a canary row behind every output"""
    n = len(bad_in)
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
    head = (ctypes.c_uint64(program.handle), plan.words.ctypes.data_as(_u32p), len(plan.words), plan.n_columns, 4, n)
    tail = (vp(d_in[0]), vp(d_in[1]), vp(d_in[2]), ctypes.cast(vp(d_bad), _u32p), vp(d_own), vp(d_shared), vp(d_h2r), vp(d_h2l), stream)
    lib = _lib.load()
    _lib.check(lib.hm_verify_terms_dev(*head, *tail) if m is None else lib.hm_verify_terms_multi_dev(*head, m, *tail))
    torch.cuda.current_stream(dev).synchronize()
    assert all(torch.equal(a, b) for a, b in zip(d_in, kept)), "the call wrote to its records, evaluations or instance values"
    host = lambda t: t.cpu().numpy().view(np.uint64)
    got = dict(bad=d_bad.cpu().numpy(), own=host(d_own).reshape(n + 1, lay.own_points, 4), shared=host(d_shared), h2r=host(d_h2r), h2l=host(d_h2l))
    for name in ("own", "shared", "h2r", "h2l"):
        assert (got[name][n].view(np.int64) == FILL).all(), f"{name}: the row behind the last proof was written"
    assert got["bad"][n] == BAD_CANARY
    return got


def random_records(lay, rows, count, seed, omega):
    """``count`` records of uniform integers for a layout of m circuits; the record before the last has x = omega (flagged)"""
    rng = random.Random(seed)
    draw = lambda: rng.randrange(R)
    out = []
    for b in range(count):
        ch = {name: draw() for name in bvm.RECORD}
        if count > 1 and b == count - 2:
            ch["x"] = omega
        insts = [[[draw() for _ in range(rows)] for _ in range(lay.cs.num_instance)] for _ in range(lay.circuits)]
        out.append((ch, draw(), [draw() for _ in range(lay.n_scalars)], insts))
    return out


def arrays_of(plan, lay, recs):
    records = np.stack([fr_array([ch[n] for n in bvm.RECORD] + [rb]) for ch, rb, _, _ in recs])
    evals = np.stack([fr_array(e) for _, _, e, _ in recs])
    inst = np.stack([fr_array(plan.instance_row(one)) for _, _, _, insts in recs for one in insts])
    return records, evals, inst


def test_the_two_entries_write_the_same_words_at_one_circuit():
    """Poseidon k = 6, B = 3, one of the three flagged by the kernels (x = omega)"""
    s = vt.setup("poseidon_k6_rows64")
    lay1 = bvm.ProofLayout(s.cs, s.k, circuits=1)
    multi = bvm.MultiTermsPlan(lay1, s.omega, [64] * s.cs.num_instance)
    assert np.array_equal(multi.lane.words, s.plan.words) and multi.lowered is multi.lane.lowered
    program = ev.CompiledGraph(**s.plan.lowered)
    try:
        recs = random_records(lay1, 64, 3, 77, s.omega)
        records, evals, inst = arrays_of(multi, lay1, recs)
        bad_in = np.zeros(3, dtype=np.int32)
        old = call_entry(program, s.plan, s.layout, None, records, evals, inst, bad_in)
        new = call_entry(program, multi, lay1, 1, records, evals, inst, bad_in)
        assert old["bad"].tolist()[:3] == [0, 1, 0]
        for name in ("bad", "own", "shared", "h2r", "h2l"):
            assert np.array_equal(old[name], new[name]), name
        assert old["own"][0].any() and not old["own"][1].any()
    finally:
        program.destroy()


@pytest.mark.parametrize("config,m", [("merkle_sum_k9_rows1", 3), ("poseidon_k6_rows64", 33), ("overflow_v2_k5_rows0", 64)])
def test_records_no_transcript_produces(config, m):
    """B = 6 proofs of uniform integers straight into the entry: proof 0 flagged by the caller (all-ones words, never read), proof 4
    flagged by every lane (x = omega); the others equal ``terms_from_challenges`` word for word"""
    s = vt.setup(config)
    lay = bvm.ProofLayout(s.cs, s.k, circuits=m)
    plan = bvm.MultiTermsPlan(lay, s.omega, [s.rows] * s.cs.num_instance)
    program = ev.CompiledGraph(**plan.lowered)
    try:
        recs = random_records(lay, s.rows, 6, 1000 + m, s.omega)
        records, evals, inst = arrays_of(plan, lay, recs)
        records[0], evals[0], inst[:m] = np.uint64(2 ** 64 - 1), np.uint64(2 ** 64 - 1), np.uint64(2 ** 64 - 1)
        bad_in = np.array([1, 0, 0, 0, 0, 0], dtype=np.int32)
        got = call_entry(program, plan, lay, m, records, evals, inst, bad_in)
        assert got["bad"].tolist()[:6] == [1, 0, 0, 0, 1, 0]
        for b, (ch, rb, ev_, insts) in enumerate(recs):
            if b in (0, 4):
                assert not got["own"][b].any() and not got["shared"][b].any() and not got["h2r"][b].any() and not got["h2l"][b].any()
                continue
            own, shared = bvm.terms_from_challenges(lay, s.omega, insts, ev_, ch)
            assert fr_ints(got["own"][b]) == [rb * c % R for c in own[:-1]], b
            assert fr_ints(got["shared"][b]) == [rb * c % R for c in shared], b
            assert (fr_ints(got["h2r"][b:b + 1])[0], fr_ints(got["h2l"][b:b + 1])[0]) == (rb * own[-1] % R, rb)
    finally:
        program.destroy()


# ---- the recorded three-circuit proof ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    cs, k = pc.constraint_system("poseidon_k6")
    meta = np.load(os.path.join(GOLDEN, "proof_poseidon_k6_x3.npz"))
    vk = VerifyingKey(EvaluationDomain(cs.degree(), k), cs, meta["fixed_commitments"], meta["permutation_commitments"])
    proof = open(os.path.join(GOLDEN, "proof_poseidon_k6_x3.bin"), "rb").read()
    params = SimpleNamespace(g2=g2_bytes(G2_GENERATOR), s_g2=g2_bytes(g2_mul(pc.SRS_S)))
    return SimpleNamespace(vk=vk, instances=[ps.words_to_ints(i) for i in meta["instances"]], proof=proof, params=params)


@pytest.mark.parametrize("pairing,transcript", MODES)
def test_the_recorded_proof_through_the_device(golden, pairing, transcript):
    g = golden
    assert h.verify_proofs(g.params, g.vk, [g.instances], [g.proof], seed=2, pairing=pairing, transcript=transcript, circuits=3)
    assert h.verify_each(g.params, g.vk, [g.instances] * 2, [g.proof] * 2, seed=2, pairing=pairing, transcript=transcript, circuits=3) == [True, True]
    swapped = [g.instances[1], g.instances[0], g.instances[2]]
    assert not h.verify_proofs(g.params, g.vk, [swapped], [g.proof], seed=2, pairing=pairing, transcript=transcript, circuits=3)


# ---- verdicts: every lane's contribution reaches the sum ----------------------------------------------------------------------------------
def put(proof, at, data):
    return proof[:at] + data + proof[at + 32:]


@pytest.mark.parametrize("what", ["evaluation of circuit 0", "evaluation of circuit 1", "evaluation of circuit 2", "instance of the last circuit"])
def test_a_tampered_circuit_is_named(stacks, what):
    s, m, B, victim = stacks("poseidon"), 3, 4, 2
    lay = s.layout(m)
    members = [s.proof(m, seed) for seed in (21, 22, 21, 22)]
    instances, proof = members[victim]
    if what.startswith("evaluation"):
        c = int(what[-1])
        slot = lay.scalar_slots[next(at for at, (key, _) in enumerate(lay.eval_keys) if key[0] == "advice" and key[2] == c) + 1]
        value = (int.from_bytes(proof[32 * slot:32 * slot + 32], "little") + 1) % R
        members[victim] = (instances, put(proof, 32 * slot, value.to_bytes(32, "little")))
    else:
        changed = [list(i) for i in instances]
        changed[m - 1][0] = (changed[m - 1][0] + 1) % R
        members[victim] = (changed, proof)
    assert not h.verify_proof_multi(s.params, s.vk, *members[victim], trapdoor=pc.SRS_S)
    bv = batch(s, m, members, pairing="device", transcript="device")
    want = [b != victim for b in range(B)]
    assert bv._prepare()["bad"] == [False] * B                                 # well-formed: only the sums can tell
    assert bv.finalize(trapdoor=pc.SRS_S) is False and bv.finalize() is False
    assert bv.failing(trapdoor=pc.SRS_S) == [victim] and bv.failing(method="each") == [victim]
    assert bv.verdicts() == want and bv.verdicts(trapdoor=pc.SRS_S) == want
    bv.close()


# ---- malformed proofs -------------------------------------------------------------------------------------------------------------------------
def test_malformed_proofs_are_flagged_and_kept_out_of_the_sums(stacks):
    s, m = stacks("poseidon"), 3
    lay = s.layout(m)
    instances, good = s.proof(m, 21)
    non_residue = next(x for x in range(1, 50) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) != 1)
    last_eval = lay.scalar_slots[lay.eval_index[(("perm_z", lay.nsets - 1, m - 1), 1)]]
    assert last_eval == max(lay.scalar_slots[lay.eval_index[key]] for key in lay.eval_index if key[0][-1] == m - 1 and len(key[0]) == 3)
    advice_of_circuit_1 = lay.point_slots[lay.own_index[("advice", 0, 1)]]
    bad = {1: good[:-32], 3: put(good, 32 * last_eval, R.to_bytes(32, "little")),
           4: put(good, 32 * advice_of_circuit_1, non_residue.to_bytes(32, "little"))}
    for transcript in ("host", "device"):
        bv = batch(s, m, [(instances, bad.get(b, good)) for b in range(6)], transcript=transcript, pairing="device")
        st = bv._prepare()
        assert st["bad"] == [b in bad for b in range(6)] and bv.malformed() == sorted(bad)
        own = lay.own_points
        rows = st["d_own"].cpu().numpy().reshape(6, own, 4)
        assert all(rows[b].any() != (b in bad) for b in range(6)) and not st["d_h2_l"].cpu().numpy()[sorted(bad)].any()
        assert not bv.finalize(trapdoor=pc.SRS_S) and bv.failing(trapdoor=pc.SRS_S) == sorted(bad)
        assert bv.verdicts() == [b not in bad for b in range(6)]
        bv.close()
    rest = batch(s, m, [(instances, good)] * 3, pairing="device")
    assert rest.finalize() and rest.finalize(trapdoor=pc.SRS_S)
    rest.close()


# ---- the device transcript ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 64])
def test_the_device_transcript_gives_the_twins_challenges(stacks, m):
    s = stacks("poseidon")
    seeds = [21, 22]
    bv = batch(s, m, [s.proof(m, seed) for seed in seeds], transcript="device")
    st = bv._prepare()
    records = st["d_records"].cpu().numpy().view(np.uint64)
    assert st["bad"] == [False, False]
    assert st["preamble"][1].cpu().tolist() == [1 + sum(len(col) for one in inst for col in one) for inst in bv._instances]
    for b, seed in enumerate(seeds):
        ch = s.terms(m, seed)[0]
        assert fr_ints(records[b]) == [ch[name] for name in bvm.RECORD] + [bv.randomizers[b]]
    bv.close()


def test_a_plan_is_cached_per_row_counts_and_circuits(stacks):
    s, m = stacks("poseidon"), 2
    bv = batch(s, m, [s.proof(m, 21)])
    bv._prepare()
    rows = tuple(len(col) for col in bv._instances[0][0])
    assert list(bv._plans) == [(rows, m)] and isinstance(bv._plans[(rows, m)], bvm.MultiTermsPlan)
    one = h.BatchVerifier(s.params, s.vk, seed=1)
    assert one.circuits == 1 and one._plan_for(rows) is one._plans[rows] and isinstance(one._plans[rows], bvm.TermsPlan)
    one.close()
    bv.close()
