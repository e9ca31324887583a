"""The SafeAccumulator circuit on the GPU: synthesis.accumulator_witness word for word against SafeAccumulatorLayout.assign_ints -- row
counts around the wave, the block and the block-totals scan, carry chains that cross a wave and a block boundary, three circuits with
different states in one call, the five (max_bits, acc_cols) shapes with the 64-bit wrap -- ``out=`` reuse, the host-pointer form, the
refusals, and the circuit through the device MockProver, keygen, create_proof / create_proofs and verify_proof.  Keys, parameters and
proofs are made once per shape and shared, never changed."""
import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.kzg import ParamsKZG

import safe_accumulator_cases as sc

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
SA = sy.SafeAccumulatorLayout
B = sy.ACCUMULATOR_BLOCK_ROWS
# 1; around a wave; around a block; two blocks and a row
ROWS = [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]
SCAN_ROWS = 64 * B + 5                    # 65 block totals: more than one wave of the scan kernel's lanes hold one
CHUNK_ROWS = 256 * B + 3                  # 257 block totals: the scan kernel's lanes take two each


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def words(columns):
    return sy.columns_to_words(columns)


def boundary(rows):
    """the row whose value starts a carry chain: the first row of the second block where there is one (its S_(r-1) comes from the
    last lane of block 0), else the first lane of the second wave, else the last row"""
    return B if rows >= B else 64 if rows >= 64 else rows


def three_circuits(b, A, rows, seed):
    """a legal ripple across the block or wave boundary; a chain into the top limb from the last lane of wave 0 -- or the wrap of the
    64-bit total; seeded values from a seeded state"""
    second = sc.pattern("wrap" if b * A == 64 else "overflow", b, A, rows, min(rows, 64), seed)
    return [sc.pattern("ripple", b, A, rows, boundary(rows), seed), second, sc.pattern("random", b, A, rows, None, seed)]


def run(b, A, k, cases, out=None):
    m, rows = len(cases), len(cases[0][1])
    dv = d([v for _, vs in cases for v in vs]).reshape(m, rows, 4)
    di = torch.tensor([[int(x) for x in ini] for ini, _ in cases], dtype=torch.int64, device="cuda")
    adv, finals, over = sy.accumulator_witness(dv, di, k, b, A, out=out)
    return dv, di, adv, finals, over


# ---- the witness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("b, A", sc.SHAPES)
def test_witness_equals_assign_ints(b, A, rows):
    k = SA.min_k(rows)
    lay, cases = SA(k, b, A, rows), three_circuits(b, A, rows, seed=rows)
    out = torch.full((3, 2 + 2 * A, 1 << k, 4), -1, dtype=torch.int64, device="cuda")          # a dirty buffer: every word must be written
    dv, di, adv, finals, over = run(b, A, k, cases, out=out)
    assert adv.data_ptr() == out.data_ptr() and tuple(finals.shape) == (3, A) and tuple(over.shape) == (3,)
    got = adv.cpu().numpy().view(np.uint64)
    expected = [words(lay.assign_ints(ini, vs)) for ini, vs in cases]
    for c, (ini, vs) in enumerate(cases):
        assert np.array_equal(got[c], expected[c]), c
    assert not got[:, :, rows + 1:].any()
    assert finals.cpu().tolist() == [lay.finals(ini, vs) for ini, vs in cases]
    assert over.cpu().tolist() == [lay.over(ini, vs) for ini, vs in cases]
    assert over.cpu().tolist()[0] == 0 or b * (A - 2) == 0   # the ripple stays legal (with two limbs there is nothing to ripple through)
    assert over.cpu().tolist()[1] >= 1                        # the chain into the top limb, or the wrap, is counted
    # one circuit alone: the second one's state and pattern, so that a wrong circuit offset shows in either call
    _, _, one, finals1, over1 = run(b, A, k, cases[1:2])
    assert np.array_equal(one.cpu().numpy().view(np.uint64)[0], expected[1])
    assert finals1.cpu().tolist() == finals.cpu().tolist()[1:2] and over1.cpu().tolist() == over.cpu().tolist()[1:2]
    # the host-pointer form
    if rows <= B + 1:
        host_adv, host_finals, host_over = sy.accumulator_witness_host(dv.cpu().numpy().view(np.uint64), di.cpu().numpy().view(np.uint64), k, b, A)
        assert np.array_equal(host_adv, got) and host_finals.tolist() == finals.cpu().tolist() and host_over.tolist() == over.cpu().tolist()


def test_the_block_totals_scan_over_more_than_a_wave_against_assign_ints():
    """(2, 3), one circuit, 65 blocks: the integer twin itself"""
    b, A, rows = 2, 3, SCAN_ROWS
    k = SA.min_k(rows)
    lay = SA(k, b, A, rows)
    ini, vs = sc.pattern("ripple", b, A, rows, 63 * B, seed=1)
    _, _, adv, finals, over = run(b, A, k, [(ini, vs)])
    assert np.array_equal(adv.cpu().numpy().view(np.uint64)[0], words(lay.assign_ints(ini, vs)))
    assert finals.cpu().tolist() == [lay.finals(ini, vs)] and over.cpu().tolist() == [lay.over(ini, vs)]


@pytest.mark.parametrize("b, A, rows, m", [(4, 16, SCAN_ROWS, 3), (4, 4, CHUNK_ROWS, 1)])
def test_the_block_totals_scan_at_full_width(b, A, rows, m):
    """65 totals per circuit at the full 64 bits (the third circuit wraps), and 257 totals, two per lane of the scan kernel: against
    the numpy twin of assign_ints (safe_accumulator_cases.numpy_columns), values below 2^b placed by a seeded generator"""
    k = SA.min_k(rows)
    rng = np.random.default_rng(rows)
    top = (1 << b) - 1
    cases = []
    for c in range(m):
        vals = rng.integers(0, top + 1, size=rows, dtype=np.uint64)
        if c % 2 == 0:
            vals[rng.random(rows) < 0.9] = 0                 # a sparse circuit: the top limb stays zero for long
        ini = [0] + [int(x) for x in rng.integers(0, top + 1, size=A - 1)]
        if c == 2:
            ini = [top] * A                                  # 2^64 - 1: the first non-zero value wraps the total
        cases.append((ini, vals))
    dv = torch.from_numpy(ps.ints_to_words(list(range(top + 1))).view(np.int64)).cuda()[
        torch.from_numpy(np.stack([vs for _, vs in cases]).astype(np.int64)).cuda()].contiguous()
    di = torch.tensor([ini for ini, _ in cases], dtype=torch.int64, device="cuda")
    adv, finals, over = sy.accumulator_witness(dv, di, k, b, A)
    got = adv.cpu().numpy().view(np.uint64)
    for c, (ini, vs) in enumerate(cases):
        cols, fin, ov = sc.numpy_columns(b, A, ini, vs, 1 << k)
        assert np.array_equal(got[c], cols), c
        assert finals[c].cpu().tolist() == fin and int(over[c]) == ov, c


def test_values_and_limbs_that_are_not_judged():
    """values at or above 2^b (2^16 + x, r - 1, 2^64 + 1) and an initial limb of 2^40 + 3: the cells are what assign_ints says"""
    b, A, rows, k = 4, 4, 70, 7
    lay = SA(k, b, A, rows)
    vs = [R - 1, 1 << b, (1 << 64) + 1, (1 << 16) + 0x123] + [v % 16 for v in range(rows - 4)]
    cases = [([0, (1 << 40) + 3, 1, 1], vs), ([1, 2, 3, 4], vs[::-1]), ([0, 0, 16, 0], [1] * rows)]
    _, _, adv, finals, over = run(b, A, k, cases)
    got = adv.cpu().numpy().view(np.uint64)
    for c, (ini, v) in enumerate(cases):
        assert np.array_equal(got[c], words(lay.assign_ints(ini, v))), c
    assert finals.cpu().tolist() == [lay.finals(ini, v) for ini, v in cases]
    assert over.cpu().tolist() == [lay.over(ini, v) for ini, v in cases] and min(over.cpu().tolist()) >= 1


def test_refusals_launch_nothing():
    b, A, k, rows = 4, 4, 5, 3
    dv, di = d([1, 2, 3]).reshape(1, rows, 4), torch.zeros((1, A), dtype=torch.int64, device="cuda")
    out = torch.full((1, 2 + 2 * A, 1 << k, 4), -1, dtype=torch.int64, device="cuda")
    bad = [
        lambda: sy.accumulator_witness(dv.reshape(rows, 4), di, k, b, A, out=out),                     # values not (m, rows, 4)
        lambda: sy.accumulator_witness(dv, di.reshape(A), k, b, A, out=out),                           # initial not (m, A)
        lambda: sy.accumulator_witness(dv, torch.zeros((1, A + 1), dtype=torch.int64, device="cuda"), k, b, A, out=out),
        lambda: sy.accumulator_witness(dv, torch.zeros((2, A), dtype=torch.int64, device="cuda"), k, b, A, out=out),
        lambda: sy.accumulator_witness(dv.cpu(), di, k, b, A, out=out),
        lambda: sy.accumulator_witness(dv, di, k, b, A, out=out[:, :, :16]),                           # out of another shape
        lambda: sy.accumulator_witness(d(list(range(26))).reshape(1, 26, 4), di, k, b, A, out=out),    # rows + 1 > 2^k - 6
        lambda: sy.accumulator_witness(dv, torch.zeros((1, 17), dtype=torch.int64, device="cuda"), k, 4, 17),     # 68 bits
        lambda: sy.accumulator_witness(dv, torch.zeros((1, 1), dtype=torch.int64, device="cuda"), k, 4, 1),
        lambda: sy.accumulator_witness(dv, di, k, 5, A),
        lambda: sy.accumulator_witness_host(np.zeros((1, 26, 4), dtype=np.uint64), np.zeros((1, A), dtype=np.uint64), k, b, A),
        lambda: sy.accumulator_witness_host(np.zeros((1, 3, 4), dtype=np.uint64), np.zeros((1, 17), dtype=np.uint64), k, 4, 17),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    adv, finals, over = sy.accumulator_witness(dv, di, k, b, A, out=out)
    torch.cuda.synchronize()
    assert not bool((out == -1).any()) and finals.cpu().tolist() == [[0, 0, 0, 6]] and over.cpu().tolist() == [0]


# ---- through the stack ----------------------------------------------------------------------------------------------------------------
STACK = {"2x3": (2, 3, 5, 3), "4x4": (4, 4, 6, 40)}         # max_bits, acc_cols, k, rows


def good_batch(b, A, rows):
    """three users whose totals stay below 2^(b (A - 1)): a legal ripple on the last row, seeded small values, zeros"""
    top = (1 << b) - 1
    quiet = ([0] + [top] * (A - 1), [0] * rows)
    if b * (A - 1) >= 12:
        return [sc.pattern("ripple", b, A, rows, rows, seed=8), ([0, 0, 1, 2], [(7 * r) % 16 for r in range(rows)]), quiet]
    return [sc.pattern("ripple", b, A, rows, rows, seed=8), ([0, 0, 1], [1, 0, 3][:rows]), quiet]


@pytest.fixture(scope="module", params=list(STACK))
def stack(request):
    b, A, k, rows = STACK[request.param]
    cs, lay = circuits.safe_accumulator(b, A), SA(k, b, A, rows)
    cases = good_batch(b, A, rows)
    assert all(sc.satisfied(b, A, ini, vs) for ini, vs in cases)
    _, _, adv, finals, over = run(b, A, k, cases)
    params = ParamsKZG.setup(k, SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    instances = finals.cpu().tolist()
    proofs = [h.create_proof(params, pk, adv[c], instances[c], 40 + c) for c in range(3)]
    yield dict(b=b, A=A, k=k, rows=rows, cs=cs, lay=lay, cases=cases, adv=adv, finals=finals, over=over, params=params, vk=vk, pk=pk,
               instances=instances, proofs=proofs)
    params.release()


def instance_tensor(instances):
    return d([x for inst in instances for x in inst]).reshape(len(instances), -1, 4)


def test_device_mock_prover_is_satisfied_on_a_good_batch(stack):
    s = stack
    assert s["over"].cpu().tolist() == [0, 0, 0]
    assert s["instances"] == [s["lay"].finals(ini, vs) for ini, vs in s["cases"]]
    mp = h.MockProver(s["cs"], s["lay"])
    mp.assert_satisfied(s["adv"], instance_tensor(s["instances"]))
    res = mp.verify(s["adv"], instance_tensor(s["instances"]))
    assert res.ok and res.failures == [] and res.total == {"gate": 0, "copy": 0, "lookup": 0}


def test_device_mock_prover_names_the_overflowing_user(stack):
    s = stack
    b, A, k, rows = s["b"], s["A"], s["k"], s["rows"]
    at = rows - 1
    cases = list(s["cases"])
    cases[1] = sc.pattern("overflow", b, A, rows, at, seed=9)                 # user 1 reaches the top limb on row rows - 1 and stays there
    _, _, adv, finals, over = run(b, A, k, cases)
    assert over.cpu().tolist() == [0, 2, 0]
    res = h.MockProver(s["cs"], s["lay"]).verify(adv, instance_tensor(finals.cpu().tolist()))
    assert not res.ok and res.users_failed == [1]
    poly = sc.poly_index(A, "overflow")
    assert res.failures == [("gate", 1, sc.GATE, poly, at), ("gate", 1, sc.GATE, poly, rows)] and res.total == {"gate": 2, "copy": 0, "lookup": 0}
    with pytest.raises(h.NotSatisfied):
        h.MockProver(s["cs"], s["lay"]).assert_satisfied(adv, instance_tensor(finals.cpu().tolist()))


def test_proofs_verify(stack):
    s = stack
    assert len(s["proofs"][0]) == h.verifier.proof_length(s["cs"])
    for c in range(3):
        assert h.verify_proof(s["params"], s["vk"], s["instances"][c], s["proofs"][c]), c
    assert h.verify_proof(s["params"], s["vk"], s["instances"][0], s["proofs"][0], trapdoor=SRS_S)


def test_create_proofs_equals_three_create_proof_calls(stack):
    s = stack
    assert h.create_proofs(s["params"], s["pk"], s["adv"], s["instances"], [40, 41, 42]) == s["proofs"]


def test_a_wrong_instance_limb_is_rejected(stack):
    s = stack
    for limb in range(s["A"]):
        wrong = list(s["instances"][0])
        wrong[limb] = (wrong[limb] + 1) % (1 << s["b"])
        assert not h.verify_proof(s["params"], s["vk"], wrong, s["proofs"][0]), limb
    assert not h.verify_proof(s["params"], s["vk"], s["instances"][1], s["proofs"][0]) or s["instances"][1] == s["instances"][0]


def test_an_overflowing_total_is_not_provable(stack):
    s = stack
    b, A, k, rows = s["b"], s["A"], s["k"], s["rows"]
    _, _, adv, finals, over = run(b, A, k, [sc.pattern("overflow", b, A, rows, rows, seed=9)])
    assert over.cpu().tolist() == [1]
    proof = h.create_proof(s["params"], s["pk"], adv[0], finals.cpu().tolist()[0], 77)
    assert not h.verify_proof(s["params"], s["vk"], finals.cpu().tolist()[0], proof, trapdoor=SRS_S)


def test_the_timed_form_writes_the_same_witness():
    """``parts=``: the four launches' device times, and word for word the untimed call's output"""
    b, A, rows = 4, 4, B + 1
    k = SA.min_k(rows)
    cases = three_circuits(b, A, rows, seed=4)
    dv, di, adv, finals, over = run(b, A, k, cases)
    parts = []
    adv2, finals2, over2 = sy.accumulator_witness(dv, di, k, b, A, parts=parts)
    assert len(parts) == 4 and all(0 <= ms < 1000 for ms in parts) and parts[2] > 0
    assert torch.equal(adv, adv2) and torch.equal(finals, finals2) and torch.equal(over, over2)
