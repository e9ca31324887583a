"""The MerkleSumTree witness on the CPU: synthesis.MerkleSumTreeLayout / assign_ints / permutation_cells against the tests' own
MockProver (tests/mock_prover.py), the reference's positive and six negative cases, the layout's properties for every depth, and
that circuits.py without a spec is what it was."""
import hashlib
import json
import os

import pytest

from halo2_experiments_amd import circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R

import mock_prover

HERE = os.path.dirname(os.path.abspath(__file__))
K = 9


def golden():
    with open(os.path.join(HERE, "golden", "merkle_sum_tree_case.json")) as f:
        g = json.load(f)
    leaf = (g["leaf"]["hash"], g["leaf"]["balance"])
    sib = [(e["hash"], e["balance"]) for e in g["path_elements"]]
    return leaf, sib, list(g["path_indices"])


@pytest.fixture(scope="module")
def case():
    spec = ps.default_spec(5)
    leaf, sib, idx = golden()
    lay = sy.MerkleSumTreeLayout(len(sib), K, spec)
    cs = circuits.merkle_sum_tree(spec)
    lay.check_constraint_system(cs)
    root = ps.MerkleSumTree.verify_path(leaf, ([h for h, _ in sib], [b for _, b in sib], idx), spec)
    return spec, leaf, sib, idx, lay, cs, lay.fixed_columns(), root


def run(case, leaf=None, sib=None, idx=None, assets=500, instance=None):
    spec, leaf0, sib0, idx0, lay, cs, fixed, root = case
    leaf, sib, idx = leaf or leaf0, sib or sib0, idx or idx0
    adv = lay.assign_ints(leaf, sib, idx, assets)
    inst = instance or lay.instance(leaf0, root[0], assets)
    return mock_prover.verify(cs, fixed, adv, inst, lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS), adv


def test_golden_case_is_satisfied(case):
    spec, leaf, sib, idx, lay, cs, fixed, root = case
    failures, adv = run(case)
    assert failures == []
    h, b = leaf
    for l, ((eh, eb), bit) in enumerate(zip(sib, idx)):
        h, b = ps.MerkleSumTree.verify_path((h, b), ([eh], [eb], [bit]), spec)
        kind, col, row = lay.digest_cell(l)
        assert adv[col][row] == h
        assert adv[lay.sum_cell(l)[1]][lay.sum_cell(l)[2]] == b
    assert (h, b) == root and lay.instance(leaf, root[0], 500)[0][2] == h
    assert b == 400 and adv[sy.LT][lay.lt_row] == 1
    # one changed cell of the trace is noticed (the issue's 37-row check, through the whole circuit)
    adv[sy.STATE[2]][lay.perm_row(1) + 7] += 1
    bad = mock_prover.verify(cs, fixed, adv, lay.instance(leaf, root[0], 500), lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS)
    assert mock_prover.gate_names(bad) == ["partial rounds"] and {f[3] for f in bad} == {lay.perm_row(1) + 6, lay.perm_row(1) + 7}


def _copy_failures(failures):
    return [f for f in failures if f[0] == "copy"]


def test_negative_wrong_root(case):
    spec, leaf, sib, idx, lay, *_ = case
    failures, _ = run(case, instance=lay.instance(leaf, 1000, 500))
    assert failures == [("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 2))]


def test_negative_wrong_leaf_hash(case):
    spec, leaf, sib, idx, lay, cs, fixed, root = case
    failures, _ = run(case, instance=lay.instance((1000, leaf[1]), root[0], 500))
    assert failures == [("copy", ("advice", sy.A, 0), ("instance", 0, 0))]


def test_negative_wrong_leaf_balance(case):
    spec, leaf, sib, idx, lay, cs, fixed, root = case
    failures, _ = run(case, instance=lay.instance((leaf[0], 1000), root[0], 500))
    assert failures == [("copy", ("advice", sy.B, 1), ("instance", 0, 1))]


def test_negative_non_binary_index(case):
    lay = case[4]
    failures, _ = run(case, idx=[2, 0, 0, 0, 0])
    names = mock_prover.gate_names(failures)
    assert "bool constraint" in names and "swap constraint" in names
    assert all(f[3] == lay.prove_row(0) for f in failures if f[0] == "gate")
    # the swapped hash gives another root: the only copy that fails is the one to the instance
    assert _copy_failures(failures) == [("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 2))]


def test_negative_swapped_index(case):
    lay = case[4]
    failures, _ = run(case, idx=[1, 0, 0, 0, 0])
    assert failures == [("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 2))]


def test_negative_assets_below_sum(case):
    lay = case[4]
    failures, adv = run(case, assets=200)
    assert adv[sy.LT][lay.lt_row] == 0 and adv[sy.C][lay.lt_row] == 1
    assert [f[:2] + f[3:] for f in failures] == [("gate", "check == is_lt", lay.lt_row)]


def test_sum_of_2_64_or_more_fails_the_lt_gate(case):
    spec, leaf, sib, idx, lay, *_ = case
    failures, adv = run(case, sib=[(1, 1 << 65)] + sib[1:], assets=500)          # lt = 0 and the difference does not fit 8 bytes
    root_fail = ("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 2))      # `run` keeps the golden path's root
    gates = [f for f in failures if f != root_fail]
    assert "lt gate" in mock_prover.gate_names(gates)
    assert all(f[0] == "gate" and f[1] in ("lt gate", "check == is_lt") and f[3] == lay.lt_row for f in gates)


@pytest.mark.parametrize("depth", range(1, 33))
def test_layout_properties(depth):
    spec = ps.default_spec(5)
    k = sy.MerkleSumTreeLayout.min_k(depth, spec)
    lay = sy.MerkleSumTreeLayout(depth, k, spec)
    cs = circuits.merkle_sum_tree()
    lay.check_constraint_system(cs)
    assert lay.used_rows <= (1 << k) - 6 and (k == 9 or lay.used_rows > (1 << (k - 1)) - 6)
    with pytest.raises(ValueError):
        sy.MerkleSumTreeLayout(depth, max(k - 1, 8) if k > 9 else 8, spec)
    used = {}
    for reg in lay.regions:
        assert reg.start >= 0 and reg.start + reg.height <= lay.used_rows
        for col in reg.columns:
            for row in reg.rows:
                assert (col, row) not in used, (reg.name, used.get((col, row)), col, row)
                used[(col, row)] = reg.name
    for a, b in lay.copies():
        for kind, col, row in (a, b):
            assert (kind, col) in cs.equality
            assert kind == "instance" or ((kind, col), row) in used
    # every selector row lies inside the region that enables it, at the offset the chip enables it at
    half, pairs = spec.r_f // 2, spec.r_p // 2
    offsets = {"merkle prove layer": {sy.BOOL_S: [0], sy.SWAP_S: [0], sy.SUM_S: [1]}, "pad-and-add": {sy.S_PAD: [1]},
               "permute state": {sy.S_FULL: list(range(half)) + list(range(half + pairs, 2 * half + pairs)),
                                 sy.S_PARTIAL: list(range(half, half + pairs))},
               "enforce sum to be less than total assets": {sy.LT_S: [0]}}
    expected = {c: [] for c in (sy.BOOL_S, sy.SWAP_S, sy.SUM_S, sy.LT_S, sy.S_FULL, sy.S_PARTIAL, sy.S_PAD)}
    for reg in lay.regions:
        for prefix, sel in offsets.items():
            if reg.name == prefix or reg.name.rsplit(" ", 1)[0] == prefix:
                for col, offs in sel.items():
                    assert ("fixed", col) in reg.columns and max(offs) < reg.height
                    expected[col] += [reg.start + o for o in offs]
    assert {c: sorted(r) for c, r in lay.selector_rows().items()} == {c: sorted(r) for c, r in expected.items()}
    assert len(expected[sy.S_FULL]) == depth * spec.r_f and len(expected[sy.S_PARTIAL]) == depth * pairs
    perm = [reg for reg in lay.regions if reg.name.startswith("permute state")]
    assert all(reg.start + reg.height - 1 not in expected[sy.S_FULL] + expected[sy.S_PARTIAL] for reg in perm)     # the output row has no gate
    c = sy.c_layout(depth, k, spec)
    assert c == {"used_rows": lay.used_rows, "n_advice": sy.N_ADVICE, "perm_rows": lay.perm_rows, "level_rows": lay.level_rows,
                 "lt_row": lay.lt_row, "const_row": lay.const_row}
    assert [lay.level_start[l] for l in range(depth)] == [2 + l * c["level_rows"] for l in range(depth)]
    if k > 9:
        with pytest.raises(Exception):
            sy.c_layout(depth, k - 1, spec)


def test_counted_rows():
    assert sy.MerkleSumTreeLayout.min_k(5) == 9 and sy.MerkleSumTreeLayout.min_k(20) == 10
    assert sy.MerkleSumTreeLayout(5, 9).lt_row + 1 + 25 == 243 and sy.MerkleSumTreeLayout(20, 10).used_rows == 963


# recorded from the parent commit (sha256 of repr(cs.polynomials()) and of repr of the uncompiled evaluate_h calculations, k = 9,
# extended_k = 12, delta = 7), before circuits.py gained its `spec` argument
PARENT_DIGESTS = {
    "merkle_sum_tree": ("8ca9bfc77b23519ae7b884646ede2ef3e5da2eeb2a20491ad9c2447416364ec1", "95d13b4a2daf886c764d0ad2fbc01f76e0be2763bf2a6783bb250173bf2dad8a"),
    "merkle_v3": ("cefa9a44d874aa2373295b111e2ac8ed39af1b96ea17ea8251cda97fdf67ad65", "db87119004f82e79de2d78bdf548077ef42e9ddb576b0b113f7e6b493febd718"),
    "poseidon": ("788258087692921d32c1d5a9acd30991df870d51f6f5d9ea5bc4b733548b8b6d", "b9f096e46c84b2353944fb7aed189118d278283f522635ffa1b616b4378f0f8b"),
}


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_without_a_spec_the_constraint_systems_are_unchanged(name):
    cs = getattr(circuits, name)()
    g, _ = circuits.evaluate_h_program(cs, 9, 12, 7)
    got = (hashlib.sha256(repr(cs.polynomials()).encode()).hexdigest(), hashlib.sha256(repr(g.calculations).encode()).hexdigest())
    assert got == PARENT_DIGESTS[name]
    with_spec = getattr(circuits, name)(ps.default_spec(3 if name == "merkle_v3" else 5))
    assert repr(with_spec.polynomials()) != repr(cs.polynomials())
    assert (with_spec.num_fixed, with_spec.num_advice, with_spec.equality) == (cs.num_fixed, cs.num_advice, cs.equality)


def test_permutation_columns_host_form(case):
    spec, leaf, sib, idx, lay, cs, fixed, root = case
    adv = lay.assign_ints(leaf, sib, idx, 500)
    inst = lay.instance(leaf, root[0], 500)
    cols = {"fixed": fixed, "advice": adv, "instance": inst}
    sigma = sy.permutation_cells(cs, lay)
    cells = [c for col in sigma for c in col]
    assert sorted(cells) == [(j, i) for j in range(len(cs.equality)) for i in range(lay.n)]
    moved = 0
    for j, col in enumerate(sigma):
        kind, c = cs.equality[j]
        for i, (j2, i2) in enumerate(col):
            kind2, c2 = cs.equality[j2]
            assert cols[kind][c][i] == cols[kind2][c2][i2]
            moved += (j2, i2) != (j, i)
    assert moved == len({c for pair in lay.copies() for c in pair})
    dom = EvaluationDomain(4, K)
    delta = pow(7, 1 << 28, R)
    ints = sy.permutation_columns_ints(cs, lay, dom.omega, delta)
    assert len({v for col in ints for v in col}) == len(cells)          # delta^j omega^i: all distinct
    j, i = sigma[0][0]
    assert ints[0][0] == pow(delta, j, R) * pow(dom.omega, i, R) % R and ints[3][17] == pow(delta, 3, R) * pow(dom.omega, 17, R) % R


def test_kernel_code_on_the_host_matches_assign_ints(case):
    """csrc/host_check.cpp runs the lane functions of the two witness kernels with the limb-bound checks on (-DHM_BOUNDS)."""
    import witness_hostcheck
    spec, leaf, sib, idx, lay, cs, fixed, root = case
    for assets, sibs, bits in ((500, sib, idx), (200, sib, [1, 0, 1, 1, 0]), ((1 << 64) + 5000, [(1, 1 << 64)] + sib[1:], idx), (500, [(1, 1 << 65)] + sib[1:], idx),
                               (R - 1, sib, idx), (3, [(R - 1, R - 2)] * 5, [0, 1, 0, 1, 0])):
        adv, inst = witness_hostcheck.run(spec, lay, leaf, sibs, bits, assets)
        assert adv == lay.assign_ints(leaf, sibs, bits, assets)
        r = ps.MerkleSumTree.verify_path(leaf, ([h for h, _ in sibs], [b for _, b in sibs], bits), spec)
        assert inst == [leaf[0], leaf[1], r[0], assets % R]
