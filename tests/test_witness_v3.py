"""The MerkleTreeV3 and Poseidon circuit witnesses on the CPU: synthesis.MerkleTreeV3Layout / PoseidonCircuitLayout (assign_ints,
fixed_columns, copies) against the tests' own MockProver, the reference's cases (/root/reference/src/circuits/merkle_v3.rs:91-93,
circuits/poseidon.rs:71-98) on BN256 with their negatives, the layouts' properties for every depth against the C layout functions,
and the kernels' lane functions compiled for the host against assign_ints."""
import pytest

from halo2_experiments_amd import circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R

import mock_prover
import poseidon_checker

K = 10
LEAF, ELEMENTS, INDICES = 99, [1, 5, 6, 9, 9], [0, 0, 0, 0, 0]
V3 = sy.MerkleTreeV3Layout
PC = sy.PoseidonCircuitLayout


@pytest.fixture(scope="module")
def case():
    spec = ps.default_spec(3)
    lay = V3(len(ELEMENTS), K, spec)
    cs = circuits.merkle_v3(spec)
    lay.check_constraint_system(cs)
    root = ps.MerkleTree.verify_path(LEAF, (ELEMENTS, INDICES), spec)
    return spec, lay, cs, lay.fixed_columns(), root


def busy_rows(lay):
    """every row a region touches, the first free row and the last usable one: the rest holds zeros in every column"""
    return sorted({r for reg in lay.regions for r in reg.rows} | {lay.used_rows, lay.n - sy.BLINDING_ROWS - 1})


def verify(case, adv, instance):
    spec, lay, cs, fixed, root = case
    return mock_prover.verify(cs, fixed, adv, instance, lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS, rows=busy_rows(lay))


def test_column_indices_follow_the_constraint_systems():
    cs = circuits.merkle_v3()
    assert (cs.num_advice, cs.num_fixed, cs.num_instance) == (7, 11, 1) == (V3.N_ADVICE, V3.N_FIXED, 1)
    assert (V3.A, V3.B, V3.C, V3.STATE, V3.PARTIAL_SBOX) == (0, 1, 2, (3, 4, 5), 6)
    assert (V3.BOOL_S, V3.SWAP_S, V3.RC_A, V3.RC_B, V3.S_FULL, V3.S_PARTIAL, V3.S_PAD) == (0, 1, (2, 3, 4), (5, 6, 7), 8, 9, 10)
    assert cs.equality == [("advice", 0), ("advice", 1), ("advice", 2), ("instance", 0), ("advice", 3), ("advice", 4), ("advice", 5), ("fixed", 5)]
    V3(5, 8).check_constraint_system(cs)
    pcs = circuits.poseidon()
    assert (pcs.num_advice, pcs.num_fixed, pcs.num_instance) == (6, 13, 1) == (PC.N_ADVICE, PC.N_FIXED, 1)
    assert (PC.STATE, PC.PARTIAL_SBOX, PC.RC_A, PC.RC_B) == ((0, 1, 2, 3, 4), 5, (0, 1, 2, 3, 4), (5, 6, 7, 8, 9))
    assert (PC.S_FULL, PC.S_PARTIAL, PC.S_PAD) == (10, 11, 12)
    assert pcs.equality == [("advice", c) for c in range(5)] + [("fixed", 5), ("instance", 0)]
    PC(6).check_constraint_system(pcs)
    for lay, other in ((V3(5, 8), pcs), (PC(6), cs), (V3(5, 8), circuits.merkle_sum_tree()), (PC(6), circuits.merkle_sum_tree())):
        with pytest.raises(ValueError):
            lay.check_constraint_system(other)
    # the selectors sit where the gates read them: every polynomial of a Pow5 gate is `Fixed(selector) * (...)`
    for cs_, lay_ in ((circuits.merkle_v3(ps.default_spec(3)), V3), (circuits.poseidon(ps.default_spec(5)), PC)):
        sel = {name: {p.a.column for p in polys} for name, polys in cs_.gates if name in ("full round", "partial rounds", "pad-and-add")}
        assert sel == {"full round": {lay_.S_FULL}, "partial rounds": {lay_.S_PARTIAL}, "pad-and-add": {lay_.S_PAD}}
    swap = dict(circuits.merkle_v3().gates)["swap constraint"][0]
    assert swap.a.column == V3.SWAP_S and dict(circuits.merkle_v3().gates)["bool constraint"][0].a.a.column == V3.BOOL_S


def test_counted_rows():
    assert (V3.rows_needed(5), V3.min_k(5), V3.rows_needed(20), V3.min_k(20)) == (231, 8, 921, 10)
    assert (V3(5, 8).used_rows, V3(20, 10).used_rows) == (231, 921)
    assert (PC.rows_needed(), PC.min_k(), PC(6).used_rows) == (48, 6, 48)
    assert V3.rows_needed(3, ps.Spec(3, 2, 4, 10)) == 1 + 3 * (6 + 4 + 5 + 1) + 9


@pytest.mark.parametrize("depth", range(1, 33))
def test_layout_properties_and_the_c_layout(depth):
    spec = ps.default_spec(3)
    k = V3.min_k(depth, spec)
    lay = V3(depth, k, spec)
    cs = circuits.merkle_v3()
    lay.check_constraint_system(cs)
    assert lay.used_rows == V3.rows_needed(depth, spec) == 1 + depth * (6 + lay.perm_rows) + 3 * depth
    assert lay.used_rows <= (1 << k) - 6 and lay.used_rows > (1 << (k - 1)) - 6
    with pytest.raises(ValueError):
        V3(depth, k - 1, spec)
    with pytest.raises(Exception):
        sy.merkle_c_layout(depth, k - 1, spec)
    c = sy.merkle_c_layout(depth, k, spec)
    assert c == {"used_rows": lay.used_rows, "n_advice": V3.N_ADVICE, "perm_rows": lay.perm_rows, "level_rows": lay.level_rows,
                 "const_row": lay.const_row}
    assert lay.level_start == [1 + l * c["level_rows"] for l in range(depth)]
    assert [lay.init_row(l) for l in range(depth)] == [s + 2 for s in lay.level_start]
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
    half, pairs = spec.r_f // 2, spec.r_p // 2
    offsets = {"merkle prove layer": {V3.BOOL_S: [0], V3.SWAP_S: [0]}, "pad-and-add": {V3.S_PAD: [1]},
               "permute state": {V3.S_FULL: list(range(half)) + list(range(half + pairs, 2 * half + pairs)), V3.S_PARTIAL: list(range(half, half + pairs))}}
    expected = {c: [] for c in (V3.BOOL_S, V3.SWAP_S, V3.S_FULL, V3.S_PARTIAL, V3.S_PAD)}
    for reg in lay.regions:
        for prefix, sel in offsets.items():
            if reg.name.rsplit(" ", 1)[0] == prefix:
                for col, offs in sel.items():
                    assert ("fixed", col) in reg.columns and max(offs) < reg.height
                    expected[col] += [reg.start + o for o in offs]
    assert {c: sorted(r) for c, r in lay.selector_rows().items()} == {c: sorted(r) for c, r in expected.items()}
    assert len(expected[V3.S_FULL]) == depth * spec.r_f and len(expected[V3.S_PARTIAL]) == depth * pairs


def test_poseidon_layout_and_the_c_layout():
    spec = ps.default_spec(5)
    lay = PC(6, spec)
    assert [(r.name, r.start, r.height) for r in lay.regions] == [
        ("load private inputs", 0, 1), ("copy input cells to hash input cells", 1, 1), ("initial state", 2, 1), ("pad-and-add", 3, 3),
        ("permute state", 6, 37), ("constants", 43, 5)]
    for k in (6, 7, 11):
        assert sy.poseidon_c_layout(k, spec) == {"used_rows": 48, "n_advice": 6, "perm_rows": 37, "level_rows": 43, "const_row": 43}
    with pytest.raises(ValueError):
        PC(5, spec)
    with pytest.raises(Exception):
        sy.poseidon_c_layout(5, spec)
    small = ps.Spec(5, 4, 4, 10)
    assert PC(5, small).used_rows == 2 + 4 + 10 + 5 and sy.poseidon_c_layout(5, small)["used_rows"] == 21
    with pytest.raises(ValueError):
        PC(6, ps.default_spec(3))
    with pytest.raises(ValueError):
        V3(5, 8, spec)
    with pytest.raises(ValueError):
        V3(0, 8)
    with pytest.raises(ValueError):
        V3(33, 12)
    with pytest.raises(ValueError):
        V3(2, 8, ps.Spec(3, 2, 8, 55))
    cs = circuits.poseidon()
    for a, b in lay.copies():
        assert all((kind, col) in cs.equality for kind, col, _ in (a, b))


def test_reference_case_is_satisfied(case):
    spec, lay, cs, fixed, root = case
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    assert verify(case, adv, lay.instance(LEAF, root)) == []
    # the same on every usable row once, not only on the rows the regions touch
    assert mock_prover.verify(cs, fixed, adv, lay.instance(LEAF, root), lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS) == []
    rc, mds, _ = spec.constants()
    h = LEAF
    for l, e in enumerate(ELEMENTS):
        h = poseidon_checker.digest([h, e], rc, mds, spec.r_f, spec.r_p)
        _, col, row = lay.digest_cell(l)
        assert adv[col][row] == h
    assert h == root == lay.instance(LEAF, root)[0][1]


def test_negative_wrong_public_root(case):
    spec, lay, cs, fixed, root = case
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    assert verify(case, adv, lay.instance(LEAF, 0)) == [("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 1))]


def test_negative_wrong_leaf_in_the_instance(case):
    spec, lay, cs, fixed, root = case
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    assert verify(case, adv, lay.instance(1000, root)) == [("copy", ("advice", V3.A, 0), ("instance", 0, 0))]


def test_negative_index_two(case):
    """An index of 2 fails the bool gate.  On the reference's path the swap gate sees it too (2 c (b - a) - 2 (b - a) = 2 (b - a) for
    c = 2 and a swapped pair) and the swapped hash changes the root; where the path element equals the node the swap is vacuous and
    the bool gate is the only failure."""
    spec, lay, cs, fixed, root = case
    failures = verify(case, lay.assign_ints(LEAF, ELEMENTS, [2, 0, 0, 0, 0]), lay.instance(LEAF, root))
    gates = [f for f in failures if f[0] == "gate"]
    assert mock_prover.gate_names(gates) == ["bool constraint", "swap constraint"] and all(f[3] == lay.prove_row(0) for f in gates)
    assert [f for f in failures if f[0] != "gate"] == [("copy", lay.digest_cell(lay.depth - 1), ("instance", 0, 1))]
    elements = [LEAF] + ELEMENTS[1:]
    same_root = ps.MerkleTree.verify_path(LEAF, (elements, INDICES), spec)
    failures = verify(case, lay.assign_ints(LEAF, elements, [2, 0, 0, 0, 0]), lay.instance(LEAF, same_root))
    assert failures == [("gate", "bool constraint", 0, lay.prove_row(0))]
    failures = verify(case, lay.assign_ints(LEAF, ELEMENTS, [0, 0, 2, 0, 0]), lay.instance(LEAF, root))
    assert {f[3] for f in failures if f[0] == "gate"} == {lay.prove_row(2)}


def test_negative_index_one_without_swapping(case):
    spec, lay, cs, fixed, root = case
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    adv[V3.C][lay.prove_row(1)] = 1                      # the index says "right child", the pair below stays as it was
    assert verify(case, adv, lay.instance(LEAF, root)) == [("gate", "swap constraint", 0, lay.prove_row(1))]


def test_negative_one_changed_state_cell(case):
    spec, lay, cs, fixed, root = case
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    adv[V3.STATE[2]][lay.perm_row(1) + 7] += 1           # a partial-round row: read by its own gate and by the row above
    bad = verify(case, adv, lay.instance(LEAF, root))
    assert mock_prover.gate_names(bad) == ["partial rounds"] and {f[3] for f in bad} == {lay.perm_row(1) + 6, lay.perm_row(1) + 7}
    adv = lay.assign_ints(LEAF, ELEMENTS, INDICES)
    adv[V3.STATE[0]][lay.perm_row(4) + 2] += 1           # a full-round row
    bad = verify(case, adv, lay.instance(LEAF, root))
    assert mock_prover.gate_names(bad) == ["full round"] and {f[3] for f in bad} == {lay.perm_row(4) + 1, lay.perm_row(4) + 2}


def test_mixed_indices_are_satisfied(case):
    spec, lay, cs, fixed, root = case
    bits = [1, 0, 1, 1, 0]
    r = ps.MerkleTree.verify_path(LEAF, (ELEMENTS, bits), spec)
    assert r != root
    adv = lay.assign_ints(LEAF, ELEMENTS, bits)
    assert verify(case, adv, lay.instance(LEAF, r)) == []
    assert [adv[V3.C][lay.prove_row(l)] for l in range(5)] == bits
    assert (adv[V3.A][lay.prove_row(0) + 1], adv[V3.B][lay.prove_row(0) + 1]) == (ELEMENTS[0], LEAF)


def test_poseidon_circuit_reference_case():
    spec = ps.default_spec(5)
    lay = PC(7, spec)
    cs = circuits.poseidon(spec)
    lay.check_constraint_system(cs)
    msg = [99, 99, 99, 99]
    rc, mds, _ = spec.constants()
    digest = poseidon_checker.digest(msg, rc, mds, spec.r_f, spec.r_p)
    assert digest == ps.hash_ints(spec, msg)
    adv, fixed = lay.assign_ints(msg), lay.fixed_columns()
    _, col, row = lay.digest_cell()
    assert adv[col][row] == digest
    usable = lay.n - sy.BLINDING_ROWS
    assert mock_prover.verify(cs, fixed, adv, lay.instance(digest), lay.copies(), lay.n, usable) == []
    assert mock_prover.verify(cs, fixed, adv, lay.instance(digest + 1), lay.copies(), lay.n, usable) == [("copy", lay.digest_cell(), ("instance", 0, 0))]
    adv[PC.STATE[1]][PC.COPY_ROW] += 1                   # a hash input that is not the private input
    bad = mock_prover.verify(cs, fixed, adv, lay.instance(digest), lay.copies(), lay.n, usable)
    assert sorted(bad) == sorted([("copy", ("advice", 1, PC.LOAD_ROW), ("advice", 1, PC.COPY_ROW)), ("copy", ("advice", 1, PC.COPY_ROW), ("advice", 1, lay.pad_row() + 1))])


def test_permutation_cells_take_the_new_layouts(case):
    spec, lay, cs, fixed, root = case
    cols = {"fixed": fixed, "advice": lay.assign_ints(LEAF, ELEMENTS, INDICES), "instance": lay.instance(LEAF, root)}
    sigma = sy.permutation_cells(cs, lay)
    assert sorted(c for col in sigma for c in col) == [(j, i) for j in range(len(cs.equality)) for i in range(lay.n)]
    moved = 0
    for j, col in enumerate(sigma):
        kind, c = cs.equality[j]
        for i, (j2, i2) in enumerate(col):
            kind2, c2 = cs.equality[j2]
            assert cols[kind][c][i] == cols[kind2][c2][i2]
            moved += (j2, i2) != (j, i)
    assert moved == len({c for pair in lay.copies() for c in pair})
    play = PC(6)
    assert len(sy.permutation_cells(circuits.poseidon(), play)) == 7


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_kernel_code_on_the_host_matches_assign_ints(depth):
    """csrc/host_check.cpp runs the lane functions of the new kernels with the limb-bound checks on (-DHM_BOUNDS)."""
    import witness_v3_hostcheck as hc
    spec = ps.default_spec(3)
    lay = V3(depth, V3.min_k(depth, spec), spec)
    elements = (ELEMENTS + [R - 1])[:depth]
    for leaf, bits in ((LEAF, [0] * depth), (LEAF, [1, 0, 1, 1, 0][:depth]), (R - 1, [1] * depth)):
        adv, inst = hc.run_merkle(spec, lay, leaf, elements, bits)
        assert adv == lay.assign_ints(leaf, elements, bits)
        assert inst == [leaf, ps.MerkleTree.verify_path(leaf, (elements, bits), spec)]
    # the path's nodes read from a built tree (integers from the tests' checker) instead of the chain
    rc, mds, _ = spec.constants()
    leaves = [(7 * i + 3) % R for i in range(1 << depth)]
    levels = [leaves]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([poseidon_checker.digest([lv[2 * i], lv[2 * i + 1]], rc, mds, spec.r_f, spec.r_p) for i in range(len(lv) // 2)])
    index = (1 << depth) - 2 if depth > 1 else 1
    sib = [levels[l][(index >> l) ^ 1] for l in range(depth)]
    bits = [(index >> l) & 1 for l in range(depth)]
    adv, inst = hc.run_merkle(spec, lay, leaves[index], sib, bits, nodes=[v for lv in levels for v in lv])
    assert adv == lay.assign_ints(leaves[index], sib, bits) and inst == [leaves[index], levels[-1][0]]


def test_poseidon_kernel_code_on_the_host_matches_assign_ints():
    import witness_v3_hostcheck as hc
    spec = ps.default_spec(5)
    lay = PC(6, spec)
    for msg in ([99] * 4, [0, 1, R - 1, R - 2]):
        adv, inst = hc.run_poseidon(spec, lay, msg)
        assert adv == lay.assign_ints(msg) and inst == [ps.hash_ints(spec, msg)]
