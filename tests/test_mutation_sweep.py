"""The mutation sweep on the host (tests/mutation_cases.py): every advice cell of the four circuits plus a delta, judged by the tests' own
checker, must be caught exactly where ``EXPECTED`` -- written from the reference's chips, not from the constraint system -- says a gate or
a copy catches it, and by a lookup exactly where the changed value leaves its table.  An omitted gate, copy or lookup in circuits.py or
in a layout's ``copies()`` changes these sets; the negative controls at the end take one of each away and show which cells move."""
import dataclasses

import pytest

import mutation_cases as mc


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_constrained_cells_are_the_expected_ones(name):
    c = mc.case(name)
    want = mc.expected_sets(c)
    cells_total, constrained_total, zero_total = mc.TOTALS[name]
    assert c.cs.num_advice * c.n == cells_total
    sets = {}
    for delta_name, delta in mc.DELTAS.items():
        cells, verdicts = mc.verdicts(name, delta_name)
        got = sets[delta_name] = mc.caught_by(cells, verdicts)
        assert len(cells) == len(set(cells)) == mc.SWEPT[name] and want["constrained"] <= set(cells)
        for kind in ("gate", "copy", "constrained"):
            assert got[kind] == want[kind], (delta_name, kind, sorted(got[kind] ^ want[kind])[:10])
        assert got["lookup"] == mc.expected_lookup_set(c, cells, delta), delta_name
        assert len(got["constrained"]) == constrained_total
        # a blinding row is never checked, and no usable row reads one
        assert not any(row >= c.usable for _, row in got["failing"])
    assert sets["one"]["constrained"] == sets["random"]["constrained"]
    # every cell that holds something is constrained (over ALL rows, the ones the sum tree's sweep leaves out included)
    nonzero = {(col, row) for col in range(c.cs.num_advice) for row in range(c.n) if c.advice[col][row]}
    assert nonzero <= want["constrained"]
    if zero_total is not None:
        zero = sorted(want["constrained"] - nonzero)
        assert len(zero) == zero_total
        if name == "poseidon":
            assert zero == [(col, row) for col in range(4) for row in (2, 3)]
        if name == "merkle_v3":
            assert zero == [(2, 44), (3, 3), (3, 4), (3, 46), (3, 47), (4, 3), (4, 4), (4, 46), (4, 47)]
        if name == "merkle_sum_tree":
            assert zero == [(4, 2)] + [(col, row) for col in (5, 6, 7, 8) for row in (4, 5, 47, 48)]
    assert mc.FREE_ASSIGNED[name] == []
    # the lookups: a random element always leaves the table; plus 1 only from the table's last entry
    lookup_cells = {(col, row) for col, row in cells if col in mc.LOOKUP_COLUMNS[name] and row < c.usable}
    assert sets["random"]["lookup"] == lookup_cells
    if name == "merkle_sum_tree":
        assert sets["one"]["lookup"] == set() and len(lookup_cells) == 8 * 93 and c.lay.lt_row == 88
    if name == "overflow_check_v2":
        assert sets["one"]["lookup"] == {cell for cell in lookup_cells if c.advice[cell[0]][cell[1]] == 15} and len(sets["one"]["lookup"]) >= 4
        assert len(lookup_cells) == 104 and sorted(got["constrained"]) == [(col, row) for col in range(5) for row in range(26)]


def test_the_sum_tree_sweep_holds_every_constrained_cell():
    c = mc.case("merkle_sum_tree")
    rows = mc.swept_rows(c)
    assert rows == list(range(91)) + list(range(504, 512)) and len(mc.mutants(c)) == 99 * 20
    assert mc.expected_sets(c)["constrained"] <= set(mc.mutants(c))
    assert sorted(c.advice[4][r] for r in (2, 45)) == [0, 1]             # one index bit 0, one index bit 1


def test_instance_cells_are_held_by_their_copies():
    for name in mc.NAMES:
        c = mc.case(name)
        cells = mc.instance_mutants(c)
        assert len(cells) == {"poseidon": 1, "merkle_v3": 2, "merkle_sum_tree": 4, "overflow_check_v2": 0}[name]
        named = [sum(("instance", 0, row) in pair for pair in c.copies) for _, row in cells]
        assert mc.host_verdicts(c, cells, 1, kind="instance") == [(0, n, 0, 0) for n in named] and all(named)


# ---- negative controls: a lost constraint moves exactly these cells ------------------------------------------------------------------
def _sweep(c, delta=1, **changed):
    cells = mc.mutants(c)
    return mc.caught_by(cells, mc.host_verdicts(c, cells, delta, **changed))


def _without_gate(cs, name):
    assert name in [g for g, _ in cs.gates]
    return dataclasses.replace(cs, gates=[(g, polys) for g, polys in cs.gates if g != name])


def test_control_a_lost_sum_gate():
    """without "sum constraint" the two sum cells (column e, row 1 of each "merkle prove layer") are no longer caught by a gate.  They
    stay constrained: each is still copied on (to the next level's balance, to the lt row), which is why the sweep pins the kinds and
    not only the union."""
    c = mc.case("merkle_sum_tree")
    base = mc.caught_by(*mc.verdicts(c.name, "one"))
    got = _sweep(c, cs=_without_gate(c.cs, "sum constraint"))
    lost = {(4, 3), (4, 46)}
    assert lost == {c.lay.sum_cell(l)[1:] for l in range(2)}
    assert base["gate"] - got["gate"] == lost and got["gate"] <= base["gate"]
    assert got["copy"] == base["copy"] and got["constrained"] == base["constrained"] and lost <= got["copy"]


def test_control_a_lost_is_lt_gate():
    """without "check == is_lt" the check cell (column c of the lt row) is free, and nothing else moves"""
    c = mc.case("merkle_sum_tree")
    base = mc.caught_by(*mc.verdicts(c.name, "one"))
    got = _sweep(c, cs=_without_gate(c.cs, "check == is_lt"))
    assert base["constrained"] - got["constrained"] == {(2, 88)} and got["constrained"] <= base["constrained"]
    assert base["gate"] - got["gate"] == {(2, 88)} and got["copy"] == base["copy"]


@pytest.mark.parametrize("name", ["merkle_v3", "merkle_sum_tree"])
def test_control_a_lost_level_copy(name):
    """without the copy of level 0's digest into level 1 its two ends -- the digest cell and column a of level 1's first row -- are no
    longer caught by a copy; both stay caught by gates (the last full round, the swap gate), so the union does not move"""
    c = mc.case(name)
    base = mc.caught_by(*mc.verdicts(name, "one"))
    digest, entry = c.lay.digest_cell(0), ("advice", 0, c.lay.prove_row(1))
    assert (digest, entry) in c.copies
    got = _sweep(c, copies=[pair for pair in c.copies if pair != (digest, entry)])
    lost = {"merkle_v3": {(3, 43), (0, 44)}, "merkle_sum_tree": {(5, 44), (0, 45)}}[name]
    assert lost == {digest[1:], entry[1:]}
    assert base["copy"] - got["copy"] == lost and got["copy"] <= base["copy"]
    assert got["gate"] == base["gate"] and got["constrained"] == base["constrained"]


def test_control_a_lost_lookup():
    """without the range lookup of limb column 3, a random element in that column is caught by the gate alone on all 26 rows"""
    c = mc.case("overflow_check_v2")
    base = mc.caught_by(*mc.verdicts(c.name, "random"))
    cs = dataclasses.replace(c.cs, lookups=c.cs.lookups[:2] + c.cs.lookups[3:])
    assert c.cs.lookups[2][0][0].column == 3
    got = _sweep(c, delta=mc.DELTAS["random"], cs=cs, tables=c.tables[:2] + c.tables[3:])
    assert base["lookup"] - got["lookup"] == {(3, row) for row in range(26)} and got["lookup"] <= base["lookup"]
    assert got["gate"] == base["gate"] and got["constrained"] == base["constrained"]
