"""The logUp lookup argument without a GPU: the grouping rule on every constraint system of circuits.py, the
pure-integer twin of m and phi (tests/logup_twin.py) and what it must satisfy, the argument's expressions on the twin's columns, the
proof layout and length, and the host twins of the kernels (libhm_hostcheck.so, compiled with the bound checks on) against the
integer twin at the shapes the GPU test uses."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib, circuits, evaluation as ev, poseidon as ps
from halo2_experiments_amd.domain import FR_MODULUS as R, EvaluationDomain
from halo2_experiments_amd.proof_layout import GwcTermsPlan, MultiTermsPlan, ProofLayout, TermsPlan
from halo2_experiments_amd.transcript import LOOKUPS, check_lookup
from halo2_experiments_amd.verifier import evaluate_expression, opening_points, proof_length

import logup_twin as tw

SYSTEMS = {
    "poseidon": circuits.poseidon, "merkle_v3": circuits.merkle_v3, "merkle_sum_tree": circuits.merkle_sum_tree,
    "overflow_check_v2<4,4>": lambda: circuits.overflow_check_v2(4, 4), "overflow_check_v2<16,4>": lambda: circuits.overflow_check_v2(16, 4),
    "sorted_column<4,4>": lambda: circuits.sorted_column(4, 4), "sorted_column<16,8>": lambda: circuits.sorted_column(16, 8),
    "safe_accumulator<4,4>": lambda: circuits.safe_accumulator(4, 4),
}


def rule(cs):
    """the grouping rule of the issue, stated again: -> per argument, the indices of its lookups"""
    D = cs.degree()
    deg = lambda exprs: max(circuits.degree(e) for e in exprs)
    args, open_of = [], {}
    for j, (ins, tabs) in enumerate(cs.lookups):
        key = tuple(tabs)
        g = open_of.get(key)
        if g is not None and 2 + deg(tabs) + sum(deg(cs.lookups[i][0]) for i in args[g]) + deg(ins) <= D:
            args[g].append(j)
        else:
            open_of[key] = len(args)
            args.append([j])
    return args


# ---- the grouping ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SYSTEMS) + list(circuits.CONSTRAINT_SYSTEMS))
def test_grouping_rule(name):
    cs = (SYSTEMS.get(name) or circuits.CONSTRAINT_SYSTEMS[name])()
    k = 9
    before = (cs.degree(), EvaluationDomain(cs.degree(), k).extended_k, cs.permutation_chunk_len(), cs.permutation_sets(), cs.queries())
    groups = cs.logup_arguments()
    want = rule(cs)
    assert [(tabs, ins_list) for tabs, ins_list in groups] == [(list(cs.lookups[a[0]][1]), [list(cs.lookups[j][0]) for j in a]) for a in want]
    assert sorted(j for a in want for j in a) == list(range(len(cs.lookups)))          # every lookup in exactly one argument
    assert sum(len(ins_list) for _, ins_list in groups) == len(cs.lookups)
    F = ev.Fixed
    for g, (tabs, ins_list) in enumerate(groups):
        polys = ev.logup_expressions(ins_list, tabs, lambda r: F(100, r), lambda r: F(101, r), F(102), F(103), F(104))
        assert len(polys) == 3 and max(circuits.degree(p) for p in polys) <= cs.degree(), g
        assert circuits.degree(polys[2]) == 2 + max(circuits.degree(e) for e in tabs) + sum(max(circuits.degree(e) for e in ins) for ins in ins_list)
    assert (cs.degree(), EvaluationDomain(cs.degree(), k).extended_k, cs.permutation_chunk_len(), cs.permutation_sets(), cs.queries()) == before
    assert cs.logup_arguments() == groups                                               # a pure function
    if not cs.lookups:
        assert groups == [] and proof_length(cs, lookup="logup") == proof_length(cs)
    print(name, "D", cs.degree(), "lookups", len(cs.lookups), "arguments", [len(i) for _, i in groups])


def test_the_sum_tree_groups_by_its_degree_bound():
    """computed from the rule, not written down: with D = 6 and inputs and table of degree 1 an argument holds D - 3 inputs"""
    cs = circuits.merkle_sum_tree()
    per = cs.degree() - 3
    L = len(cs.lookups)
    assert [len(i) for _, i in cs.logup_arguments()] == [per] * (L // per) + ([L % per] if L % per else [])
    assert len(cs.logup_arguments()) < L                                                # it does group


def test_two_tables_keep_their_own_open_arguments():
    """lookups into two tables, interleaved: a lookup joins the open argument of ITS table, and a full argument is closed for good"""
    A, Fx = ev.Advice, ev.Fixed
    gate = Fx(9) * A(0) * A(0) * A(0) * A(0)                                            # degree 5: two inputs per argument
    lookups = [([A(0)], [Fx(0)]), ([A(1)], [Fx(1)]), ([A(2)], [Fx(0)]), ([A(3)], [Fx(0)]), ([A(4)], [Fx(1)]), ([A(5) * A(6)], [Fx(0)]),
               ([A(7)], [Fx(0)])]
    cs = circuits.ConstraintSystem("two tables", "test", 10, 8, 0, [("g", [gate])], lookups, [])
    assert cs.degree() == 5 and rule(cs) == [[0, 2], [1, 4], [3], [5], [6]]
    assert [[ins[0] for ins in ins_list] for _, ins_list in cs.logup_arguments()] == [[A(0), A(2)], [A(1), A(4)], [A(3)], [A(5) * A(6)], [A(7)]]


# ---- the integer twin ------------------------------------------------------------------------------------------------------------------
CASES = [(rows, c, kind) for rows in tw.MULTIPLICITY_ROWS for c in (1, 3) for kind in tw.MULTIPLICITY_TABLES]


@pytest.mark.parametrize("rows, c, kind", CASES)
def test_twin_sums_to_zero_and_counts_every_input(rows, c, kind):
    table, inputs = tw.multiplicity_case(rows, c, kind)
    m, missing = tw.multiplicities(table, inputs)
    assert not missing and sum(m) == c * rows
    first = {}
    for i, v in enumerate(table):
        first.setdefault(v, i)
    assert all(m[i] == 0 for i, v in enumerate(table) if first[v] != i)                 # a repeated value: zero on its later rows
    if rows >= 2:
        assert len(first) < rows
    beta = random.Random(rows).randrange(R)
    phi = tw.running_sum(table, inputs, m, beta)
    assert len(phi) == rows + 1 and phi[0] == 0 and phi[rows] == 0
    assert all(tw.third_polynomial(table, inputs, m, phi, beta, i) == 0 for i in range(rows))


def test_twin_catches_an_input_changed_without_its_multiplicity():
    table, inputs = tw.multiplicity_case(26, 3, "range")
    m, _ = tw.multiplicities(table, inputs)
    beta = 0x1234567890ABCDEF
    row = 7
    other = next(v for v in table if v != inputs[1][row])                               # another value of the table
    before = tw.running_sum(table, inputs, m, beta)
    inputs[1][row] = other
    assert tw.third_polynomial(table, inputs, m, before, beta, row) != 0                # the columns as they were: that row fails
    assert all(tw.third_polynomial(table, inputs, m, before, beta, i) == 0 for i in range(26) if i != row)
    phi = tw.running_sum(table, inputs, m, beta)                                        # the prover's phi with the stale m
    assert phi[26] != 0                                                                 # l_last * phi fails
    honest_m, _ = tw.multiplicities(table, inputs)
    honest = tw.running_sum(table, inputs, honest_m, beta)
    assert honest[26] == 0
    # with the columns the verifier would hold the prover to (phi of the honest m, the stale m) the third polynomial fails on that row
    bad = [i for i in range(26) if tw.third_polynomial(table, inputs, m, honest, beta, i)]
    assert bad and set(bad) <= {i for i in range(26) if m[i] != honest_m[i]}
    assert tw.multiplicities(table, [[max(table) + 1] * 26])[1]                         # a value outside the table is missing


def test_expressions_vanish_on_the_twin_columns_and_not_on_a_forged_row():
    """evaluation.logup_expressions, evaluated row by row by the verifier's expression evaluator on the twin's m and phi: the three
    polynomials are zero on every row of an honest witness; theta compresses two-column inputs and tables"""
    rng = random.Random(5)
    u, n = 26, 32
    t0, t1 = [rng.randrange(40) for _ in range(u)], [rng.randrange(R) for _ in range(u)]
    picks = [[rng.randrange(u) for _ in range(u)] for _ in range(2)]
    theta, beta = rng.randrange(R), rng.randrange(R)
    table = [(t0[i] * theta + t1[i]) % R for i in range(u)]
    inputs = [[table[p] for p in pick] for pick in picks]
    m, missing = tw.multiplicities(table, inputs)
    phi = tw.running_sum(table, inputs, m, beta)
    assert not missing
    A, F = ev.Advice, ev.Fixed
    ins_list = [[A(0), A(1)], [A(2), A(3)]]
    polys = ev.logup_expressions(ins_list, [F(0), F(1)], lambda r: F(2, r), lambda r: F(3, r), F(4), F(5), F(6))
    adv = [[t0[p] for p in picks[0]], [t1[p] for p in picks[0]], [t0[p] for p in picks[1]], [t1[p] for p in picks[1]]]
    pad = lambda col: list(col) + [rng.randrange(R) for _ in range(n - len(col))]      # blinding rows
    fixed = [pad(t0), pad(t1), phi + [rng.randrange(R) for _ in range(n - u - 1)], pad(m), [1] + [0] * (n - 1),
             [int(i == u) for i in range(n)], [int(i < u) for i in range(n)]]
    adv = [pad(col) for col in adv]

    def values(row):
        leaf = lambda kind, column, r: (fixed if kind == "fixed" else adv)[column][(row + r) % n]
        return [evaluate_expression(p, leaf, {"Theta": theta, "Beta": beta, "Gamma": 0}) for p in polys]

    assert all(values(row) == [0, 0, 0] for row in range(n))
    fixed[3][4] = (fixed[3][4] + 1) % R                                                 # a forged multiplicity
    assert values(4)[2] != 0 and all(values(row) == [0, 0, 0] for row in range(n) if row != 4)


# ---- layout and length -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["merkle_sum_tree", "overflow_check_v2<4,4>", "sorted_column<4,4>", "poseidon", "safe_accumulator<4,4>"])
@pytest.mark.parametrize("encoding", ["halo2", "evm"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_layout_and_length(name, encoding, multiopen):
    cs, k = SYSTEMS[name](), 9
    lay = ProofLayout(cs, k, encoding, multiopen=multiopen, lookup="logup")
    G, L = len(cs.logup_arguments()), len(cs.lookups)
    w = 2 if encoding == "evm" else 1
    assert 32 * lay.slots == proof_length(cs, 1, encoding, multiopen, k, "logup") and (lay.L, lay.G) == (0, G)
    q = opening_points(cs, k, "logup") - opening_points(cs, k) if multiopen == "gwc" else 0      # logUp names no rotation -1
    assert proof_length(cs, 1, encoding, multiopen, k) - 32 * lay.slots == 32 * (w * (3 * L - 2 * G) + 5 * L - 3 * G) - 32 * w * q
    assert [key for key in lay.point_keys if key[0] == "logup_m"] == [("logup_m", g) for g in range(G)]
    assert [key for key in lay.point_keys if key[0] == "logup_phi"] == [("logup_phi", g) for g in range(G)]
    assert not [key for key in lay.point_keys if key[0].startswith("lookup")]
    assert [e for e in lay.eval_keys if e[0][0].startswith("logup")] == [e for g in range(G) for e in
                                                                         ((("logup_phi", g), 0), (("logup_phi", g), 1), (("logup_m", g), 0))]
    assert sum(a for a, _ in lay.transcript_schedule()) == lay.slots
    assert lay.point_keys[:cs.num_advice] == [("advice", i) for i in range(cs.num_advice)]       # C_p and C_id stay where they are
    if not L:
        halo2 = ProofLayout(cs, k, encoding, multiopen=multiopen)
        assert (lay.point_keys, lay.eval_keys, lay.queries) == (halo2.point_keys, halo2.eval_keys, halo2.queries)
    if multiopen == "shplonk" and encoding == "halo2":
        multi = ProofLayout(cs, k, circuits=3, lookup="logup")
        assert 32 * multi.slots == proof_length(cs, 3, lookup="logup", k=k) and multi.lane.lookup == "logup"
    plan = GwcTermsPlan if multiopen == "gwc" else TermsPlan
    with pytest.raises(ValueError, match="halo2"):
        plan(lay, 1, [])
    with pytest.raises(ValueError, match="halo2"):
        MultiTermsPlan(lay, 1, [])


def test_the_lookup_keyword_is_checked():
    assert LOOKUPS == ("halo2", "logup") and check_lookup("logup", "t") == "logup"
    cs = circuits.overflow_check_v2(4, 4)
    for call in (lambda: check_lookup("plookup", "t"), lambda: proof_length(cs, lookup="mv"), lambda: ProofLayout(cs, 5, lookup="mv"),
                 lambda: circuits.evaluate_h_program(cs, 5, 7, 7, lookup="mv")):
        with pytest.raises(ValueError, match="lookup must be"):
            call()


def test_the_h_program_has_two_columns_per_argument():
    cs = circuits.merkle_sum_tree()
    G = len(cs.logup_arguments())
    _, halo2 = circuits.evaluate_h_program(cs, 9, 12, 7, divide=False)
    g, lay = circuits.evaluate_h_program(cs, 9, 12, 7, divide=False, lookup="logup")
    assert lay.lookup0 == halo2.lookup0 and lay.t_inv == lay.lookup0 + 2 * G and halo2.t_inv == halo2.lookup0 + 3 * len(cs.lookups)


# ---- the host twins of the kernels, under bound tracking ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostcheck():
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.hc_logup_multiplicities.restype = ctypes.c_int
    lib.hc_logup_multiplicities.argtypes = [u32p, u32p, ctypes.c_uint32, ctypes.c_uint64, u32p]
    lib.hc_grand_sum.restype = ctypes.c_int
    lib.hc_grand_sum.argtypes = [u32p, ctypes.c_uint64, u32p]
    lib.hc_logup_count_bits.restype = ctypes.c_uint32
    lib.hc_logup_count_bits.argtypes = []
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def host_multiplicities(lib, table, inputs):
    rows = len(table)
    t = np.ascontiguousarray(ps.ints_to_words(table)).view(np.uint32)
    f = np.ascontiguousarray(ps.ints_to_words([v for col in inputs for v in col])).view(np.uint32)
    m = np.zeros(rows * 8, dtype=np.uint32)
    rc = lib.hc_logup_multiplicities(_p(t), _p(f), len(inputs), rows, _p(m))
    return ps.words_to_ints(m.view(np.uint64).reshape(rows, 4)), rc


@pytest.mark.parametrize("rows, c, kind", CASES)
def test_host_multiplicities_equal_the_twin(hostcheck, rows, c, kind):
    table, inputs = tw.multiplicity_case(rows, c, kind)
    got, rc = host_multiplicities(hostcheck, table, inputs)
    assert rc == 0 and got == tw.multiplicities(table, inputs)[0]


def test_host_multiplicities_report_a_missing_input_and_refuse_bad_shapes(hostcheck):
    assert hostcheck.hc_logup_count_bits() == tw.COUNT_BITS
    table, inputs = tw.multiplicity_case(26, 3, "range")
    inputs[2][25] = R - 1
    got, rc = host_multiplicities(hostcheck, table, inputs)
    assert rc == 1 and got == tw.multiplicities(table, inputs)[0] and sum(got) == 3 * 26 - 1
    z = np.zeros(8, dtype=np.uint32)
    assert hostcheck.hc_logup_multiplicities(_p(z), _p(z), 1, 0, _p(z)) == -1
    assert hostcheck.hc_logup_multiplicities(_p(z), _p(z), 0, 1, _p(z)) == -1
    assert hostcheck.hc_logup_multiplicities(_p(z), _p(z), 2, 1 << 31, _p(z)) == -1   # c * rows = 2^32


@pytest.mark.parametrize("values", tw.GRAND_SUM_VALUES)
@pytest.mark.parametrize("n", tw.GRAND_SUM_LENGTHS)
def test_host_grand_sum_equals_the_twin(hostcheck, n, values):
    column = tw.grand_sum_columns(n, values, 1)[0]
    terms = np.ascontiguousarray(ps.ints_to_words(column)).view(np.uint32).reshape(-1)
    out = np.zeros(n * 8, dtype=np.uint32)
    assert hostcheck.hc_grand_sum(_p(terms), n, _p(out)) == 0
    assert ps.words_to_ints(out.view(np.uint64).reshape(n, 4)) == tw.prefix_sums(column)
    assert hostcheck.hc_grand_sum(_p(terms), n, _p(terms)) == 0                          # in place
    assert np.array_equal(terms, out)
