"""CPU: every primitive of csrc/ff29.h and csrc/g1.h, op by op on raw limbs, against Python integers (ff29_model.py) with the operands AT
the documented limits: coordinates that really lie in [11p, 12p), lazy limbs that really are 2^31 - 1, column sums at the last
admissible value, subtrahends at the subtraction constants, every exceptional branch of the addition laws under every representative.

The ops run in a stand-alone program (unit_ops_host.cpp over csrc/unit_ops.h) built with AddressSanitizer and UBSan, once plain
and once with -DHM_BOUNDS, where every operand is declared at the class the case states: a precondition of the tracker that an
admissible case violates, or a result outside the bound the tracker derives, aborts that child with its message.

Branch coverage, from the model alone: g1_madd_nz's hh = h^2 comes out as p and as 2p among the equal-x cases.  Its rr0 = r0^2,
and the squares of g1_add_nz and g1x_madd_fast, can only come out as p: r0 = +-S2 - Y1 + 6p is k p with k <= 9, and the square
of k p is below (k^2 / 169.28 + 1) p, which reaches 2p only from k = 14 (169.28 = 2^261 / p); likewise k <= 4 for g1_add_nz
(U2 - U1 + 3p) and k <= 10 for g1x_madd_fast (U2 - X1 + 9p).  The test asserts exactly that.

The -DHM_BOUNDS build also writes out the (vb, lb, tb) the tracker derived for every field result, and the comparison holds them
against the result's exact value: that is the check of the tracker's own double value bounds.

Constructed cases ("top_limb"): a stored X1 / Y1 in the last 2^232-block of its class against a U2 / S2 whose top limb is 0, for
g1_madd_nz, g1x_madd_fast and g1_neg_affine.  What they show about the subtraction constants: a constant one multiple of p
smaller (fe_sub<12,29> for g1_madd_nz's h) makes the top limb of the difference wrap to 2^32 - 1 on exactly these cases, and
fe_norm's carry into the top limb wraps it back, because the difference U2 - X1 + 12p is still positive as an integer -- so where
the difference is normalised next, such a constant computes the same limbs for every admissible operand and only the tracker's
precondition (b.tb <= S[8]) tells it apart; a constant two multiples smaller (fe_sub<3,29> for r0 under a Y1 in [4p, 5p)) goes
negative and is caught by the limbs."""
import os
import re
import subprocess

import numpy as np
import pytest

import ff29_model as m
import unit_ops_cases as uc
from halo2_experiments_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
BUILDS = ["plain", "hm_bounds"]
TABLES = ["fq", "fr", "curve"]


@pytest.fixture(scope="module")
def blocks():
    """{table name: [(table, op number, records)]} and the curve cases' expectations"""
    out = {f.name: [(f.index, uc.OPS[name], arr) for name, arr in uc.field_tables(f).items()] for f in m.FIELDS}
    out["curve"] = [(2, uc.OPS[name], arr) for name, (arr, _) in uc.curve_tables().items()]
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory, blocks):
    """{(build, table name): the runner's result blocks}: both builds compiled side by side, each run once over every table"""
    tmp = tmp_path_factory.mktemp("unit_ops")
    cmd = ["g++", "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", _lib.CSRC, os.path.join(HERE, "unit_ops_host.cpp")]
    exes = {b: str(tmp / f"unit_ops_{b}") for b in BUILDS}
    procs = [subprocess.Popen(cmd + (["-DHM_BOUNDS"] if b == "hm_bounds" else []) + ["-o", exes[b]]) for b in BUILDS]
    assert [p.wait() for p in procs] == [0, 0], "the runner does not compile"
    out = {}
    for t in TABLES:
        uc.write_blocks(str(tmp / f"{t}.cases"), blocks[t])
    for b in BUILDS:
        for t in TABLES:
            res = str(tmp / f"{t}.{b}.results")
            r = subprocess.run([exes[b], str(tmp / f"{t}.cases"), res], capture_output=True, text=True)
            out[b, t] = (r, uc.read_blocks(res, blocks[t]) if r.returncode == 0 else None)
    return out


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("build", BUILDS)
def test_every_op_matches_the_model(blocks, results, build, table):
    r, outs = results[build, table]
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # an HM_BOUNDS violation or a sanitizer report ends up here
    assert r.stderr == "", r.stderr[-3000:]
    names = {num: name for name, num in uc.OPS.items() if name.startswith("UC_" if table == "curve" else "UF_")}
    total = compared = 0
    if table == "curve":
        tables = uc.curve_tables()
        by_op = {names[op]: o for (_, op, _), o in zip(blocks[table], outs)}
        for (_, op, ins), o in zip(blocks[table], outs):
            compared += uc.check_curve(names[op], ins, tables[names[op]][1], o, by_op)
            total += ins.shape[0]
    else:
        field = m.FIELDS[TABLES.index(table)]
        for (_, op, ins), o in zip(blocks[table], outs):
            assert (o[:, 44] == int(build == "hm_bounds")).all()      # the tracked bounds of the results are there, and checked below
            compared += uc.check_field(field, names[op], ins, o)
            total += ins.shape[0]
    assert compared == total and total == sum(b[2].shape[0] for b in blocks[table]), "a generated case was not compared"
    print(f"{table} {build}: {total} cases over {len(outs)} ops")


@pytest.mark.parametrize("table", TABLES)
def test_bound_tracking_build_is_bit_identical(results, table):
    (ra, a), (rb, b) = results["plain", table], results["hm_bounds", table]
    assert ra.returncode == 0 and rb.returncode == 0
    words = uc.CURVE_OUT if table == "curve" else 28                  # beyond: the tracked bounds, which only one build writes
    assert all(np.array_equal(x[:, :words], y[:, :words]) for x, y in zip(a, b))


def test_exceptional_branches_are_covered():
    """see the module's docstring: asserted from the model alone"""
    cov = uc.branch_coverage(uc.curve_tables())
    assert cov["madd_hh"] == {1, 2}, cov
    # the square of k p is ceil(k^2 p / 2^261) p = p for k <= 13 (169 p < 2^261 < 170 p): r0 has k <= 9, g1_add_nz k <= 4, PP k <= 10
    assert cov["madd_rr0"] == {1} and cov["add_hh"] == {1} and cov["add_rr0"] == {1} and cov["xmadd_pp"] == {1}, cov
    kinds = {name: {mt.get("kind") for mt in meta} for name, (_, meta) in uc.curve_tables().items()}
    assert "top_limb" in kinds["UC_MADD_NZ"] and "top_limb" in kinds["UC_XMADD_FAST_LOCKSTEP"]
    assert {"generic", "equal"} <= kinds["UC_MADD_NZ"] and {"generic", "equal"} <= kinds["UC_ADD_NZ"]
    assert {"generic", "equal", "restart", "chain"} <= kinds["UC_XMADD"] and {"generic", "equal", "restart", "chain"} <= kinds["UC_MADD"]
    metas = uc.curve_tables()["UC_MADD_NZ"][1]
    assert any(mt["kind"] == "equal" and mt["exp"] is None for mt in metas) and any(mt["kind"] == "equal" and mt["exp"] is not None for mt in metas)


def test_the_table_has_every_subtraction_the_sources_instantiate():
    found = set()
    for name in sorted(os.listdir(_lib.CSRC)):
        if name.endswith((".h", ".hip", ".inc", ".cpp")) and name not in ("unit_ops.h", "devcheck.hip"):
            with open(os.path.join(_lib.CSRC, name)) as f:
                found |= {(int(k), int(b)) for k, b in re.findall(r"fe_sub\s*<\s*(\d+)\s*,\s*(\d+)\s*>", f.read())}
    assert found and found == set(uc.SUBS), (sorted(found), uc.SUBS)


def test_generated_constants_match_the_moduli():
    """csrc/bn256_constants.inc against the values the model derives from the oracle's P and R"""
    with open(os.path.join(_lib.CSRC, "bn256_constants.inc")) as f:
        c = m.parse_constants(f.read())
    for field, name in ((m.FQ, "FqParams"), (m.FR, "FrParams")):
        d = c[name]
        assert d["MOD"] == field.mod and d["INV29"] == field.inv29 and d["ONE"] == field.one
        assert d["EXT2INT"] == field.ext2int and d["INT2EXT"] == field.int2ext
        assert d["TOPMOD"] == field.topmod and d["QK"] == field.qk
        assert d["MOD32"] == [(field.p >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
