"""The host side of the ledger's id proof (tests/test_ledger_distinct_gpu.py has the proofs): ``verify_ledger_user`` with ``rows`` on a
ledger made on host integers through the trapdoor, the key checks of ``prove_ledger`` / ``verify_ledger`` that need no device, and
the new fields' defaults."""
import pytest

from halo2_experiments_amd import circuits, ledger as lg

import ledger_cases as lc


@pytest.fixture(scope="module")
def ledger():
    return lc.int_ledger(4, 2, seed=3)                           # 10 live rows of 16


def test_a_row_behind_the_live_rows_is_refused_only_when_rows_is_given(ledger):
    c = ledger
    public, rows = (c["c_id"], c["cs"]), c["n"] - 6
    user = lambda i, **kw: lg.verify_ledger_user(c["params"], public, i, c["ids"][i], [col[i] for col in c["bal"]], c["openings"][i], **kw)
    assert user(0) and user(rows - 1) and user(rows) and user(c["n"] - 1)              # the zero rows open to zero: valid openings
    assert user(0, rows=rows) and user(rows - 1, rows=rows)
    assert not user(rows, rows=rows) and not user(c["n"] - 1, rows=rows)
    assert not user(0, rows=0) and user(rows, rows=rows + 1)
    with pytest.raises(ValueError, match="outside the domain"):
        lg.verify_ledger_user(c["params"], public, c["n"], 0, [0, 0], None, rows=rows)


def test_the_two_kinds_of_key_are_told_apart():
    sorted_cs, range_cs = circuits.sorted_column(4, 4), circuits.overflow_check_v2(4, 4, unblinded_value=True)
    assert lg._sorted_parameters(sorted_cs, "t") == (4, 4) and lg._sorted_parameters(circuits.sorted_column(16, 8), "t") == (16, 8)
    for cs in (range_cs, circuits.overflow_check_v2(4, 4), circuits.poseidon()):
        with pytest.raises(ValueError, match="sorted_column"):
            lg._sorted_parameters(cs, "t")


def test_the_new_fields_default_to_none():
    proof = lg.LedgerProof(None, [None], [b""], 0, [0], None)
    assert proof.id_proof is None and proof.rows is None and proof.columns is None
    assert lg.ARGSORT_TILE == 1024
