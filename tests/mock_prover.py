"""The tests' own MockProver: given a constraint system and ALL columns as Python integers, it evaluates every gate polynomial
on every usable row with the oracle's expression evaluator, compares the two cells of every copy, and looks every lookup input
up in its table column.  It shares nothing with synthesis.assign_ints or the witness kernel: the gates come from circuits.py, the
evaluator from oracle/graph_ref.py, and what it is given is data."""
from oracle import graph_ref

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def lookup_tables(cs, fixed, advice, instance, n, usable_rows):
    """the table of every lookup: the set of its table expressions' values on the usable rows"""
    return [{tuple(graph_ref.evaluate_expression(t, fixed, advice, instance, [], row, 1, n) for t in tabs) for row in range(usable_rows)}
            for _, tabs in cs.lookups]


def verify(cs, fixed, advice, instance, copies, n, usable_rows, rows=None, tables=None):
    """-> list of failures: ("gate", name, poly index, row) / ("copy", cell_a, cell_b) / ("lookup", lookup index, row).
    usable_rows: n - (blinding_factors + 1); rows: restrict the gate and lookup checks to these rows (default: every usable row);
    tables: what ``lookup_tables`` gave for these columns, for a caller that checks many witnesses against tables that do not change
    (tables over fixed columns); default: every table is built here, from the columns given."""
    failures = []
    cols = {"fixed": fixed, "advice": advice, "instance": instance}
    rows = range(usable_rows) if rows is None else [r for r in rows if r < usable_rows]
    for name, polys in cs.gates:
        for pi, p in enumerate(polys):
            for row in rows:
                if graph_ref.evaluate_expression(p, fixed, advice, instance, [], row, 1, n) % R:
                    failures.append(("gate", name, pi, row))
    for a, b in copies:
        if cols[a[0]][a[1]][a[2]] % R != cols[b[0]][b[1]][b[2]] % R:
            failures.append(("copy", a, b))
    for li, (ins, tabs) in enumerate(cs.lookups):
        table = tables[li] if tables is not None else \
            {tuple(graph_ref.evaluate_expression(t, fixed, advice, instance, [], row, 1, n) for t in tabs) for row in range(usable_rows)}
        for row in rows:
            if tuple(graph_ref.evaluate_expression(e, fixed, advice, instance, [], row, 1, n) for e in ins) not in table:
                failures.append(("lookup", li, row))
    return failures


def gate_names(failures):
    return sorted({f[1] for f in failures if f[0] == "gate"})
