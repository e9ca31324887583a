"""CPU suite: the lowering of evaluate_h programs (csrc/graph_lower.h: copy propagation, register forwarding and store elision,
the static value-bound analysis, slot allocation) on programs that ``GraphEvaluator.add_expression`` never emits.

``hc_graph_replay`` (csrc/host_check.cpp, the HM_BOUNDS build) lowers a program with the code ``hm_graph_create`` runs and
interprets the LOWERED program with the primitives of the kernel, with worst-case bound tracking.  For the hand-written programs
of tests/graph_programs.py and a seeded sweep of random ones, in both column formats:

  * the values equal oracle/graph_ref word for word;
  * for every lowered calculation the tracked bound is at most the lowering's static bound, and the static bound of what is
    stored or forwarded is at most GE_CAP; no precondition of a primitive is violated (the library aborts when one is);
  * over the committed seeds every decision the lowering can take occurs (graph_programs.REQUIRED_FACTS) and every shape the
    generator promises is produced (graph_programs.SHAPES).

The replays run in a child process: an HM_BOUNDS violation aborts the process, and the test reports the program instead."""
import ctypes
import itertools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import graph_programs as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_SEEDS = range(7000, 7320)                  # 320 random programs of 5 .. 120 calculations
HAND_SIZES = [(1, 1), (2, 8), (64, 2)]           # (rows of a segment, segments)
COMBOS = list(itertools.product(gp.SEGMENT_ROWS, gp.SEGMENT_COUNTS))
MAX_CALC_ROWS = 12000                            # the oracle is Python: rows x calculations of one program stays under this


def sweep_size(seed: int, n_calcs: int):
    """Every (segment, segments) combination in turn; a program too long for its turn takes the largest size it can afford."""
    seg, segments = COMBOS[seed % len(COMBOS)]
    if seg * segments * n_calcs > MAX_CALC_ROWS:
        seg, segments = max((c for c in COMBOS if c[0] * c[1] * n_calcs <= MAX_CALC_ROWS), key=lambda c: (c[0] * c[1], c[1]))
    return seg, segments


def run_one(hc, p, seg, segments, data_seed, emit):
    """One program at one size, both column formats -> (failures, facts, facts of the internal format alone)."""
    d = gp.make_data(random.Random(data_seed), seg, segments)
    exp = gp.oracle_values(p, d)
    bad, facts, internal_facts = [], set(), set()
    for internal in (False, True):
        what = f"{p.name} seg={seg} segments={segments} data_seed={data_seed} {'internal' if internal else 'external'}"
        emit("BEGIN " + what)
        r = gp.host_replay(hc, p, d, internal)
        bad += gp.check_replay(p, r, exp, what)
        if r.rc == 0:
            facts |= gp.lowering_facts(r)
            if internal:
                internal_facts |= gp.lowering_facts(r)
    if bad:
        bad.append(p.describe())
    return bad, facts, internal_facts


def child_main(mode: str) -> None:
    emit = lambda s: print(s, flush=True)
    hc = gp.hostcheck()
    failures, facts, internal_facts, shapes, sizes = {}, set(), set(), set(), set()
    if mode == "hand":
        for p in gp.hand_written():
            shapes |= gp.shapes(p)
            for i, (seg, segments) in enumerate(HAND_SIZES):
                bad, f, fi = run_one(hc, p, seg, segments, 100 + i, emit)
                facts |= f
                internal_facts |= fi
                if bad:
                    failures.setdefault(p.name, []).extend(bad)
    else:
        for seed in SWEEP_SEEDS:
            p = gp.random_program(seed)
            shapes |= gp.shapes(p)
            seg, segments = sweep_size(seed, len(p.lower()["calcs"]))
            sizes.add((seg, segments))
            bad, f, fi = run_one(hc, p, seg, segments, seed, emit)
            facts |= f
            internal_facts |= fi
            if bad:
                failures[p.name] = bad
    emit("RESULT " + json.dumps(dict(failures=failures, facts=sorted(facts), internal_facts=sorted(internal_facts), shapes=sorted(shapes),
                                     sizes=sorted(sizes))))


def run_child(mode: str) -> dict:
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_graph_lowering_host as t; t.child_main({mode!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    lines = r.stdout.splitlines()
    begun = [ln[6:] for ln in lines if ln.startswith("BEGIN ")]
    result = next((json.loads(ln[7:]) for ln in lines if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or result is None:
        return dict(aborted=begun[-1] if begun else "(before the first program)", returncode=r.returncode, stderr=r.stderr[-2000:], begun=begun)
    return result


@pytest.fixture(scope="module")
def hand():
    return run_child("hand")


@pytest.fixture(scope="module")
def sweep():
    return run_child("sweep")


def _no_abort(res):
    assert "aborted" not in res, f"the replay process ended with {res['returncode']} in: {res['aborted']}\n{res['stderr']}"


@pytest.mark.parametrize("name", [p.name for p in gp.hand_written()])
def test_hand_written_program(hand, name):
    """Exactness and bounds for one named program, at 1 x 1, 2 x 8 and 64 x 2 rows, both column formats."""
    if "aborted" in hand and hand["aborted"].split(" ")[0] != name and any(b.split(" ")[0] == name for b in hand["begun"]):
        return                                                       # finished before another program aborted the process
    _no_abort(hand)
    assert not hand["failures"].get(name), "\n".join(hand["failures"][name])


def test_hand_written_programs_cover_every_rule(hand):
    """The hand-written list alone reaches every decision of the lowering and every shape of the generator's list."""
    _no_abort(hand)
    assert not set(gp.REQUIRED_FACTS) - set(hand["facts"]), sorted(set(gp.REQUIRED_FACTS) - set(hand["facts"]))
    assert "copy_propagated:column" in hand["internal_facts"]
    assert not set(gp.SHAPES) - set(hand["shapes"]), sorted(set(gp.SHAPES) - set(hand["shapes"]))


def test_random_sweep_exactness_and_bounds(sweep):
    """>= 300 seeded random programs: values == oracle, tracked <= static <= GE_CAP, no abort; both column formats."""
    _no_abort(sweep)
    assert len(SWEEP_SEEDS) >= 300
    assert not sweep["failures"], "\n".join(f"{k}:\n  " + "\n  ".join(v) for k, v in list(sweep["failures"].items())[:5])


def test_random_sweep_coverage(sweep):
    """Coverage as a condition: the committed seeds reach every operation, every flag set and clear, both kinds of removed
    Store, both result forms, a recycled slot, every shape of the generator's list and every size."""
    _no_abort(sweep)
    assert not set(gp.REQUIRED_FACTS) - set(sweep["facts"]), sorted(set(gp.REQUIRED_FACTS) - set(sweep["facts"]))
    assert "copy_propagated:column" in sweep["internal_facts"]
    assert not set(gp.SHAPES) - set(sweep["shapes"]), sorted(set(gp.SHAPES) - set(sweep["shapes"]))
    assert {tuple(s) for s in sweep["sizes"]} == set(COMBOS)


def test_random_programs_are_reproducible():
    """The same seed gives the same program and the same inputs in every process (no hash() of a string anywhere)."""
    a, b = gp.random_program(7001), gp.random_program(7001)
    assert a.g.calculations == b.g.calculations and np.array_equal(a.lower()["calcs"], b.lower()["calcs"])
    assert gp.make_data(random.Random(5), 2, 2) == gp.make_data(random.Random(5), 2, 2)
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import graph_programs as gp; print(gp.random_program(7001).describe())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True, env=dict(os.environ, PYTHONHASHSEED="12345"))
    assert out.stdout.strip() == a.describe()


def test_replay_refuses_what_graph_create_refuses():
    """graph_validate (csrc/graph_lower.h) is the validation of hm_graph_create: every promise, without a GPU."""
    hc = gp.hostcheck()
    col = lambda c, rot=0, lg=0: (2 << 30) | (rot << 20) | (lg << 14) | c
    inter = lambda i: (1 << 30) | i

    def refused(calcs, n_const=1, n_dyn=0, n_rot=1, n_cols=1, n_inter=4):
        cols = [np.zeros((4, 4), dtype=np.uint64) for _ in range(n_cols)]
        r = gp.host_replay_raw(hc, np.array(calcs, dtype=np.uint32), [0] * n_const, n_dyn, [0] * n_rot, n_cols, n_inter, cols,
                               np.zeros((max(n_dyn, 1), 4), dtype=np.uint64), 2, 1, False, np.zeros((4, 4), dtype=np.uint64))
        return r.error if r.rc == -1 else None

    ok = [[0, col(0), 0, 0, 0], [2, inter(0), inter(0), 0, 1]]
    assert refused(ok) is None
    assert "target out of range" in refused([[0, col(0), 0, 0, 4]])
    assert "written twice" in refused([[0, col(0), 0, 0, 1], [0, col(0), 0, 0, 1]])
    assert "read before" in refused([[2, inter(1), 0, 0, 0]])
    assert "unknown operation" in refused([[8, 0, 0, 0, 0]])
    assert "source out of range" in refused([[6, col(1), 0, 0, 0]])                    # column
    assert "source out of range" in refused([[6, col(0, rot=1), 0, 0, 0]])             # rotation
    assert "source out of range" in refused([[6, 1, 0, 0, 0]])                         # constant
    assert "source out of range" in refused([[6, inter(4), 0, 0, 0]])                  # intermediate index
    assert "source out of range" in refused([[6, col(0, lg=31), 0, 0, 0]])             # a short column of more than 2^30 rows
    assert refused([[6, 1, 0, 0, 0]], n_dyn=1) is None                                 # ... constant 1 exists once there is a per-call one
    assert "16 per-call" in refused(ok, n_dyn=17)
    assert refused(ok) is None


def test_one_row_column_is_encoded_as_two_rows():
    """The instruction's log2(rows) field reads 0 as "full size": a period-1 column must not be lowered to that."""
    from halo2_experiments_amd import evaluation as ev
    g = ev.GraphEvaluator()
    g.add_custom_gates([ev.Fixed(0, 1) * ev.Advice(0)])
    low = g.lower(1, 1, 0, short_columns={0: 0})
    fixed_reads = [w for w in low["calcs"][:, 1:4].ravel().tolist() if (w >> 30) == 2 and (w & 0x3FFF) == 0]
    assert fixed_reads and all((w >> 14) & 63 == 1 for w in fixed_reads)
    assert low["short_columns"] == {0: 0}


if __name__ == "__main__":
    child_main(sys.argv[1])
