"""Records for the batch verifier's terms kernel (csrc/verify_terms.inc), shared by tests/test_verify_terms_fuzz.py (the two phases on the
host, under bound tracking) and tests/test_verify_terms_fuzz_gpu.py (the kernel).  No proof, key or SRS: a record is a set of challenges,
a weight r_b, the evaluations in the proof's order and the instance columns, all integers below r, and what the kernel must answer is
what ``batch_verifier.terms_from_challenges`` answers on the same integers:

    own = r_b * own[:-1],   shared = r_b * shared,   (h2_r, h2_l) = (r_b * u, r_b)        or, where the twin raises MalformedProof,
    d_bad = 1 and all-zero rows.

The numerator (the gate, permutation and lookup expressions folded in y) is not an output of the kernel.  It is checked through h(x) =
numerator / (x^n - 1), which the generator's scalar -- the last entry of ``shared`` -- sums with every other evaluation: a wrong
numerator moves that one word.

``cases(cs, k, inst_rows, seed)`` gives four classes, the class being the first letter of the label:

  A  random              everything uniform below r; never flagged
  B  edge values         the evaluations, the instance values, r_b and theta, beta, gamma, y, y', v drawn from EDGE about half of the
                         time and uniform otherwise; x and u uniform; one record of all-zero and one of all r - 1 evaluations; never
                         flagged
  C  degenerate, flagged x = 0, 1, -1, omega, omega^(n - blinding - 1), omega^(n - 1); u = x omega^rot for every rotation outside the
                         first rotation set -- each on a random and on an edge record
  D  degenerate, exact   u = x omega^rot for every rotation inside the first set (the vanishing value is 0: the scalar of [h] is 0),
                         u = 0, each of y, y', v, theta, beta, gamma at 0, r_b = 0 (zero rows and NO flag) and r_b = r - 1

This file imports no torch."""
import functools
import random
from types import SimpleNamespace

from halo2_experiments_amd import batch_verifier as bvm, circuits, poseidon as ps
from halo2_experiments_amd.bn256 import FR_MODULUS as R, FR_ROOT_OF_UNITY, FR_S

EDGE = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 2 ** 29 - 1, 2 ** 29, 2 ** 64 - 1, 2 ** 232, 2 ** 253, 2 ** 261 % R,
        pow(2, -261, R), pow(2, -256, R)]
SOFT = ("theta", "beta", "gamma", "y", "y2", "v")              # the challenges a record of class B draws from EDGE; x and u stay uniform

# id -> (constraint system, k, rows of every instance column).  k = 3 is the smallest k with n >= blinding + 3; at k = 6 poseidon's first
# rotation set has three points; merkle_sum_tree has lookups (theta is live) and at k = 28 takes 28 squarings to x^n with rotations
# near 2^28; overflow_check_v2(8, 4) has no instance query (the one-element instance array); rows 0, 1 and 64 = VT_MAX_INST_ROWS.
CONFIGS = {
    "poseidon_k3_rows1": (lambda: circuits.poseidon(ps.default_spec(5)), 3, 1),
    "poseidon_k6_rows0": (lambda: circuits.poseidon(ps.default_spec(5)), 6, 0),
    "poseidon_k6_rows64": (lambda: circuits.poseidon(ps.default_spec(5)), 6, 64),
    "merkle_v3_k8_rows5": (lambda: circuits.merkle_v3(ps.default_spec(3)), 8, 5),
    "merkle_sum_k9_rows0": (lambda: circuits.merkle_sum_tree(ps.default_spec(5)), 9, 0),
    "merkle_sum_k9_rows1": (lambda: circuits.merkle_sum_tree(ps.default_spec(5)), 9, 1),
    "merkle_sum_k28_rows64": (lambda: circuits.merkle_sum_tree(ps.default_spec(5)), 28, 64),
    "overflow_v2_k5_rows0": (lambda: circuits.overflow_check_v2(8, 4), 5, 0),
}


def omega_of(k: int) -> int:
    """the generator of the domain of 2^k rows (``EvaluationDomain.omega``, also at k = 28 where no extended domain exists)"""
    return pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R)


@functools.lru_cache(maxsize=None)
def setup(config: str) -> SimpleNamespace:
    make, k, rows = CONFIGS[config]
    cs = make()
    layout = bvm.ProofLayout(cs, k)
    omega = omega_of(k)
    plan = bvm.TermsPlan(layout, omega, [rows] * cs.num_instance)
    return SimpleNamespace(config=config, cs=cs, k=k, rows=rows, omega=omega, layout=layout, plan=plan)


def cases(cs, k, inst_rows, seed, total=150):
    """-> [(label, ch, r_b, evals, inst_cols)], ``total`` records: every record of classes C and D, the rest split between A and B.
    ``inst_rows``: the rows of every instance column."""
    layout = bvm.ProofLayout(cs, k)
    n, omega = layout.n, omega_of(k)
    rng = random.Random(seed)
    uniform = lambda: rng.randrange(R)
    edgy = lambda: rng.choice(EDGE) if rng.random() < 0.5 else uniform()

    def record(draw):
        ch = {name: draw() if name in SOFT else uniform() for name in bvm.RECORD}
        return ch, draw(), [draw() for _ in range(layout.n_scalars)], [[draw() for _ in range(inst_rows)] for _ in range(cs.num_instance)]

    def changed(base, **change):
        ch, rb, evals, inst = base
        rb = change.pop("rb", rb)
        if "u_rot" in change:
            change["u"] = dict(ch, **change)["x"] * pow(omega, change.pop("u_rot") % n, R) % R
        return dict(ch, **change), rb, evals, inst

    first, out_c, out_d = layout.sets[0][0], [], []
    outside = [rot for rot in layout.super_rotations if rot not in first]
    assert outside, "every registered circuit opens more than one rotation set"
    xs = [("x=0", 0), ("x=1", 1), ("x=-1", R - 1), ("x=omega", omega), ("x=omega^l_last", pow(omega, n - cs.blinding_factors - 1, R)),
          ("x=omega^(n-1)", pow(omega, n - 1, R))]
    for kind, draw in (("random", uniform), ("edge", edgy)):
        for name, x in xs:
            out_c.append((f"C:{name}:{kind}",) + changed(record(draw), x=x))
        for rot in outside:
            out_c.append((f"C:u=x*omega^{rot}:{kind}",) + changed(record(draw), u_rot=rot))
    for rot in first:
        out_d.append((f"D:u=x*omega^{rot}",) + changed(record(uniform), u_rot=rot))
    out_d.append(("D:u=0",) + changed(record(uniform), u=0))
    for name in SOFT:
        out_d.append((f"D:{name}=0",) + changed(record(uniform), **{name: 0}))
    out_d.append(("D:rb=0",) + changed(record(uniform), rb=0))
    out_d.append(("D:rb=r-1",) + changed(record(edgy), rb=R - 1))

    rest = total - len(out_c) - len(out_d)
    assert rest >= 4, "cases: total leaves no room for classes A and B"
    out_a = [(f"A:{i}",) + record(uniform) for i in range(rest // 2)]
    out_b = []
    for name, value in (("evals=0", 0), ("evals=r-1", R - 1)):
        ch, rb, evals, inst = record(edgy)
        out_b.append((f"B:{name}", ch, rb, [value] * len(evals), inst))
    out_b += [(f"B:{i}",) + record(edgy) for i in range(rest - len(out_a) - len(out_b))]
    return out_a + out_b + out_c + out_d


def expected(layout, omega, case):
    """-> (scalars, numerator): scalars = (own, shared, h2_r, h2_l) as the kernel must write them, or None where the twin raises
    ``MalformedProof``; numerator: the twin's, or None when it raised before it had one"""
    _, ch, rb, evals, inst_cols = case
    details = {}
    try:
        own, shared = bvm.terms_from_challenges(layout, omega, inst_cols, evals, ch, details)
    except bvm.MalformedProof:
        return None, details.get("numerator")
    return ([rb * c % R for c in own[:-1]], [rb * c % R for c in shared], rb * own[-1] % R, rb), details["numerator"]


@functools.lru_cache(maxsize=None)
def judged(config: str, seed: int, total: int):
    """the records of ``config`` with what the twin says of each, computed once per session: [(case, scalars or None, numerator)].
    Asserts what the classes promise: no record of class A, B or D is flagged, every record of class C is."""
    s = setup(config)
    out = []
    for case in cases(s.cs, s.k, s.rows, seed, total):
        scalars, numerator = expected(s.layout, s.omega, case)
        assert (scalars is None) == (case[0][0] == "C"), f"{config}: the twin and the class of {case[0]} disagree"
        out.append((case, scalars, numerator))
    return out
