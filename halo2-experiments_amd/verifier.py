"""``verify_proof`` of ``halo2_proofs::plonk`` over KZG with the SHPLONK multiopen, on host integers alone: it needs no GPU.  It shares
the transcript and the constraint system with ``prover`` and nothing else: the proof is read through ``Blake2bRead`` in the order the
prover wrote it (RECALLED from upstream, see ``prover``), the gate, permutation and lookup expressions are evaluated at x by a small
recursive evaluator over ``evaluation.Expression``, the quotient identity fixes h(x), and ``shplonk.verify_opening`` leaves two G1 points
L, R with e(L, [s]G2) = e(R, G2) -- checked by ``pairing.pairing_check`` against the parameters' G2 points, or, when the caller knows
the trapdoor s (tests), by s * L == R in G1.  ``verify_proof_multi`` reads a ``create_proof_multi`` proof of m circuits the same way
(per circuit where the prover writes per circuit), folds every circuit's expressions into one running value in y,
and makes one opening check; ``verify_proof`` is its m = 1 case.  ``multiopen="gwc"`` reads a proof that ends in the GWC multiopen
(``gwc.verify_opening``) in place of SHPLONK's; everything before the multiopen is the same.  ``lookup="logup"`` reads a proof whose
lookups are logUp arguments (this project's own format): per circuit and argument of ``cs.logup_arguments()``
the commitment of m where the permuted pair stands, that of phi where the lookup z stands, and the evaluations phi(x), phi(wx), m(x)
where the five stand; the identity takes ``evaluation.logup_expressions``.  One key pair serves both arguments."""
from __future__ import annotations

import hashlib
import struct

from . import evaluation as ev
from .domain import FR_MODULUS
from .keygen import FR_DELTA, VerifyingKey
from .kzg import g2_from_bytes
from .pairing import g1_add, g1_mul, g1_neg, g1_on_curve, pairing_check
from . import gwc
from .shplonk import g1_words_to_int, verify_opening
from .transcript import READERS, TranscriptError, check_encoding, check_lookup, check_multiopen

R = FR_MODULUS


def _vk_digest(vk: VerifyingKey) -> int:
    """``prover.vk_digest``, stated again: the verifier imports nothing from the prover"""
    cs = vk.cs
    hsh = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    hsh.update(struct.pack("<5I", vk.domain.k, cs.num_fixed, cs.num_advice, cs.num_instance, len(cs.equality)))
    for kind, index in cs.equality:
        hsh.update(kind.encode() + struct.pack("<I", index))
    for com in list(vk.fixed_commitments) + list(vk.permutation_commitments):
        p = g1_words_to_int(com)
        hsh.update(bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"))
    return int.from_bytes(hsh.digest(), "little") % R


def opening_points(cs, k: int = None, lookup: str = "halo2") -> int:
    """q, the distinct points the multiopen's queries name -- the witness points a "gwc" proof ends in: the distinct rotations of
    the advice and fixed queries, of the permutation and lookup arguments (0, 1, the last row; 0, -1, 1) and of h and the random
    polynomial (0).  Two rotations give one point exactly when they agree mod n = 2^k; without ``k`` they are compared as they are,
    which is the same count whenever every rotation lies within (-n / 2, n / 2).  ``lookup="logup"``: the arguments name 0 and 1."""
    adv_q, fix_q, _ = cs.queries()
    nsets, L = cs.permutation_sets(), len(cs.lookups)
    rots = [r for _, r in adv_q] + [r for _, r in fix_q] + [0]
    rots += ([0, 1] if nsets else []) + ([-(cs.blinding_factors + 1)] if nsets > 1 else [])
    rots += ([0, 1] if lookup == "logup" else [0, -1, 1]) if L else []
    return len({r % (1 << k) for r in rots} if k is not None else set(rots))


def proof_length(cs, circuits: int = 1, encoding: str = "halo2", multiopen: str = "shplonk", k: int = None, lookup: str = "halo2") -> int:
    """the bytes of a proof of ``circuits`` circuits of ``cs``, counted from the constraint system: 32 per point and per scalar, or
    with ``encoding="evm"`` 64 per point and 32 per scalar.  ``multiopen="gwc"``: the proof ends in ``opening_points(cs, k)`` points
    where a SHPLONK proof ends in two.  ``lookup="logup"``: per circuit and argument of ``cs.logup_arguments()`` two points (m, phi)
    and three scalars where a lookup has three and five."""
    check_encoding(encoding, "proof_length")
    check_multiopen(multiopen, "proof_length")
    check_lookup(lookup, "proof_length")
    adv_q, fix_q, _ = cs.queries()
    P, nsets, L = len(cs.equality), cs.permutation_sets(), len(cs.lookups)
    G = len(cs.logup_arguments()) if lookup == "logup" else 0
    lk_points, lk_scalars = (2 * G, 3 * G) if lookup == "logup" else (3 * L, 5 * L)
    points = circuits * (cs.num_advice + lk_points + nsets) + 1 + (cs.degree() - 1) + (opening_points(cs, k, lookup) if multiopen == "gwc" else 2)
    scalars = circuits * (len(adv_q) + (3 * nsets - 1 if nsets else 0) + lk_scalars) + len(fix_q) + 1 + P
    return 32 * ((2 if encoding == "evm" else 1) * points + scalars)


def evaluate_expression(e, leaf, scalars) -> int:
    """e at one point: ``leaf(kind, column, rotation)`` gives the columns' evaluations, ``scalars`` beta / gamma / theta"""
    if isinstance(e, ev.Constant):
        return e.value % R
    if isinstance(e, ev.Fixed):
        return leaf("fixed", e.column, e.rotation)
    if isinstance(e, ev.Advice):
        return leaf("advice", e.column, e.rotation)
    if isinstance(e, ev.Instance):
        return leaf("instance", e.column, e.rotation)
    if isinstance(e, ev.ProofScalar):
        return scalars[e.name]
    if isinstance(e, ev.Negated):
        return -evaluate_expression(e.a, leaf, scalars) % R
    if isinstance(e, ev.Sum):
        return (evaluate_expression(e.a, leaf, scalars) + evaluate_expression(e.b, leaf, scalars)) % R
    if isinstance(e, ev.Product):
        return evaluate_expression(e.a, leaf, scalars) * evaluate_expression(e.b, leaf, scalars) % R
    if isinstance(e, ev.Scaled):
        return evaluate_expression(e.a, leaf, scalars) * e.factor % R
    raise ValueError(f"verify_proof: no value for {type(e).__name__}")


def _instance_columns(cs, instance):
    single = len(instance) > 0 and isinstance(instance[0], int)
    cols = [list(instance)] if single else [list(c) for c in instance]
    if len(cols) != cs.num_instance:
        raise ValueError(f"instance: {cs.num_instance} column(s) expected")
    return [[int(v) % R for v in c] for c in cols]


def verify_proof(params, vk: VerifyingKey, instance, proof: bytes, trapdoor: int = None, encoding: str = "halo2",
                 multiopen: str = "shplonk", lookup: str = "halo2") -> bool:
    """True when ``proof`` is a valid proof of ``vk``'s circuit for ``instance`` (a list of integers for a one-column system, or one
    list per instance column).  ``params`` needs ``g2`` / ``s_g2`` only.  A malformed proof -- short or long, a point off the curve, a
    scalar not below r -- is False, not an exception.  ``encoding``: the proof's wire format, as ``create_proof`` names it; a proof
    in the other one is a malformed proof.  ``multiopen``: the scheme the proof ends in, as ``create_proof`` names it; a proof of the
    other scheme has another length, or fails.  ``lookup``: the lookup argument the proof carries, as ``create_proof`` names it; a
    proof of the other argument has another length, or fails."""
    check_encoding(encoding, "verify_proof")
    check_multiopen(multiopen, "verify_proof")
    check_lookup(lookup, "verify_proof")
    try:
        return _verify(params, vk, [instance], proof, trapdoor, encoding, multiopen, lookup)
    except TranscriptError:
        return False


def verify_proof_multi(params, vk: VerifyingKey, instances, proof: bytes, trapdoor: int = None, multiopen: str = "shplonk",
                       lookup: str = "halo2") -> bool:
    """True when ``proof`` is a valid ``create_proof_multi`` proof that every entry of ``instances`` -- one per circuit, each in the
    form ``verify_proof`` takes -- has a witness satisfying ``vk``'s circuit.  The proof is read in the prover's order (per circuit
    where the prover writes per circuit); the expression list is evaluated once per circuit, with that circuit's evaluations and
    instance values, into ONE running value folded in y; one opening, one pairing check.  Malformed: False, as in ``verify_proof``.
    ``multiopen``, ``lookup``: as in ``verify_proof``."""
    check_multiopen(multiopen, "verify_proof_multi")
    check_lookup(lookup, "verify_proof_multi")
    try:
        return _verify(params, vk, list(instances), proof, trapdoor, multiopen=multiopen, lookup=lookup)
    except TranscriptError:
        return False


def _verify(params, vk, instances, proof, trapdoor, encoding: str = "halo2", multiopen: str = "shplonk", lookup: str = "halo2") -> bool:
    cs, dom = vk.cs, vk.domain
    n, omega, blinding = 1 << dom.k, dom.omega, cs.blinding_factors
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    deg, last = cs.degree(), -(blinding + 1)
    m = len(instances)
    if m < 1 or len(proof) != proof_length(cs, m, encoding, multiopen, dom.k, lookup):
        return False
    logup = lookup == "logup"
    groups = cs.logup_arguments() if logup else []
    if logup:
        L = 0                                              # the lookups are read, evaluated and opened as their arguments
    G = len(groups)
    inst_cols = [_instance_columns(cs, instance) for instance in instances]
    M = range(m)
    t = READERS[encoding](proof)
    t.common_scalar(_vk_digest(vk))
    for c in M:
        for values in inst_cols[c]:
            for v in values:
                t.common_scalar(v)
    com = {}                                               # what belongs to circuit c: (kind, index, c)
    for c in M:
        for i in range(cs.num_advice):
            com[("advice", i, c)] = t.read_point()
    theta = t.squeeze_challenge()
    for c in M:
        for j in range(L):
            com[("lookup_a", j, c)] = t.read_point()
            com[("lookup_s", j, c)] = t.read_point()
        for g in range(G):
            com[("logup_m", g, c)] = t.read_point()
    beta = t.squeeze_challenge()
    gamma = t.squeeze_challenge()
    for c in M:
        for i in range(nsets):
            com[("perm_z", i, c)] = t.read_point()
    for c in M:
        for j in range(L):
            com[("lookup_z", j, c)] = t.read_point()
        for g in range(G):
            com[("logup_phi", g, c)] = t.read_point()
    com[("random",)] = t.read_point()
    y = t.squeeze_challenge()
    h_pieces = [t.read_point() for _ in range(deg - 1)]
    x = t.squeeze_challenge()
    rot = lambda r: x * pow(omega, r, R) % R

    adv_q, fix_q, inst_q = cs.queries()
    evals = {}
    for c in M:
        for i, r in adv_q:
            evals[(("advice", i, c), rot(r))] = t.read_scalar()
    for i, r in fix_q:
        evals[(("fixed", i), rot(r))] = t.read_scalar()
    evals[(("random",), x)] = t.read_scalar()
    for j in range(P):
        evals[(("sigma", j), x)] = t.read_scalar()
    for c in M:
        for i in range(nsets):
            for r in (0, 1) + ((last,) if i + 1 < nsets else ()):
                evals[(("perm_z", i, c), rot(r))] = t.read_scalar()
    for c in M:
        for j in range(L):
            for kd, r in (("lookup_z", 0), ("lookup_z", 1), ("lookup_a", 0), ("lookup_a", -1), ("lookup_s", 0)):
                evals[((kd, j, c), rot(r))] = t.read_scalar()
        for g in range(G):
            for kd, r in (("logup_phi", 0), ("logup_phi", 1), ("logup_m", 0)):
                evals[((kd, g, c), rot(r))] = t.read_scalar()

    # ---- the Lagrange values the arguments and the instance columns need ---------------------------------------------------------------------
    xn = pow(x, n, R)
    n_inv = pow(n, -1, R)

    def lagrange_at(i: int, point: int) -> int:          # l_i(point) = omega^i (point^n - 1) / (n (point - omega^i))
        w = pow(omega, i, R)
        if point == w:
            return 1
        return w * (pow(point, n, R) - 1) % R * n_inv % R * pow(point - w, -1, R) % R

    l0 = lagrange_at(0, x)
    l_last = lagrange_at(n - blinding - 1, x)
    l_blind = sum(lagrange_at(i, x) for i in range(n - blinding, n)) % R
    l_active = (1 - l_last - l_blind) % R

    def instance_eval(circuit: int, column: int, r: int) -> int:
        pt = rot(r)
        return sum(v * lagrange_at(i, pt) for i, v in enumerate(inst_cols[circuit][column]) if v) % R

    # ---- h(x) from the identity: the expressions in the prover's order, folded in y ---------------------------------------------------------------
    nf = cs.num_fixed
    sigma0, z0 = nf, nf + P
    i_l0, i_last, i_active, i_x, lookup0 = z0 + nsets, z0 + nsets + 1, z0 + nsets + 2, z0 + nsets + 3, z0 + nsets + 4
    special = {i_l0: l0, i_last: l_last, i_active: l_active, i_x: x}

    def leaf_of(c: int):
        def leaf(kind: str, column: int, r: int) -> int:
            if kind == "instance":
                return instance_eval(c, column, r)
            if kind == "advice":
                return evals[(("advice", column, c), rot(r))]
            if column < nf:
                return evals[(("fixed", column), rot(r))]
            if column in special:
                return special[column]
            if column < z0:
                return evals[(("sigma", column - sigma0), rot(r))]
            if column < i_l0:
                return evals[(("perm_z", column - z0, c), rot(r))]
            if logup:
                g, part = divmod(column - lookup0, 2)
                return evals[((("logup_phi", "logup_m")[part], g, c), rot(r))]
            j, part = divmod(column - lookup0, 3)
            return evals[((("lookup_z", "lookup_a", "lookup_s")[part], j, c), rot(r))]
        return leaf

    F = ev.Fixed
    kind = {"advice": ev.Advice, "fixed": ev.Fixed, "instance": ev.Instance}
    exprs = list(cs.polynomials())
    exprs += ev.permutation_expressions([kind[kd](i) for kd, i in cs.equality], [F(sigma0 + j) for j in range(P)],
                                        [lambda r, i=i: F(z0 + i, r) for i in range(nsets)], F(i_l0), F(i_last), F(i_active), F(i_x), chunk,
                                        FR_DELTA, last)
    for g, (tabs, ins_list) in enumerate(groups):
        b = lookup0 + 2 * g
        exprs += ev.logup_expressions(ins_list, tabs, lambda r, b=b: F(b, r), lambda r, b=b: F(b + 1, r), F(i_l0), F(i_last), F(i_active))
    for j, (ins, tabs) in enumerate([] if logup else cs.lookups):
        b = lookup0 + 3 * j
        exprs += ev.lookup_expressions(ins, tabs, lambda r, b=b: F(b, r), lambda r, b=b: F(b + 1, r), lambda r, b=b: F(b + 2, r), F(i_l0),
                                       F(i_last), F(i_active))
    scalars = {"Beta": beta, "Gamma": gamma, "Theta": theta}
    acc = 0
    for c in M:                                            # circuit 0's gates, permutation and lookup terms, then circuit 1's ...
        leaf = leaf_of(c)
        for e in exprs:
            acc = (acc * y + evaluate_expression(e, leaf, scalars)) % R
    if xn == 1:
        return False
    hx = acc * pow(xn - 1, -1, R) % R
    h_com = None
    for piece in reversed(h_pieces):                       # sum_i x^(n i) [h_i]
        h_com = g1_add(g1_mul(xn, h_com) if h_com is not None else None, piece)
    com[("h",)] = h_com
    for c, point in enumerate(vk.fixed_commitments):
        com[("fixed", c)] = g1_words_to_int(point)
    for j, point in enumerate(vk.permutation_commitments):
        com[("sigma", j)] = g1_words_to_int(point)

    # ---- the multiopen --------------------------------------------------------------------------------------------------------------------------------
    q = lambda key, pt: (key, pt, evals[(key, pt)])
    queries = []
    for c in M:
        queries += [q(("advice", i, c), rot(r)) for i, r in adv_q]
        queries += [qq for i in range(nsets) for qq in (q(("perm_z", i, c), x), q(("perm_z", i, c), rot(1)))]
        queries += [q(("perm_z", i, c), rot(last)) for i in reversed(range(nsets - 1))]
        for j in range(L):
            queries += [q(("lookup_z", j, c), x), q(("lookup_a", j, c), x), q(("lookup_s", j, c), x), q(("lookup_a", j, c), rot(-1)),
                        q(("lookup_z", j, c), rot(1))]
        for g in range(G):
            queries += [q(("logup_phi", g, c), x), q(("logup_m", g, c), x), q(("logup_phi", g, c), rot(1))]
    queries += [q(("fixed", i), rot(r)) for i, r in fix_q] + [q(("sigma", j), x) for j in range(P)]
    queries += [(("h",), x, hx), q(("random",), x)]
    if any(com[key] is None for key, _, _ in queries):
        return False                                         # the identity cannot be absorbed or opened
    left, right = (gwc.verify_opening if multiopen == "gwc" else verify_opening)(t, queries, com)
    if t.remaining():
        return False
    if trapdoor is not None:
        return g1_mul(trapdoor, left) == right
    g2, s_g2 = g2_from_bytes(params.g2), g2_from_bytes(params.s_g2)
    return g1_on_curve(left) and pairing_check([(left, s_g2), (g1_neg(right), g2)])
