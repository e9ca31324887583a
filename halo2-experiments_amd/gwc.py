"""The GWC multiopen of ``halo2_proofs::poly::kzg::multiopen`` (``ProverGWC`` / ``VerifierGWC``; RECALLED from upstream tag v2023_02_02,
not pinned against its bytes), the counterpart of ``shplonk``: the point groups, the prover on the GPU and the verifier on host
integers.  Everything below the multiopen -- commitments, transcripts, evaluations -- is shared with SHPLONK; the queries are the same
lists.

  - ``construct_point_groups``: the distinct points in order of first appearance, every group's queries in list order (upstream's
    ``construct_intermediate_sets`` of the gwc module).  A (key, point) pair named twice is refused, not deduplicated: the lists
    of ``prover`` / ``verifier`` hold none.
  - prover: v is squeezed; per group i the witness W_i = commit(kate_division(sum_j v^j p_ij, z_i)) is written -- the constant
    sum_j v^j e_ij drops out of the division.  One ``set_quotient`` with ONE point per group (``set_quotient_batch`` over the proofs in
    ``create_openings``), one ``best_multiexp_batch`` for all witnesses.  The prover squeezes no u.
  - verifier: v, the q points W_i, then u;  L = sum_i u^i W_i,  R = sum_i u^i z_i W_i + sum_i u^i sum_j v^j C_ij
    - (sum_i u^i sum_j v^j e_ij) G, and the final check is e(L, [s]G2) = e(R, G2): s L == R under the trapdoor.

``quotient_ints`` / ``create_opening_ints`` are the integer twins the tests use."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .bn256 import FR_MODULUS
from .pairing import G1_GEN, g1_msm
from .shplonk import _powers, g1_words_to_int, kate_ints, set_quotient, set_quotient_batch

R = FR_MODULUS


# ---- the point groups -------------------------------------------------------------------------------------------------------------------
def construct_point_groups(queries) -> List[Tuple[int, list]]:
    """``queries``: (commitment key, point, eval) triples in the order the prover / verifier lists them.  Returns [(point, [(key,
    eval)])]: the distinct points in order of first appearance, the members of a group in list order.  ValueError when a
    (key, point) pair stands twice."""
    groups: List[Tuple[int, list]] = []
    at: dict = {}
    seen = set()
    for key, pt, ev in queries:
        pt = int(pt) % R
        if (key, pt) in seen:
            raise ValueError(f"gwc: the query list names {key!r} twice at one point")
        seen.add((key, pt))
        if pt not in at:
            at[pt] = len(groups)
            groups.append((pt, []))
        groups[at[pt]][1].append((key, ev))
    return groups


# ---- integers ---------------------------------------------------------------------------------------------------------------------------
def quotient_ints(polys: Sequence[Sequence[int]], v: int, z: int) -> List[int]:
    """kate_division(sum_j v^j polys[j], z): the witness polynomial of one group, len - 1 coefficients"""
    n = len(polys[0])
    weights = _powers(v, len(polys))
    return kate_ints([sum(w * p[i] for w, p in zip(weights, polys)) % R for i in range(n)], z)


def create_opening_ints(queries, polys: dict, v: int) -> List[List[int]]:
    """the witness polynomials of ``create_opening`` for the challenge v, on integer coefficient lists ``polys[key]``"""
    return [quotient_ints([polys[key] for key, _ in members], v, z) for z, members in construct_point_groups(queries)]


# ---- prover -----------------------------------------------------------------------------------------------------------------------------
def create_opening(params, transcript, queries, polys: dict) -> None:
    """``ProverGWC::create_proof``.  ``queries``: (key, point, eval) triples; ``polys[key]``: the (n, 4) coefficient tensor on the GPU that
    ``key`` commits.  Writes W_0 .. W_{q-1} to ``transcript``."""
    from .arithmetic import best_multiexp_batch

    v = transcript.squeeze_challenge()
    witnesses = []
    for z, members in construct_point_groups(queries):
        cols = [polys[key] for key, _ in members]
        witnesses.append(set_quotient(cols, _powers(v, len(cols)), [z]))
    for com in best_multiexp_batch(witnesses, params.g_handle):
        transcript.write_point(g1_words_to_int(com))


def create_openings(params, transcripts, queries_per_proof, polys_per_proof) -> None:
    """``create_opening`` for m independent proofs of one structure, every device step one call over all proofs: one
    ``set_quotient_batch`` per point group and ONE ``best_multiexp_batch`` over the m q witnesses.  Every proof lists the same keys
    at the same rotations in the same order (the structural check of ``shplonk.create_openings``), so the groups -- which queries
    share a point -- are derived once, from proof 0; the points themselves differ per proof."""
    from .arithmetic import best_multiexp_batch

    m = len(transcripts)
    if m == 0:
        return
    if len(queries_per_proof) != m or len(polys_per_proof) != m:
        raise ValueError("create_openings: one query list and one polynomial table per transcript")
    q0 = [(key, int(pt) % R) for key, pt, _ in queries_per_proof[0]]
    for qs in queries_per_proof:
        if [key for key, _, _ in qs] != [key for key, _ in q0]:
            raise ValueError("create_openings: every proof must list the same keys in the same order")
    groups0 = construct_point_groups(queries_per_proof[0])
    where = {}                                             # proof 0's point -> the first query that names it
    for i, (_, pt) in enumerate(q0):
        where.setdefault(pt, i)
    group_of = [where[pt] for _, pt in q0]                 # per query: the first query of its group
    for b in range(m):
        pts = [int(pt) % R for _, pt, _ in queries_per_proof[b]]
        if len({pts[i] for i in where.values()}) != len(where) or any(pts[i] != pts[g] for i, g in enumerate(group_of)):
            raise ValueError(f"create_openings: proof {b}'s points do not have the structure of proof 0's")
    vs = [tr.squeeze_challenge() for tr in transcripts]
    per_group = []
    for z0, members in groups0:
        keys = [key for key, _ in members]
        per_group.append(set_quotient_batch([[polys_per_proof[b][key] for key in keys] for b in range(m)],
                                            [_powers(vs[b], len(keys)) for b in range(m)],
                                            [[int(queries_per_proof[b][where[z0]][1]) % R] for b in range(m)], [1] * m))
    coms = best_multiexp_batch([per_group[i][b] for b in range(m) for i in range(len(groups0))], params.g_handle)
    at = 0
    for tr in transcripts:
        for _ in groups0:
            tr.write_point(g1_words_to_int(coms[at]))
            at += 1


# ---- verifier ---------------------------------------------------------------------------------------------------------------------------
def verify_opening(transcript, queries, commitments: dict):
    """``VerifierGWC::verify_proof`` up to the pairing: squeezes v, reads W_0 .. W_{q-1}, squeezes u and returns the two G1 points
    (L, R) with e(L, [s]G2) = e(R, G2) for a valid opening -- equivalently s * L == R.  ``commitments[key]``: the (x, y) point of
    ``key``.  Host integers only."""
    v = transcript.squeeze_challenge()
    ws = [transcript.read_point() for _ in construct_point_groups(queries)]
    u = transcript.squeeze_challenge()
    scalars, points = opening_terms(queries, commitments, v, u, ws)
    return g1_msm(_powers(u, len(ws)), ws), g1_msm(scalars, points)


def opening_terms(queries, commitments: dict, v: int, u: int, ws):
    """The scalars and the points whose sum is the R of ``verify_opening``, for the challenges v, u and the witnesses ``ws``: one term
    per member in the order of the groups, then the generator, then W_0 .. W_{q-1} with u^i z_i.  (L is sum_i u^i W_i.)"""
    groups = construct_point_groups(queries)
    if len(ws) != len(groups):
        raise ValueError("gwc: one witness per point group")
    scalars, points, e_sum, u_i = [], [], 0, 1
    for z, members in groups:
        v_j = 1
        for key, ev in members:
            coeff = u_i * v_j % R
            scalars.append(coeff)
            points.append(commitments[key])
            e_sum = (e_sum + coeff * ev) % R
            v_j = v_j * v % R
        u_i = u_i * u % R
    scalars.append(-e_sum % R)
    points.append(G1_GEN)
    u_i = 1
    for (z, _), w in zip(groups, ws):
        scalars.append(u_i * z % R)
        points.append(w)
        u_i = u_i * u % R
    return scalars, points
