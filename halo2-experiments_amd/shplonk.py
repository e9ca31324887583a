"""The SHPLONK multiopen of ``halo2_proofs::poly::kzg::multiopen`` (``ProverSHPLONK`` / ``VerifierSHPLONK``; RECALLED from upstream
tag v2023_02_02, not pinned against its bytes): the rotation sets, the prover on the GPU and the verifier on host integers.

  - ``construct_intermediate_sets``: every commitment's set of points (ordered as integers, upstream's ``BTreeSet<F>``), the distinct
    sets in order of first appearance with their commitments in order of first appearance, and the super point set (RECALLED).
  - prover: y, v are squeezed; per set i the device adds v^i * (sum_j y^j P_ij - R_i) / Z_i to h through ONE call of
    ``hm_shplonk_set_quotient_bn256_fr_dev`` (csrc/shplonk.inc); h is committed, u squeezed; one more call with t = 1 divides
    sum_i v^i Z_{T \\ S_i}(u) sum_j y^j P_ij - Z_T(u) h by (X - u) and scales by 1 / Z_{T \\ S_0}(u), upstream's normalisation; the
    result is committed.  The constants R_i(u) of upstream's linearisation do not enter: kate_division drops a constant (RECALLED order of
    the transcript: y, v, [h], u, [h']).
  - verifier: the same sets from the claimed evaluations; L = [h'], R = sum_i v^i z_i (sum_j y^j C_ij - r_i G) - Z_T(u) / z_0' [h]
    + u [h'], with z_i normalised as upstream does, and the final check is e(L, [s]G2) = e(R, G2).

``set_quotient_ints`` is the integer twin of the kernel, stated the long way (interpolate, subtract, divide point by point);
``set_quotient_kate_ints`` is the identity the kernel computes by.  They play the role ``assign_ints`` plays for the witnesses."""
from __future__ import annotations

import ctypes
from typing import Hashable, List, Sequence, Tuple

from . import _lib
from ._marshal import _is_tensor, _ptr, _ptr_array, _stream_ptr, _tensor_rows
from .bn256 import FR_MODULUS, fr_array, fr_words, g1_ints
from .pairing import G1_GEN, g1_msm

R = FR_MODULUS
MAX_POINTS = _lib.HM_SHPLONK_MAX_POINTS
_LANES_MAX, _THREADS = 65536, 256


# ---- integers ---------------------------------------------------------------------------------------------------------------------------
def kate_ints(a: Sequence[int], z: int) -> List[int]:
    """``kate_division``: the quotient of a(X) - a(z) by X - z, len(a) - 1 coefficients"""
    q, acc = [0] * (len(a) - 1), 0
    for i in range(len(a) - 1, 0, -1):
        acc = (a[i] + z * acc) % R
        q[i - 1] = acc
    return q


def eval_ints(a: Sequence[int], x: int) -> int:
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % R
    return acc


def lagrange_interpolate_ints(points: Sequence[int], evals: Sequence[int]) -> List[int]:
    """the coefficients of the polynomial of degree < t through (points[l], evals[l])"""
    t = len(points)
    out = [0] * t
    for l in range(t):
        num, den = [1], 1
        for k in range(t):
            if k == l:
                continue
            num = [(a - points[k] * b) % R for a, b in zip([0] + num, num + [0])]
            den = den * (points[l] - points[k]) % R
        c = evals[l] * pow(den, -1, R) % R
        for i, a in enumerate(num):
            out[i] = (out[i] + c * a) % R
    return out


def vanishing_eval(points, x: int) -> int:
    acc = 1
    for p in points:
        acc = acc * (x - p) % R
    return acc


def _check_points(points) -> List[int]:
    pts = [int(p) % R for p in points]
    if not 1 <= len(pts) <= MAX_POINTS:
        raise ValueError(f"set quotient: need 1 <= t <= {MAX_POINTS} points")
    if len(set(pts)) != len(pts):
        raise ValueError("set quotient: two equal points")
    return pts


def _combine_ints(polys, weights, n):
    if not polys or len(polys) != len(weights):
        raise ValueError("set quotient: one weight per polynomial, at least one polynomial")
    return [sum(w * p[i] for w, p in zip(weights, polys)) % R for i in range(n)]


def set_quotient_ints(polys, weights, points, scale: int = 1) -> List[int]:
    """scale * (N - R) / Z_S for N = sum_j weights[j] polys[j], as n coefficients (the top t are zero): upstream's chain --
    interpolate R over the points from N's evaluations, subtract, divide by (X - p) point after point."""
    pts = _check_points(points)
    n = len(polys[0])
    if n < len(pts) + 1:
        raise ValueError("set quotient: need n >= t + 1")
    num = _combine_ints(polys, weights, n)
    r = lagrange_interpolate_ints(pts, [eval_ints(num, p) for p in pts])
    for i, c in enumerate(r):
        num[i] = (num[i] - c) % R
    for p in pts:
        assert eval_ints(num, p) == 0
        num = kate_ints(num, p)
    return [scale * c % R for c in num] + [0] * len(pts)


def set_quotient_coefficients(points, scale: int = 1) -> List[int]:
    """d_l = scale / prod_{l' != l} (p_l - p_l'): the partial fractions of scale / Z_S (csrc/shplonk.inc: shq_coefficients)"""
    pts = _check_points(points)
    out = []
    for l, p in enumerate(pts):
        den = 1
        for k, q in enumerate(pts):
            if k != l:
                den = den * (p - q) % R
        out.append(scale * pow(den, -1, R) % R)
    return out


def set_quotient_kate_ints(polys, weights, points, scale: int = 1) -> List[int]:
    """the same n coefficients by the identity the kernel uses: sum_l d_l * kate(N, p_l)"""
    n = len(polys[0])
    d = set_quotient_coefficients(points, scale)
    num = _combine_ints(polys, weights, n)
    qs = [kate_ints(num, int(p) % R) for p in points]
    return [sum(dl * q[i] for dl, q in zip(d, qs)) % R for i in range(n - 1)] + [0]


def set_quotient_plan(n: int) -> Tuple[int, int, int]:
    """(B, G, lanes) of the kernel's scans for n rows (csrc/shplonk.inc: shq_plan): a lane owns B consecutive rows, a workgroup 256
    lanes.  n <= 4 B is one lane; the last chunk is ragged when B does not divide n; n > 256 B needs a second workgroup."""
    b = -(-n // _LANES_MAX)
    if b < 4:
        b = 4 if n >= 4 else 1
    lanes = -(-n // b)
    return b, -(-lanes // _THREADS), lanes


# ---- the rotation sets ------------------------------------------------------------------------------------------------------------------
def construct_intermediate_sets(queries):
    """``queries``: (commitment key, point, eval) triples in the order the prover / verifier lists them.  Returns
    (rotation_sets, super_point_set): rotation_sets = [(points, [(key, evals)])] with the points of a set in ascending integer order,
    the evals of a commitment in its points' order, the sets and the commitments in order of first appearance; the super point set as
    an ascending list."""
    queries = [(key, int(pt) % R, ev) for key, pt, ev in queries]
    by_key: dict = {}
    evals: dict = {}
    for key, pt, ev in queries:
        by_key.setdefault(key, set()).add(pt)
        evals.setdefault((key, pt), ev)                # upstream's get_eval finds the first matching query
    sets: List[Tuple[tuple, list]] = []
    for key, pts in by_key.items():                    # dicts keep insertion order: first appearance
        pts_t = tuple(sorted(pts))
        for have, keys in sets:
            if have == pts_t:
                keys.append(key)
                break
        else:
            sets.append((pts_t, [key]))
    rotation_sets = [(list(pts), [(key, [evals[(key, p)] for p in pts]) for key in keys]) for pts, keys in sets]
    return rotation_sets, sorted({pt for _, pt, _ in queries})


# ---- the device entry -------------------------------------------------------------------------------------------------------------------
def set_quotient(polys, weights, points, scale: int = 1, out=None, accumulate: bool = False):
    """``out (+)= scale * (sum_j weights[j] polys[j] - R) / prod_l (X - points[l])`` on the device, one call of
    ``hm_shplonk_set_quotient_bn256_fr_dev``: ``polys`` a list of (n, 4) GPU tensors, ``weights`` / ``points`` / ``scale`` integers.
    Rows at and above n - t come out zero (left alone when accumulating).  Returns ``out`` (a new tensor when None)."""
    import torch

    polys = list(polys)
    if not polys:
        raise ValueError("set_quotient: no polynomial")
    if len(weights) != len(polys):
        raise ValueError("set_quotient: one weight per polynomial")
    pts = _check_points(points)
    n = _tensor_rows(polys[0], 4, "polys") if _is_tensor(polys[0]) else -1
    for p in polys:
        if not _is_tensor(p) or _tensor_rows(p, 4, "polys") != n:
            raise ValueError("set_quotient: polynomials must be GPU tensors of one length")
    if n < len(pts) + 1:
        raise ValueError("set_quotient: need n >= t + 1")
    if out is None:
        if accumulate:
            raise ValueError("set_quotient: nothing to accumulate into")
        out = torch.empty((n, 4), dtype=torch.int64, device=polys[0].device)
    elif not _is_tensor(out) or _tensor_rows(out, 4, "out") != n:
        raise ValueError("set_quotient: out differs in length")
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().hm_shplonk_set_quotient_bn256_fr_dev(_ptr_array(polys), _ptr(fr_array(weights)), len(polys), n, _ptr(fr_array(pts)), len(pts),
                                                                    _ptr(fr_words(int(scale) % R)), ctypes.c_void_p(out.data_ptr()),
                                                                    1 if accumulate else 0, ctypes.c_void_p(_stream_ptr(out))))
    return out


def set_quotient_batch(polys, weights, points, scales, outs=None, accumulate: bool = False):
    """``set_quotient`` for a batch of independent proofs in ONE launch chain (``hm_shplonk_set_quotient_batch_bn256_fr_dev``): per proof b
    ``polys[b]`` (the same count m for all; the same tensor may occur in several proofs), ``weights[b]``, ``points[b]`` (the same
    count t for all) and ``scales[b]``.  ``outs[b]`` may be one of proof b's own inputs, never another proof's input or output.
    Returns the list of outputs (new tensors when ``outs`` is None), word for word the loop of ``set_quotient``."""
    import torch

    polys = [list(p) for p in polys]
    proofs = len(polys)
    if proofs == 0:
        return []
    m = len(polys[0])
    if m == 0 or any(len(p) != m for p in polys):
        raise ValueError("set_quotient_batch: every proof needs the same number (>= 1) of polynomials")
    if len(weights) != proofs or any(len(w) != m for w in weights):
        raise ValueError("set_quotient_batch: one weight per polynomial")
    if len(points) != proofs or len(scales) != proofs:
        raise ValueError("set_quotient_batch: one point set and one scale per proof")
    pts = [_check_points(p) for p in points]
    t = len(pts[0])
    if any(len(p) != t for p in pts):
        raise ValueError("set_quotient_batch: every proof needs the same number of points")
    n = _tensor_rows(polys[0][0], 4, "polys") if _is_tensor(polys[0][0]) else -1
    for p in (q for row in polys for q in row):
        if not _is_tensor(p) or _tensor_rows(p, 4, "polys") != n:
            raise ValueError("set_quotient_batch: polynomials must be GPU tensors of one length")
    if n < t + 1:
        raise ValueError("set_quotient_batch: need n >= t + 1")
    if outs is None:
        if accumulate:
            raise ValueError("set_quotient_batch: nothing to accumulate into")
        outs = list(torch.empty((proofs, n, 4), dtype=torch.int64, device=polys[0][0].device))
    elif len(outs) != proofs or any(not _is_tensor(o) or _tensor_rows(o, 4, "outs") != n for o in outs):
        raise ValueError("set_quotient_batch: one output of the polynomials' length per proof")
    outs = list(outs)
    with torch.cuda.device(outs[0].device):
        _lib.check(_lib.load().hm_shplonk_set_quotient_batch_bn256_fr_dev(
            _ptr_array([p for row in polys for p in row]), _ptr(fr_array([[int(w) % R for w in row] for row in weights])), m, n,
            _ptr(fr_array(pts)), t, _ptr(fr_array([int(s) % R for s in scales])), _ptr_array(outs), 1 if accumulate else 0, proofs,
            ctypes.c_void_p(_stream_ptr(outs[0]))))
    return outs


# ---- prover and verifier ----------------------------------------------------------------------------------------------------------------
g1_words_to_int = g1_ints        # 12 (or 8) Montgomery words of a normalised G1 -> (x, y) integers, None for the identity


def _powers(base: int, count: int) -> List[int]:
    out, acc = [], 1
    for _ in range(count):
        out.append(acc)
        acc = acc * base % R
    return out


def create_opening(params, transcript, queries, polys: dict) -> None:
    """``ProverSHPLONK::create_proof``.  ``queries``: (key, point, eval) triples; ``polys[key]``: the (n, 4) coefficient tensor on the GPU
    that ``key`` commits.  Writes [h] and [h'] to ``transcript``."""
    y = transcript.squeeze_challenge()
    v = transcript.squeeze_challenge()
    rotation_sets, super_points = construct_intermediate_sets(queries)
    h = None
    for i, (pts, members) in enumerate(rotation_sets):
        cols = [polys[key] for key, _ in members]
        h = set_quotient(cols, _powers(y, len(cols)), pts, scale=pow(v, i, R), out=h, accumulate=i > 0)
    transcript.write_point(g1_words_to_int(params.commit(h)))
    u = transcript.squeeze_challenge()
    zt = vanishing_eval(super_points, u)
    cols, weights, z0 = [], [], None
    for i, (pts, members) in enumerate(rotation_sets):
        z_i = vanishing_eval([p for p in super_points if p not in pts], u)
        z0 = z_i if i == 0 else z0
        for j, (key, _) in enumerate(members):
            cols.append(polys[key])
            weights.append(pow(v, i, R) * z_i % R * pow(y, j, R) % R)
    final = set_quotient(cols + [h], weights + [-zt % R], [u], scale=pow(z0, -1, R))
    transcript.write_point(g1_words_to_int(params.commit(final)))


def create_openings(params, transcripts, queries_per_proof, polys_per_proof) -> None:
    """``create_opening`` for m independent proofs of one structure, every device step batched over the proofs: one
    ``set_quotient_batch`` per rotation set, one for the final division, and two ``best_multiexp_batch`` calls.  ``transcripts[b]``,
    ``queries_per_proof[b]`` and ``polys_per_proof[b]`` are what ``create_opening`` takes for proof b.  Every proof lists the same keys at
    the same rotations in the same order, so the rotation sets -- which keys, in what order, and which of a proof's queries gives
    each point -- are derived once, from proof 0; the points themselves differ per proof.  (A set's quotient and a vanishing product
    are symmetric in the points, so the integer order of proof 0's points serves every proof.)"""
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
    rotation_sets, super_points = construct_intermediate_sets(queries_per_proof[0])
    where = {}                                             # proof 0's point -> the first query that names it
    for i, (_, pt) in enumerate(q0):
        where.setdefault(pt, i)
    point = lambda b, pt0: int(queries_per_proof[b][where[pt0]][1]) % R
    sets = [([where[p] for p in pts], [key for key, _ in members]) for pts, members in rotation_sets]
    for b in range(m):
        if len({point(b, p) for p in super_points}) != len(super_points):
            raise ValueError(f"create_openings: proof {b}'s points do not have the structure of proof 0's")
    ys = [tr.squeeze_challenge() for tr in transcripts]
    vs = [tr.squeeze_challenge() for tr in transcripts]
    hs = None
    for i, (at, keys) in enumerate(sets):
        hs = set_quotient_batch([[polys_per_proof[b][key] for key in keys] for b in range(m)], [_powers(ys[b], len(keys)) for b in range(m)],
                                [[int(queries_per_proof[b][q][1]) % R for q in at] for b in range(m)], [pow(vs[b], i, R) for b in range(m)],
                                outs=hs, accumulate=i > 0)
    for tr, com in zip(transcripts, best_multiexp_batch(hs, params.g_handle)):
        tr.write_point(g1_words_to_int(com))
    us = [tr.squeeze_challenge() for tr in transcripts]
    cols, weights, scales = [], [], []
    for b in range(m):
        sp = [point(b, p) for p in super_points]
        zt = vanishing_eval(sp, us[b])
        cb, wb, z0 = [], [], None
        for i, (at, keys) in enumerate(sets):
            mine = {int(queries_per_proof[b][q][1]) % R for q in at}
            z_i = vanishing_eval([p for p in sp if p not in mine], us[b])
            z0 = z_i if i == 0 else z0
            for j, key in enumerate(keys):
                cb.append(polys_per_proof[b][key])
                wb.append(pow(vs[b], i, R) * z_i % R * pow(ys[b], j, R) % R)
        cols.append(cb + [hs[b]])
        weights.append(wb + [-zt % R])
        scales.append(pow(z0, -1, R))
    finals = set_quotient_batch(cols, weights, [[u] for u in us], scales)
    for tr, com in zip(transcripts, best_multiexp_batch(finals, params.g_handle)):
        tr.write_point(g1_words_to_int(com))


def verify_opening(transcript, queries, commitments: dict):
    """``VerifierSHPLONK::verify_proof`` up to the pairing: reads [h] and [h'] and returns the two G1 points (L, R) with
    e(L, [s]G2) = e(R, G2) for a valid opening -- equivalently s * L == R.  ``commitments[key]``: the (x, y) point of ``key``.  Host integers only."""
    y = transcript.squeeze_challenge()
    v = transcript.squeeze_challenge()
    h1 = transcript.read_point()
    u = transcript.squeeze_challenge()
    h2 = transcript.read_point()
    scalars, points = opening_terms(queries, commitments, y, v, u, h1, h2)
    return h2, g1_msm(scalars, points)


def opening_terms(queries, commitments: dict, y: int, v: int, u: int, h1, h2):
    """The scalars and the points whose sum is the R of ``verify_opening``, for the challenges y, v, u and the points [h] = ``h1``,
    [h'] = ``h2``: one term per commitment in the order of the rotation sets, then the generator, [h] and [h']."""
    rotation_sets, super_points = construct_intermediate_sets(queries)
    zt = vanishing_eval(super_points, u)
    scalars, points, r_outer, z0_inv = [], [], 0, None
    for i, (pts, members) in enumerate(rotation_sets):
        z_i = vanishing_eval([p for p in super_points if p not in pts], u)
        if i == 0:
            z0_inv, z_i = pow(z_i, -1, R), 1
        else:
            z_i = z_i * z0_inv % R
        outer = pow(v, i, R) * z_i % R
        for j, (key, evals) in enumerate(members):
            yj = pow(y, j, R)
            r_eval = eval_ints(lagrange_interpolate_ints(pts, evals), u)
            scalars.append(outer * yj % R)
            points.append(commitments[key])
            r_outer = (r_outer + outer * yj % R * r_eval) % R
    scalars += [-r_outer % R, -z0_inv * zt % R, u]
    points += [G1_GEN, h1, h2]
    return scalars, points
