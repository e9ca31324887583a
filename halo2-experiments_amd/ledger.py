"""A ledger over KZG: "every balance is in range, the columns sum to the published totals, and row i is MINE" -- one opening per user,
whatever the number of assets, and many users checked on the GPU with a verdict each.

What ``solvency.py`` leaves open is closed by one more column and two challenges.  Columns are padded with zeros to n = 2^k rows:

    f_id            the id column: field elements the operator chooses, pairwise distinct
    f_0 .. f_{P-1}  the balance columns
    C_p             the first commitment of asset p's range proof (``overflow_check_v2(..., unblinded_value=True)``, as in solvency.py)
    C_id            params.commit_lagrange(f_id)
    gamma           Blake2b-512, person b"halo2amd-ledger\\0" (16 bytes), of  k (u32 LE) | P (u32 LE) | C_id | C_0 | .. | C_{P-1},
                    every point as 64 bytes (x then y, canonical integers little-endian; the identity as 64 zero bytes), the digest
                    read little-endian and reduced mod r: drawn after every commitment is fixed, recomputed by every verifier
    g               f_id + sum_p gamma^(p+1) f_p,          C_gamma = C_id + sum_p gamma^(p+1) C_p   (host integers, P + 1 products)
    eta             Blake2b-512, person b"halo2amd-totals\\0", of gamma's message | S_id | T_0 | .. | T_{P-1}, the published column sums
                    as 32 little-endian bytes each, reduced mod r: drawn after the commitments AND the claimed sums are fixed

User i holds pi_i = [(g(s) - g(omega^i)) / (s - omega^i)]G and checks e(pi_i, [s]G2) = e(C_gamma - [y_i]G + [omega^i]pi_i, G2) with
y_i = id_i + sum_p gamma^(p+1) b_{p,i}: by Schwartz-Zippel over gamma a wrong id, or a wrong balance of any asset, passes with
probability <= (P + 1) / r.  The totals take ONE opening at 0, of C_eta = C_id + sum_p eta^(p+1) C_p, whose value is
(S_id + sum_p eta^(p+1) T_p) / n for the published column sums.  It is NOT an opening of C_gamma: gamma is known to the prover before
it publishes the sums, so one linear equation in gamma could be met by understating T_0 by d and raising the unverifiable S_id by
gamma d; eta depends on the sums themselves, so wrong sums survive with probability <= P / r.  (A deviation from the first
statement of this feature, which hashed the commitments only and opened C_gamma at 0.)  The 6 rows no gate reaches are pinned as in solvency.py: their combined openings (rows n - 6 .. n - 1 of
``ledger_openings``) are checked with all values zero, and a combined value of zero at a gamma drawn after the commitments pins
every column to zero there.

That the ids are pairwise distinct -- so that no row, id included, can be handed to two users and carry their liability once -- is
proved under a second key, and only under it: ``prove_ledger(..., id_pk=)`` adds ``id_proof``, a proof of ``circuits.sorted_column``
whose first commitment is C_id itself (the id column is unblinded there), and ``verify_ledger(..., id_vk=)`` checks it and that
commitment.  The circuit wants the rows in ascending id order with neighbours less than 2^(max_bits * acc_cols) apart, and then
max_bits * acc_cols + k <= 253 makes any two ids differ (``circuits.sorted_column`` has the argument); ``ledger_order`` gives the
permutation that brings a ledger into that order.  The selector reaches rows 0 .. rows - 2, so the statement is about the ``rows`` live
rows: pass ``rows`` to ``verify_ledger_user`` / ``verify_ledger_users`` as well, which then refuse an index at or behind it.  Without
the second key nothing of this is proved, as before: a duplicate id is then caught by the two users comparing their rows, not by a
circuit, and the module checks nothing about ids beyond their canonical form.  Commitments are deterministic (nothing is hidden), as in
solvency.py.  ``verify_ledger_user`` on host integers is the oracle; ``verify_ledger_users`` builds every user's pairing operands in
one kernel (csrc/ledger.inc: one lane per user) and checks them with one ``device_pairing.run_device`` call."""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, device_pairing
from ._marshal import _dev_ptr, _is_tensor, _ptr, _stream_ptr, _u32p
from .arithmetic import linear_combination
from .bn256 import FR_MODULUS, fq_array, fr_array, fr_ints, fr_words, g1_ints, g1_words
from .domain import EvaluationDomain
from .keygen import ProvingKey, VerifyingKey
from .kzg import g2_from_bytes
from .openings import _point, _scalar_int, domain_omega, open_all, open_at, verify_opening
from .pairing import g1_add, g1_mul, g1_on_curve
from .prover import create_proofs
from .solvency import _range_parameters
from .synthesis import BLINDING_ROWS, range_witness, sorted_witness
from .transcript import TranscriptError, check_encoding, check_lookup, check_multiopen, g1_decompress_int, g1_uncompressed_int
from .verifier import verify_proof

R = FR_MODULUS
PERSON = b"halo2amd-ledger\0"
TOTALS_PERSON = b"halo2amd-totals\0"
_vp = ctypes.c_void_p


@dataclass
class LedgerProof:
    """Published: ``id_commitment`` and ``commitments[p]`` ((x, y) integers, None for a zero column), ``range_proofs[p]`` the bytes
    of asset p's range proof, ``id_total`` and ``totals[p]`` the column sums as integers, ``zero_opening`` the opening of C_eta at 0
    (8 affine words).  The prover's own: ``columns``, the padded id and balance columns, a (P + 1, n, 4) GPU tensor from which
    ``ledger_openings`` makes the users' openings.  With an id key (module docstring): ``id_proof``, the bytes of the sorted-column
    proof over the id column, and ``rows``, the live rows it speaks about -- both published."""
    id_commitment: Optional[Tuple[int, int]]
    commitments: List[Optional[Tuple[int, int]]]
    range_proofs: List[bytes]
    id_total: int
    totals: List[int]
    zero_opening: np.ndarray
    columns: object = None
    id_proof: bytes = None
    rows: int = None


# ---- the statement on host integers ---------------------------------------------------------------------------------------------------
def ledger_gamma(k: int, id_commitment, commitments) -> int:
    """The challenge of the module docstring.  Points: (x, y) integers, None, or 8 / 12 affine words."""
    h = hashlib.blake2b(digest_size=64, person=PERSON)
    h.update(int(k).to_bytes(4, "little") + len(commitments).to_bytes(4, "little"))
    for c in [id_commitment] + list(commitments):
        pt = _point(c)
        h.update(bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "little") % R


def ledger_eta(k: int, id_commitment, commitments, id_total: int, totals) -> int:
    """The challenge of the opening at 0: it binds the published sums as well as the commitments (module docstring)."""
    h = hashlib.blake2b(digest_size=64, person=TOTALS_PERSON)
    h.update(int(k).to_bytes(4, "little") + len(commitments).to_bytes(4, "little"))
    for c in [id_commitment] + list(commitments):
        pt = _point(c)
        h.update(bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"))
    for t in [id_total] + list(totals):
        h.update((int(t) % R).to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "little") % R


def combined_commitment(gamma: int, id_commitment, commitments):
    """C_gamma = C_id + sum_p gamma^(p+1) C_p on host integers"""
    acc, power = _point(id_commitment), 1
    for c in commitments:
        power = power * gamma % R
        acc = g1_add(acc, g1_mul(power, _point(c)))
    return acc


def combined_value(gamma: int, first: int, rest: Sequence[int]) -> int:
    """first + sum_p gamma^(p+1) rest[p] mod r"""
    acc = 0
    for v in reversed(list(rest)):
        acc = (acc + int(v)) * gamma % R
    return (acc + int(first)) % R


def _public(public, who: str):
    """-> (C_id, [C_p]) as integer points, from a LedgerProof or the pair itself"""
    if isinstance(public, LedgerProof):
        c_id, cs = public.id_commitment, public.commitments
    else:
        try:
            c_id, cs = public
        except (TypeError, ValueError):
            raise ValueError(f"{who}: public must be a LedgerProof or (id_commitment, commitments)") from None
    cs = [_point(c) for c in cs]
    if len(cs) < 1:
        raise ValueError(f"{who}: at least one asset")
    return _point(c_id), cs


class LedgerStatement(NamedTuple):
    """What every user check of one ledger shares, computed once (``ledger_statement``): C_gamma costs P + 1 scalar multiplications
    on host integers.  ``c_gamma`` is False when a commitment is off the curve."""
    k: int
    id_commitment: object
    commitments: list
    gamma: int
    c_gamma: object


def ledger_statement(params, public, k: int = None) -> LedgerStatement:
    """``public`` (a ``LedgerProof`` or (id_commitment, commitments)) -> the ``LedgerStatement`` that ``verify_ledger_user`` and
    ``verify_ledger_users`` take in its place, so that many calls on one ledger derive gamma and C_gamma once"""
    return LedgerStatement(*_statement(params, public, k, "ledger_statement"))


def _statement(params, public, k, who: str):
    """-> (k, C_id, [C_p], gamma, C_gamma or False when a commitment is off the curve)"""
    if isinstance(public, LedgerStatement):
        if k is not None and int(k) != public.k:
            raise ValueError(f"{who}: the statement was made for k = {public.k}")
        return tuple(public)
    k = params.k if k is None else int(k)
    c_id, cs = _public(public, who)
    gamma = ledger_gamma(k, c_id, cs)
    on_curve = all(g1_on_curve(c) for c in [c_id] + cs)
    return k, c_id, cs, gamma, (combined_commitment(gamma, c_id, cs) if on_curve else False)


# ---- the prover ---------------------------------------------------------------------------------------------------------------------------
def _words_canonical(w: np.ndarray) -> np.ndarray:
    """(.., 4) uint64 words -> per element: below r"""
    mod = [(R >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    lt = np.zeros(w.shape[:-1], dtype=bool)
    eq = np.ones(w.shape[:-1], dtype=bool)
    for j in (3, 2, 1, 0):
        lt |= eq & (w[..., j] < np.uint64(mod[j]))
        eq &= w[..., j] == np.uint64(mod[j])
    return lt


ARGSORT_TILE = 1024                  # csrc/sorted.hip: SRT_TILE, the records one workgroup sorts in LDS


def _sorted_parameters(cs, who: str) -> Tuple[int, int]:
    p = cs.parameters
    if not (p.get("sorted") is True and "max_bits" in p and "acc_cols" in p and tuple(cs.unblinded_advice) == (0,)):
        raise ValueError(f"{who}: the id key is not of circuits.sorted_column")
    return p["max_bits"], p["acc_cols"]


def ledger_order(ids):
    """The permutation that brings a ledger into the order ``prove_ledger(..., id_pk=)`` wants: ``ids`` (rows, 4) GPU tensor of
    canonical Montgomery words -> (rows,) int64 GPU tensor, the rows sorted by the ids' canonical integers, equal ids by ascending row
    (a function of the input alone; ``hm_fr_argsort_bn256_dev``).  The caller applies it: ``ids[perm]``, ``balances[:, perm]``."""
    import torch

    if not (_is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[1] == 4 and ids.shape[0] >= 1):
        raise ValueError("ledger_order: ids must be a (rows, 4) int64 GPU tensor with at least one row")
    ids = ids.contiguous()
    perm = torch.empty(ids.shape[0], dtype=torch.int64, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.load().hm_fr_argsort_bn256_dev(_vp(ids.data_ptr()), ids.shape[0], _dev_ptr(perm), _vp(_stream_ptr(ids))))
    return perm


def prove_ledger(params, pk: ProvingKey, ids, balances, seed: int, check: bool = True, encoding: str = "halo2",
                 multiopen: str = "shplonk", id_pk: ProvingKey = None, lookup: str = "halo2") -> LedgerProof:
    """``balances``: a (rows, 4) GPU tensor of canonical Montgomery words, one asset, or a (P, rows, 4) stack, exactly as
    ``solvency.prove_balances`` takes them; ``ids``: a (rows, 4) GPU tensor, one id per row.  The range witness and the range proofs
    go through ``range_witness`` and ``create_proofs`` (asset p with seed + p); ``check``, ``encoding`` and
    ``multiopen``, ``lookup`` as there (the id proof takes the same three).  An id whose words are not below r raises ValueError; nothing else is checked about ids unless
    ``id_pk`` is given: a proving key of ``circuits.sorted_column`` made with ``SortedColumnLayout(k, max_bits, acc_cols, rows)`` for
    these very ``rows``.  Then the ids, as passed, go through ``sorted_witness`` and ``create_proofs`` (seed + P), the proof's bytes and
    ``rows`` are stored, and ``check`` raises ValueError when a gap does not fit -- the ids are not in ascending order, not distinct,
    or neighbours are 2^(max_bits * acc_cols) or more apart; ``ledger_order`` gives the order."""
    import torch

    who = "prove_ledger"
    check_encoding(encoding, who)
    check_multiopen(multiopen, who)
    check_lookup(lookup, who)
    cs = pk.vk.cs
    max_bits, acc_cols = _range_parameters(cs, who)
    if cs.parameters.get("sorted"):
        raise ValueError(f"{who}: pk is a key of circuits.sorted_column; it belongs in id_pk")
    if not (_is_tensor(balances) and balances.is_cuda and balances.dim() in (2, 3) and balances.shape[-1] == 4):
        raise ValueError(f"{who}: balances must be a (rows, 4) or (P, rows, 4) GPU tensor")
    values = (balances.unsqueeze(0) if balances.dim() == 2 else balances).contiguous()
    P, rows = values.shape[0], values.shape[1]
    k, n = params.k, 1 << params.k
    if P < 1 or not 1 <= rows <= n - BLINDING_ROWS:
        raise ValueError(f"{who}: between 1 and 2^k - {BLINDING_ROWS} balances per asset, at least one asset")
    if not (_is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int64 and tuple(ids.shape) == (rows, 4)):
        raise ValueError(f"{who}: ids must be a (rows, 4) GPU tensor of 64-bit words, one id per row of balances")
    if not _words_canonical(ids.cpu().numpy().view(np.uint64)).all():
        raise ValueError(f"{who}: an id is not in canonical form (its words are not below r)")
    advice, over = range_witness(values, k, max_bits, acc_cols)
    if check:
        for p, count in enumerate(over.cpu().tolist()):
            if count:
                raise ValueError(f"{who}: asset {p}: {count} balance(s) at or above 2^{max_bits * acc_cols}")
    empty = [[]]                                             # the instance column holds nothing
    id_proof = None
    if id_pk is not None:
        id_bits, id_cols = _sorted_parameters(id_pk.vk.cs, who)
        id_advice, id_over = sorted_witness(ids.contiguous(), k, id_bits, id_cols)
        bad = int(id_over.cpu()[0]) if check else 0
        if bad:
            raise ValueError(f"{who}: {bad} gap(s) between neighbouring ids do not fit {id_bits * id_cols} bits: the ids are not in "
                             "ascending order, not distinct, or too far apart (ledger_order gives the permutation that sorts them)")
    proofs = create_proofs(params, pk, advice, [empty] * P, seed, encoding=encoding, multiopen=multiopen, lookup=lookup)
    if id_pk is not None:
        id_proof = bytes(create_proofs(params, id_pk, id_advice, [empty], seed + P, encoding=encoding, multiopen=multiopen, lookup=lookup)[0])
    columns = torch.zeros((P + 1, n, 4), dtype=torch.int64, device=values.device)
    columns[0, :rows] = ids
    columns[1:] = advice[:, 0]                               # rows >= `rows` are zero
    points = [g1_ints(params.commit_lagrange(columns[j])) for j in range(P + 1)]
    coeffs = EvaluationDomain(2, k).lagrange_to_coeff(columns.clone())
    sums = [c0 * n % R for c0 in fr_ints(coeffs[:, 0].cpu().numpy().view(np.uint64))]        # n f(0) is the sum of a column
    eta = ledger_eta(k, points[0], points[1:], sums[0], sums[1:])                             # after the sums are fixed
    combined = linear_combination([coeffs[j] for j in range(P + 1)], fr_array([pow(eta, j, R) for j in range(P + 1)]))
    _, zero_opening = open_at(params, combined, 0)
    if id_pk is None:
        return LedgerProof(points[0], points[1:], list(proofs), sums[0], sums[1:], zero_opening, columns)
    return LedgerProof(points[0], points[1:], list(proofs), sums[0], sums[1:], zero_opening, columns, id_proof, rows)


def ledger_openings(params, proof_or_columns):
    """Every user's opening, (n, 8) affine words on the GPU, row i the opening of C_gamma at omega^i: the gamma-combination of the
    P + 1 columns by ``linear_combination``, then ONE ``open_all(..., form="lagrange")`` whatever P is.  A ``LedgerProof`` (the
    prover's, with its ``columns``) brings its commitments; a bare (P + 1, n, 4) GPU tensor -- the id column first -- is committed
    to here to derive gamma."""
    who = "ledger_openings"
    if isinstance(proof_or_columns, LedgerProof):
        columns = proof_or_columns.columns
        if columns is None:
            raise ValueError(f"{who}: this LedgerProof does not carry the prover's columns")
    else:
        columns = proof_or_columns
    if not (_is_tensor(columns) and columns.is_cuda and columns.dim() == 3 and columns.shape[0] >= 2 and columns.shape[-1] == 4):
        raise ValueError(f"{who}: a LedgerProof, or a (P + 1, n, 4) GPU tensor of the id column and the balance columns")
    count, n = columns.shape[0], columns.shape[1]
    if n < 1 or n & (n - 1) or n > params.n:
        raise ValueError(f"{who}: the columns must hold 2^k <= params.n rows")
    k = n.bit_length() - 1
    if isinstance(proof_or_columns, LedgerProof):
        gamma = ledger_gamma(k, proof_or_columns.id_commitment, proof_or_columns.commitments)
    else:
        points = [g1_ints(params.commit_lagrange(columns[j].contiguous())) for j in range(count)]
        gamma = ledger_gamma(k, points[0], points[1:])
    combined = linear_combination([columns[j].contiguous() for j in range(count)], fr_array([pow(gamma, j, R) for j in range(count)]))
    return open_all(params, combined, form="lagrange")


# ---- the verifiers -----------------------------------------------------------------------------------------------------------------------
def verify_ledger_totals(params, public, id_total: int, totals, zero_opening, pairing: str = "host", k: int = None) -> bool:
    """The one opening at 0: ``zero_opening`` opens C_eta = C_id + sum_p eta^(p+1) C_p at 0 to (id_total + sum_p eta^(p+1) totals[p]) / n,
    with eta = ``ledger_eta`` of the commitments and these very sums -- so sums that compensate each other under gamma, or under
    any challenge known before they were published, do not pass.  ``verify_ledger`` calls it."""
    who = "verify_ledger_totals"
    k, c_id, cs, _, c_gamma = _statement(params, public, k, who)
    if len(totals) != len(cs):
        raise ValueError(f"{who}: one total per asset")
    if c_gamma is False:
        return False
    id_total, totals = int(id_total) % R, [int(t) % R for t in totals]
    eta = ledger_eta(k, c_id, cs, id_total, totals)
    at_zero = combined_value(eta, id_total, totals) * pow(1 << k, -1, R) % R
    return verify_opening(params, combined_commitment(eta, c_id, cs), 0, at_zero, zero_opening, pairing=pairing)


def verify_ledger(params, vk: VerifyingKey, proof: LedgerProof, pairing: str = "host", tail=None, encoding: str = "halo2",
                  multiopen: str = "shplonk", id_vk: VerifyingKey = None, lookup: str = "halo2") -> bool:
    """Per asset: the range proof verifies and its first commitment is ``proof.commitments[p]``; then the one opening of C_eta at 0
    yields (id_total + sum_p eta^(p+1) totals[p]) / n, eta = ``ledger_eta`` of the commitments and these very sums.  ``tail``: six (8,) openings -- rows n - 6 .. n - 1 of ``ledger_openings``
    -- checked with the id and every balance zero (see the module docstring).  ``pairing``: where the opening checks run;
    ``encoding`` / ``multiopen`` / ``lookup``: the range proofs' (and the id proof's) wire format, multiopen scheme and lookup argument.  ``id_vk``: a verifying key of
    ``circuits.sorted_column`` (its parameters carry ``sorted=True``; anything else raises ValueError) made for the ledger's live rows;
    then False unless ``proof.id_proof`` verifies under it and its first commitment, decoded as the balance commitments are, is
    ``proof.id_commitment`` -- the ids of rows 0 .. rows - 1 are pairwise distinct (module docstring)."""
    who = "verify_ledger"
    check_encoding(encoding, who)
    check_multiopen(multiopen, who)
    check_lookup(lookup, who)
    _range_parameters(vk.cs, who)
    if vk.cs.parameters.get("sorted"):
        raise ValueError(f"{who}: vk is a key of circuits.sorted_column; it belongs in id_vk")
    if id_vk is not None:
        _sorted_parameters(id_vk.cs, who)
        if id_vk.domain.k != vk.domain.k:
            raise ValueError(f"{who}: id_vk is a key for k = {id_vk.domain.k}, vk for k = {vk.domain.k}")
    P = len(proof.commitments)
    if P < 1 or not (len(proof.range_proofs) == len(proof.totals) == P):
        return False
    k = vk.domain.k
    n = 1 << k
    for p in range(P):
        rp = proof.range_proofs[p]
        if not verify_proof(params, vk, [[]], rp, encoding=encoding, multiopen=multiopen, lookup=lookup):
            return False
        try:
            first = g1_uncompressed_int(bytes(rp[:64])) if encoding == "evm" else g1_decompress_int(bytes(rp[:32]))
        except TranscriptError:
            return False
        if first != _point(proof.commitments[p]):
            return False
    if id_vk is not None:
        ip = proof.id_proof
        if not isinstance(ip, (bytes, bytearray)) or not verify_proof(params, id_vk, [[]], bytes(ip), encoding=encoding, multiopen=multiopen, lookup=lookup):
            return False
        try:
            first = g1_uncompressed_int(bytes(ip[:64])) if encoding == "evm" else g1_decompress_int(bytes(ip[:32]))
        except TranscriptError:
            return False
        if first != _point(proof.id_commitment):
            return False
    _, _, _, _, c_gamma = _statement(params, proof, k, who)
    if c_gamma is False or not verify_ledger_totals(params, proof, proof.id_total, proof.totals, proof.zero_opening, pairing=pairing, k=k):
        return False
    if tail is not None:
        if len(tail) != BLINDING_ROWS:
            return False
        omega = domain_omega(k)
        for j in range(BLINDING_ROWS):
            if not verify_opening(params, c_gamma, pow(omega, n - BLINDING_ROWS + j, R), 0, tail[j], pairing=pairing):
                return False
    return True


def verify_ledger_user(params, public, i: int, user_id, balances, opening, pairing: str = "host", k: int = None, rows: int = None) -> bool:
    """User i's own check on host integers -- the oracle of ``verify_ledger_users``.  ``public``: a ``LedgerProof``,
    (id_commitment, commitments) or a ``LedgerStatement``; ``user_id`` and every entry of ``balances`` (one per asset): an integer or 4 words; ``opening``:
    (x, y) integers, None, or 8 affine words.  k = params.k unless given.  ``rows``: the ledger's live rows, as the id proof's key was
    made for them; an index at or behind it is False -- the distinctness proved under the id key does not reach such a row."""
    who = "verify_ledger_user"
    k, _, cs, gamma, c_gamma = _statement(params, public, k, who)
    if not 0 <= int(i) < 1 << k:
        raise ValueError(f"{who}: the row is outside the domain")
    bal = [_scalar_int(b) for b in balances]
    if len(bal) != len(cs):
        raise ValueError(f"{who}: one balance per asset")
    if c_gamma is False or (rows is not None and int(i) >= int(rows)):
        return False
    y = combined_value(gamma, _scalar_int(user_id), bal)
    return verify_opening(params, c_gamma, pow(domain_omega(k), int(i), R), y, opening, pairing=pairing)


def _words(x, shape, name: str, who: str):
    """-> a contiguous int64 GPU tensor or a contiguous uint64 array of exactly ``shape``; integers are not taken here"""
    if _is_tensor(x):
        import torch

        if not (x.is_cuda and x.dtype == torch.int64 and tuple(x.shape) == shape):
            raise ValueError(f"{who}: {name} must be a {shape} int64 GPU tensor or uint64 array")
        return x.contiguous()
    arr = np.asarray(x)
    if arr.dtype != np.uint64 or arr.shape != shape:
        raise ValueError(f"{who}: {name} must be a {shape} int64 GPU tensor or uint64 array")
    return np.ascontiguousarray(arr)


def launch_pairs(k: int, gamma: int, c_gamma, d_idx, d_ids, d_bal, d_open):
    """``hm_kzg_ledger_pairs_bn256_dev`` on device arrays as ``ledger_pairs`` lays them out, nothing checked: -> (d_g1, d_flags),
    queued on the current stream.  A hook of tools/ledger_time.py, which times the kernel alone; not part of the module's API."""
    import torch

    B, P, device = d_ids.shape[0], d_bal.shape[1], d_ids.device
    d_g1 = torch.empty((2 * B, 8), dtype=torch.int64, device=device)
    d_flags = torch.empty(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().hm_kzg_ledger_pairs_bn256_dev(
            _vp(d_open.data_ptr()), _dev_ptr(d_idx, _u32p), _vp(d_ids.data_ptr()), _vp(d_bal.data_ptr()), _ptr(fr_words(gamma)),
            _ptr(fr_words(domain_omega(k))), _ptr(g1_words(c_gamma)), k, P, B, _vp(d_g1.data_ptr()), _dev_ptr(d_flags, _u32p),
            _vp(_stream_ptr(d_g1))))
    return d_g1, d_flags


def ledger_pairs(params, public, indices, ids, balances, openings, k: int = None, device=None):
    """The upload and the kernel call of ``verify_ledger_users`` alone (a hook of the tests and of tools/ledger_time.py, not part of the module's API): -> (k, made) with made =
    (d_g1 (2B, 8) int64, d_flags (B,) int32, d_g2 (2B, 16) int64) on the device, None for B = 0, False when a commitment is off
    the curve.  What lies on the host goes up in one copy; ``device``: where to, when every argument is a host array."""
    import torch

    who = "verify_ledger_users"
    k, _, cs, gamma, c_gamma = _statement(params, public, k, who)
    P = len(cs)
    try:
        idx = np.asarray(indices.cpu() if _is_tensor(indices) else indices)
    except Exception:
        raise ValueError(f"{who}: indices must be integers") from None
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError(f"{who}: indices must be a flat sequence of integers")
    B = int(idx.size)
    if B and (int(idx.min()) < 0 or int(idx.max()) >= 1 << k):
        raise ValueError(f"{who}: a row is outside the domain")
    if B == 0:
        return k, None
    parts = [_words(ids, (B, 4), "ids", who), _words(balances, (B, P, 4), "balances", who), _words(openings, (B, 8), "openings", who)]
    if B > 1 << 20:
        raise ValueError(f"{who}: at most 2^20 users in one call")
    if c_gamma is False:
        return k, False
    tensors = [t for t in parts if _is_tensor(t)]
    device = tensors[0].device if tensors else (device or torch.device("cuda", torch.cuda.current_device()))
    if any(t.device != device for t in tensors):
        raise ValueError(f"{who}: the tensors must lie on one device")
    s_g2, g2 = g2_from_bytes(params.s_g2), g2_from_bytes(params.g2)
    g2_words = fq_array([c for q in (s_g2, g2) for c in (q[0][0], q[0][1], q[1][0], q[1][1])]).reshape(32)
    # one upload: the two G2 rows, every host array (each a multiple of 32 bytes), the indices last
    host = [g2_words] + [p.reshape(-1) for p in parts if not _is_tensor(p)]
    tail = np.zeros((B + 1) // 2, dtype=np.uint64)
    tail.view(np.uint32)[:B] = idx.astype(np.uint32)
    up = torch.from_numpy(np.concatenate(host + [tail]).view(np.int64)).to(device)
    at = 32
    d_g2 = up[:32].reshape(2, 16).repeat(B, 1)
    dev = []
    for p in parts:
        if _is_tensor(p):
            dev.append(p)
        else:
            dev.append(up[at:at + p.size].reshape(p.shape))
            at += p.size
    d_ids, d_bal, d_open = dev
    d_idx = up[at:]
    d_g1, d_flags = launch_pairs(k, gamma, c_gamma, d_idx, d_ids, d_bal, d_open)
    return k, (d_g1, d_flags, d_g2)


def verify_ledger_users(params, public, indices, ids, balances, openings, k: int = None, rows: int = None) -> List[bool]:
    """``verify_ledger_user`` for B users on the device, every answer that user's own: ``public`` as for ``verify_ledger_user``
    (a ``LedgerStatement`` spares the host products of C_gamma); ``indices`` B rows, ``ids`` (B, 4),
    ``balances`` (B, P, 4) and ``openings`` (B, 8) words, each an int64 GPU tensor or a uint64 array.  One upload of what lies on the
    host, one kernel that writes every user's pair (pi, -R) and its flag (csrc/ledger.inc), the G2 rows ([s]G2, G2) tiled on the
    device, one ``device_pairing.run_device`` call with the offsets 0, 2, 4, .., one download of statuses and flags; user b passes
    when its status is 1 and its flag is 0 -- a flagged user's rows are identities and WOULD pass the pairing, so the flag decides.
    Flagged: an opening with a coordinate word >= p or off the curve, an id or balance word pattern >= r.  A row outside the domain
    or a wrong shape or dtype raises ValueError before any launch; B = 0 gives []; a commitment off the curve gives all False.
    ``rows``: as for ``verify_ledger_user`` -- a user whose index is at or behind it is flagged on the host, as a malformed user is
    flagged by the kernel, and comes back False whatever its pairing says."""
    import torch

    k, made = ledger_pairs(params, public, indices, ids, balances, openings, k)
    if made is None:
        return []
    B = len(indices)
    if made is False:
        return [False] * B
    outside = None
    if rows is not None:                                     # the indices are a flat sequence of integers: ledger_pairs has checked
        outside = np.asarray(indices.cpu() if _is_tensor(indices) else indices) >= int(rows)
    d_g1, d_flags, d_g2 = made
    with torch.cuda.device(d_g1.device):
        d_off = torch.arange(0, 2 * B + 1, 2, dtype=torch.int32, device=d_g1.device)
        d_status = device_pairing.run_device(d_g1, d_g2, d_off, B)
        both = torch.stack([d_status, d_flags]).cpu().numpy()
    verdicts = (both[0] == 1) & (both[1] == 0)
    if outside is not None:
        verdicts &= ~outside
    return verdicts.tolist()
