"""A checkable proof of solvency over KZG: "every balance is in range, the balances sum to T, and mine is among them"
(DESIGN.md section 25).  Composition only -- every step is an entry point of another module:

    the balance column of an asset, padded with zeros to n = 2^k rows, is advice column 0 of ``circuits.overflow_check_v2(max_bits,
    acc_cols, unblinded_value=True)``; ``synthesis.range_witness`` writes its limbs; ``create_proofs`` proves that
    every row under the key's selector is below 2^(max_bits * acc_cols), and -- the value column being unblinded -- the proof's first
    commitment C is ``params.commit_lagrange`` of the padded column: the commitment ``open_all`` / ``open_at`` open.
    f being the column's polynomial, sum_i f(omega^i) = n f(0): the total is one opening of C at 0, user i's balance one at omega^i.

What the verifier of a ``BalanceProof`` learns: C, the total per asset, and that C's column is in range on the rows of the key's
selector.  What it does not hide: C is deterministic -- equal columns give equal commitments, a guessed column can be confirmed --
and every opening reveals its balance to whoever holds it.  What it does not say: nothing constrains the rows outside the key's
selector.  Make the key with ``RangeCheckLayout(k, max_bits, acc_cols, rows=2^k - 6)`` so that only the last 6 rows (which no gate
of any halo2 circuit reaches) are left; they are part of the total, and ``user_openings`` holds their openings too: whoever wants
them pinned checks ``verify_user(params, C, i, 0, opening)`` for the 6 rows i >= 2^k - 6.  ``verify_balances(..., tail=True)`` does."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import device_pairing
from ._marshal import _is_tensor
from .bn256 import FR_MODULUS, g1_ints
from .domain import EvaluationDomain
from .keygen import ProvingKey, VerifyingKey
from .kzg import g2_from_bytes
from .openings import _point, _scalar_int, domain_omega, open_all, open_at, verify_opening
from .pairing import G1_GEN, g1_add, g1_mul, g1_neg, g1_on_curve
from .prover import create_proofs
from .synthesis import BLINDING_ROWS, range_witness
from .transcript import TranscriptError, check_encoding, check_lookup, check_multiopen, g1_decompress_int, g1_uncompressed_int
from .verifier import verify_proof

R = FR_MODULUS


@dataclass
class BalanceProof:
    """Per asset p: ``commitments[p]`` the commitment to the padded balance column ((x, y) integers, None for the zero column),
    ``range_proofs[p]`` the bytes of its range proof, ``totals[p]`` the sum of the column as an integer, ``total_openings[p]`` the
    opening of the commitment at 0 (8 affine words).  ``columns``: the padded columns, a (P, n, 4) GPU tensor -- the prover's own,
    from which ``user_openings`` makes the per-user openings; not part of what is published.  ``tail_openings[p]``: the openings of
    the 6 rows no gate reaches, as zeros ((6, 8) words)."""
    commitments: List[Optional[Tuple[int, int]]]
    range_proofs: List[bytes]
    totals: List[int]
    total_openings: List[np.ndarray]
    tail_openings: List[np.ndarray] = field(default_factory=list)
    columns: object = None


def _range_parameters(cs, who: str) -> Tuple[int, int]:
    p = cs.parameters
    if "max_bits" not in p or "acc_cols" not in p:
        raise ValueError(f"{who}: the key is not of circuits.overflow_check_v2")
    if tuple(cs.unblinded_advice) != (0,):
        raise ValueError(f"{who}: the key needs overflow_check_v2(..., unblinded_value=True): a blinded value column has another commitment "
                         "than the one the openings are of")
    return p["max_bits"], p["acc_cols"]


def prove_balances(params, pk: ProvingKey, balances, seed: int, check: bool = True, encoding: str = "halo2",
                   multiopen: str = "shplonk", lookup: str = "halo2") -> BalanceProof:
    """``balances``: a (rows, 4) GPU tensor of canonical Montgomery words, one asset, or a (P, rows, 4) stack with one column per asset;
    rows <= 2^k - 6.  The witness of every asset from ``range_witness``, the range proofs from ``create_proofs``
    (asset p with seed + p), the totals n f(0) with their openings at 0 from ``open_at``.
    ``check``: a balance at or above 2^(max_bits * acc_cols) raises ValueError naming the asset and the count; without it the proof
    is made all the same, and does not verify.  ``lookup``: the lookup argument of the range proofs, "halo2" or "logup" (``prover``); the advice commitments come first under
    either, so C_p stands where it stood.  ``encoding`` / ``multiopen``: the wire format and the multiopen scheme of the range
    proofs, as ``create_proof`` names them."""
    who = "prove_balances"
    check_encoding(encoding, who)
    check_multiopen(multiopen, who)
    check_lookup(lookup, who)
    cs = pk.vk.cs
    max_bits, acc_cols = _range_parameters(cs, who)
    if not (_is_tensor(balances) and balances.is_cuda and balances.dim() in (2, 3) and balances.shape[-1] == 4):
        raise ValueError(f"{who}: balances must be a (rows, 4) or (P, rows, 4) GPU tensor")
    values = balances.unsqueeze(0) if balances.dim() == 2 else balances
    values = values.contiguous()
    P, rows = values.shape[0], values.shape[1]
    k, n = params.k, 1 << params.k
    if P < 1 or not 1 <= rows <= n - BLINDING_ROWS:
        raise ValueError(f"{who}: between 1 and 2^k - {BLINDING_ROWS} balances per asset, at least one asset")
    advice, over = range_witness(values, k, max_bits, acc_cols)
    if check:
        for p, count in enumerate(over.cpu().tolist()):
            if count:
                raise ValueError(f"{who}: asset {p}: {count} balance(s) at or above 2^{max_bits * acc_cols}")
    empty = [[]]                                             # the instance column holds nothing
    proofs = create_proofs(params, pk, advice, [empty] * P, seed, encoding=encoding, multiopen=multiopen, lookup=lookup)
    columns = advice[:, 0].contiguous()                      # (P, n, 4): rows >= `rows` are zero
    coeffs = EvaluationDomain(2, k).lagrange_to_coeff(columns.clone())
    omega = domain_omega(k)
    commitments, totals, total_openings, tails = [], [], [], []
    for p in range(P):
        commitments.append(g1_ints(params.commit_lagrange(columns[p])))
        at_zero, opening = open_at(params, coeffs[p], 0)
        totals.append(at_zero * n % R)
        total_openings.append(opening)
        tails.append(np.stack([open_at(params, coeffs[p], pow(omega, i, R))[1] for i in range(n - BLINDING_ROWS, n)]))
    return BalanceProof(commitments, list(proofs), totals, total_openings, tails, columns)


def verify_balances(params, vk: VerifyingKey, proof: BalanceProof, pairing: str = "host", tail: bool = False,
                    encoding: str = "halo2", multiopen: str = "shplonk", lookup: str = "halo2") -> bool:
    """Per asset: the range proof verifies; its first 32-byte slot -- the commitment to advice column 0 -- decompresses to
    ``proof.commitments[p]``; the opening at 0 yields ``totals[p]`` / n.  ``tail``: also the 6 openings of ``tail_openings[p]``, as
    zeros on the rows 2^k - 6 .. 2^k - 1 (see the module docstring).  ``pairing``: where the opening checks run
    (``openings.verify_opening``).  ``encoding``: the range proofs' wire format; with "evm" the commitment is the first 64 bytes,
    read as they stand: nothing is decompressed.  ``multiopen``: the range proofs' multiopen scheme; ``lookup``: their lookup
    argument, as ``prove_balances`` was called."""
    check_encoding(encoding, "verify_balances")
    check_multiopen(multiopen, "verify_balances")
    check_lookup(lookup, "verify_balances")
    _range_parameters(vk.cs, "verify_balances")
    P = len(proof.commitments)
    if P < 1 or not (len(proof.range_proofs) == len(proof.totals) == len(proof.total_openings) == P):
        return False
    k = vk.domain.k
    n, n_inv, omega = 1 << k, pow(1 << k, -1, R), domain_omega(k)
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
        if not verify_opening(params, proof.commitments[p], 0, int(proof.totals[p]) % R * n_inv % R, proof.total_openings[p], pairing=pairing):
            return False
        if tail:
            if len(proof.tail_openings) != P or len(proof.tail_openings[p]) != BLINDING_ROWS:
                return False
            rows = list(range(n - BLINDING_ROWS, n))
            if not all(verify_users(params, proof.commitments[p], rows, [0] * BLINDING_ROWS, proof.tail_openings[p], pairing=pairing, k=k)):
                return False
    return True


def user_openings(params, proof_or_balances):
    """All per-user openings: ``open_all(..., form="lagrange")`` on the padded columns.  A ``BalanceProof`` (the prover's, with its
    ``columns``) gives (P, n, 8) affine words; a (rows, 4) / (P, rows, 4) GPU tensor of balances is padded with zeros to n = 2^k
    rows and gives (n, 8) / (P, n, 8).  Row i is the opening at omega^i."""
    import torch

    if isinstance(proof_or_balances, BalanceProof):
        if proof_or_balances.columns is None:
            raise ValueError("user_openings: this BalanceProof does not carry the prover's columns")
        return open_all(params, proof_or_balances.columns, form="lagrange")
    b = proof_or_balances
    if not (_is_tensor(b) and b.is_cuda and b.dim() in (2, 3) and b.shape[-1] == 4):
        raise ValueError("user_openings: a BalanceProof, or a (rows, 4) / (P, rows, 4) GPU tensor of balances")
    n = 1 << params.k
    if b.shape[-2] > n:
        raise ValueError("user_openings: more balances than 2^k rows")
    cols = torch.zeros(tuple(b.shape[:-2]) + (n, 4), dtype=torch.int64, device=b.device)
    cols[..., :b.shape[-2], :] = b
    return open_all(params, cols, form="lagrange")


def verify_user(params, commitment, i: int, balance, opening, pairing: str = "host", k: int = None) -> bool:
    """``verify_opening`` of ``commitment`` at omega^i (omega the 2^k-th root of unity, k = params.k unless given) with the value
    ``balance`` (an integer or 4 words)."""
    k = params.k if k is None else int(k)
    if not 0 <= int(i) < 1 << k:
        raise ValueError("verify_user: the row is outside the domain")
    return verify_opening(params, commitment, pow(domain_omega(k), int(i), R), balance, opening, pairing=pairing)


def verify_users(params, commitment, indices, balances, openings, pairing: str = "host", k: int = None) -> List[bool]:
    """``verify_user`` for many users, each with its own pairing check -- no random combination, so every answer is that user's --
    and, with ``pairing="device"``, all checks in one launch chain (``device_pairing.pairing_checks``).  ``openings``: (B, 8) words, a
    GPU tensor or an array."""
    k = params.k if k is None else int(k)
    idx = [int(i) for i in indices]
    if any(not 0 <= i < 1 << k for i in idx):
        raise ValueError("verify_users: a row is outside the domain")
    if pairing not in device_pairing.MODES:
        raise ValueError(f"pairing must be one of {device_pairing.MODES}, got {pairing!r}")
    pis = openings.detach().cpu().numpy() if _is_tensor(openings) else np.asarray(openings)
    pis = pis.view(np.uint64).reshape(-1, 8)
    ys = [_scalar_int(b) for b in (balances.detach().cpu().numpy().view(np.uint64).reshape(-1, 4) if _is_tensor(balances) else balances)]
    if len(pis) != len(idx) or len(ys) != len(idx):
        raise ValueError("verify_users: one balance and one opening per row")
    c = _point(commitment)
    if not g1_on_curve(c):
        return [False] * len(idx)
    omega, s_g2, g2 = domain_omega(k), g2_from_bytes(params.s_g2), g2_from_bytes(params.g2)
    checks, valid = [], []
    for i, y, w in zip(idx, ys, pis):
        pi = g1_ints(w)
        valid.append(g1_on_curve(pi))
        if not valid[-1]:
            pi = None
        rhs = g1_add(g1_add(c, g1_neg(g1_mul(y, G1_GEN))), g1_mul(pow(omega, i, R), pi))
        checks.append([(pi, s_g2), (g1_neg(rhs), g2)])
    if pairing == "device":
        status, _ = device_pairing.run(checks)
        answers = [s == 1 for s in status]
    else:
        answers = [device_pairing.check(pairs, "host") for pairs in checks]
    return [a and v for a, v in zip(answers, valid)]
