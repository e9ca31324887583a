"""All KZG openings of a polynomial on its domain (Feist / Khovratovich, "FK20"), and what verifies them.

The direct KZG form of a proof of solvency: commit to the balance column with one MSM; user i's proof is the opening of that
commitment at omega^i; the total is n f(0), one more opening.  One opening is a ``kate_division`` and an MSM (``open_at``); all n of
them at once cost one Fr NTT of size 2n, 2n scalar multiplications and two FFTs over G1 (``open_all``; csrc/g1_fft.hip, DESIGN.md
section 22):

    f = sum_{j<n} f_j X^j, g_i = [s^i]G1:   pi_t = [(f(s) - f(w^t)) / (s - w^t)]G1 = sum_m w^(tm) h_m,   w = omega_n,
    h_m = sum_{i=0}^{n-2-m} f_{m+1+i} g_i  (m <= n - 2),  h_{n-1} = the identity.

h is a Toeplitz product, computed through a circulant of size 2n: x_i = g_{n-2-i} for i <= n - 2 and the identity elsewhere;
y_0 = f_{n-1}, y_1 .. y_{n+1} = 0, y_{n+1+j} = f_j for 1 <= j <= n - 2.  With s^ = G1-FFT_2n(x) (``OpeningTable``: the SRS alone),
c^ = NTT_2n(y) and u^_i = [c^_i] s^_i, h is the first n entries of (2n)^-1 G1-FFT_2n(u^) taken with omega_2n^-1, and the proofs are
G1-FFT_n(h).  ``open_all_ints`` states both routes on host integers for tiny n.

Points are (.., 8) 64-bit words of affine Montgomery coordinates, (0, 0) for the identity; scalars (.., 4) Montgomery words.
"""
from __future__ import annotations

import ctypes
import secrets

import numpy as np

from . import _lib
from ._marshal import _is_tensor, _stream_ptr, _tensor_rows
from .arithmetic import InvalidPointError, best_multiexp, eval_polynomial, g1_check, kate_division, register_bases, release_bases
from .bn256 import FR_MODULUS, FR_ROOT_OF_UNITY, FR_S, fr_array, fr_int, fr_words, g1_ints
from .domain import EvaluationDomain
from .kzg import g2_from_bytes
from . import device_pairing
from .pairing import G1_GEN, g1_add, g1_mul, g1_neg, g1_on_curve

R = FR_MODULUS
LOG_N_MAX = 23                      # the circulant has 2n points and best_fft over G1 takes 2^24


def domain_omega(k: int) -> int:
    """``EvaluationDomain(., k).omega``: the 2^k-th root of unity"""
    return pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R)


def _log2_exact(n: int, who: str) -> int:
    if n < 1 or n & (n - 1):
        raise ValueError(f"{who}: the length must be a power of two, got {n}")
    return n.bit_length() - 1


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
class OpeningTable:
    """s^ for size 2^k <= params.n: a (2^(k+1), 8) GPU tensor in ``table``, built from the first 2^k monomial points of ``params`` and
    kept on the params object (one per k).  Needs ``params.g_points`` (setup(..., keep_points=True), read() or from_monomial())."""

    def __new__(cls, params, k: int = None):
        k = params.k if k is None else int(k)
        if k < 0 or k > LOG_N_MAX:
            raise ValueError(f"OpeningTable: k must lie in 0 .. {LOG_N_MAX}, got {k}")
        if k > params.k:
            raise ValueError("OpeningTable: k exceeds the size of the parameters")
        if not hasattr(params, "g_points"):
            raise ValueError("OpeningTable: the affine points were not kept (setup(..., keep_points=True))")
        cache = params.__dict__.setdefault("_opening_tables", {})
        if k not in cache:
            self = super().__new__(cls)
            self.k, self.n = k, 1 << k
            self.table = self._build(params._device_points(params.g_points), k)
            cache[k] = self
        return cache[k]

    @staticmethod
    def _build(g, k: int):
        import torch

        n = 1 << k
        if _tensor_rows(g, 8, "g_points") < n:
            raise ValueError("OpeningTable: fewer than 2^k points")
        table = torch.empty((2 * n, 8), dtype=torch.int64, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().hm_kzg_open_table_bn256_dev(ctypes.c_void_p(g.data_ptr()), k, ctypes.c_void_p(table.data_ptr()),
                                                               ctypes.c_void_p(_stream_ptr(g))))
        return table


def arrange_points(g, k: int):
    """x of the circulant as a new (2^(k+1), 8) tensor: slot i <= n - 2 is g[n - 2 - i], the others (0, 0) -- what ``OpeningTable``
    transforms, spelled with tensor indexing"""
    import torch

    n = 1 << k
    x = torch.zeros((2 * n, 8), dtype=torch.int64, device=g.device)
    if n >= 2:
        x[:n - 1] = torch.flip(g[:n - 1], dims=[0])
    return x


# ---- all openings -------------------------------------------------------------------------------------------------------------------------
def open_all(params, polys, form: str = "coeff", part_ms: list = None):
    """Every opening of the commitment of each polynomial on its own domain: ``polys`` is an (n, 4) GPU tensor, or a (P, n, 4) stack,
    with n = 2^k <= params.n; returns (n, 8) or (P, n, 8) affine words, row i the proof at omega_n^i.  ``form="lagrange"`` takes the
    evaluations on the domain instead (``lagrange_to_coeff`` runs on a copy; the caller's tensor is not modified).  ``part_ms``: a list
    that receives the device milliseconds of the last polynomial's seven steps (tools/open_all_time.py)."""
    import torch

    if form not in ("coeff", "lagrange"):
        raise ValueError(f"open_all: unknown form {form!r} (coeff or lagrange)")
    if not _is_tensor(polys):
        raise TypeError("open_all: polys must be a GPU tensor (coefficients stay in HBM)")
    if polys.dim() not in (2, 3) or polys.shape[-1] != 4:
        raise ValueError("open_all: expected (n, 4) or (P, n, 4) words")
    n = polys.shape[-2]
    k = _log2_exact(n, "open_all")
    if n > params.n:
        raise ValueError("open_all: the polynomial is longer than the parameters")
    count = polys.shape[0] if polys.dim() == 3 else 1
    _tensor_rows(polys, 4, "polys")
    table = OpeningTable(params, k)
    coeffs = polys
    if form == "lagrange":
        coeffs = EvaluationDomain(2, k).lagrange_to_coeff(polys.clone())
    out = torch.empty(tuple(polys.shape[:-1]) + (8,), dtype=torch.int64, device=polys.device)
    if count == 0:
        return out
    lib = _lib.load()
    args = (ctypes.c_void_p(table.table.data_ptr()), ctypes.c_void_p(coeffs.data_ptr()), k, count, ctypes.c_void_p(out.data_ptr()))
    with torch.cuda.device(polys.device):
        st = ctypes.c_void_p(_stream_ptr(polys))
        if part_ms is None:
            _lib.check(lib.hm_kzg_open_all_bn256_dev(*args, st))
        else:
            ms = (ctypes.c_double * 7)()
            _lib.check(lib.hm_kzg_open_all_timed_bn256_dev(*args, ms, st))
            part_ms[:] = list(ms)
    return out


def _scalar_int(v) -> int:
    return int(v) % R if isinstance(v, (int, np.integer)) else fr_int(np.asarray(v, dtype=np.uint64))


def open_at(params, poly, z):
    """One opening by the existing route, spelled out: value = ``eval_polynomial(poly, z)``, quotient = ``kate_division(poly, z)``,
    proof = ``params.commit(quotient)``.  ``poly``: an (n, 4) GPU tensor of coefficients, n <= params.n; ``z``: any field element (an
    integer or its 4 words) -- 0 for the total, omega^i for user i.  Returns (value as an integer, proof as 8 affine words)."""
    if not _is_tensor(poly):
        raise TypeError("open_at: poly must be a GPU tensor (coefficients stay in HBM)")
    n = _tensor_rows(poly, 4, "poly")
    if n == 0 or n > params.n:
        raise ValueError("open_at: the polynomial must hold 1 .. params.n coefficients")
    zw = fr_words(_scalar_int(z))
    value = fr_int(eval_polynomial(poly.reshape(1, n, 4), zw.reshape(1, 4)))
    proof = np.zeros(8, dtype=np.uint64)
    if n > 1:                                        # a constant has the empty quotient: the identity
        proof[:] = params.commit(kate_division(poly.reshape(n, 4), zw))[:8]
    return value, proof


# ---- verification -------------------------------------------------------------------------------------------------------------------------
def _point(p):
    """a G1 point as (x, y) integers or None: from that form itself, or from 8 / 12 Montgomery words"""
    if p is None or (isinstance(p, tuple) and len(p) == 2 and all(isinstance(c, int) for c in p)):
        return p
    w = p.detach().cpu().numpy() if _is_tensor(p) else np.asarray(p)
    return g1_ints(w.view(np.uint64) if w.dtype == np.int64 else w)


def verify_opening(params, commitment, z, value, proof, pairing: str = "host") -> bool:
    """e(pi, [s]G2) = e(C - [y]G + [z]pi, G2) on host integers: one pairing check, no G2 arithmetic.  ``commitment`` / ``proof``:
    (x, y) integers, None for the identity, or 8 / 12 affine words; ``z`` / ``value``: integers or 4 words.  A point off the curve
    gives False.  ``pairing="device"`` runs the pairing check on the GPU (``device_pairing``): the same boolean."""
    c, pi = _point(commitment), _point(proof)
    if not g1_on_curve(c) or not g1_on_curve(pi):
        return False
    zz, y = _scalar_int(z), _scalar_int(value)
    rhs = g1_add(g1_add(c, g1_neg(g1_mul(y, G1_GEN))), g1_mul(zz, pi))
    return device_pairing.check([(pi, g2_from_bytes(params.s_g2)), (g1_neg(rhs), g2_from_bytes(params.g2))], pairing)


def verify_openings(params, commitment, indices, values, proofs, seed=None, k: int = None, pairing: str = "host") -> bool:
    """The openings of one commitment at omega_n^(indices[b]) with the claimed ``values[b]`` and ``proofs[b]`` (a (B, 8) GPU tensor, as
    ``open_all`` returns it or rows gathered from it), checked together with one pairing: with weights r_b and n = 2^k (``k``
    defaults to params.k),

        L = sum r_b pi_b,   R = (sum r_b) C - (sum r_b y_b) G + sum (r_b omega^(i_b)) pi_b,   e(L, [s]G2) = e(R, G2).

    The two sums over the proofs are MSMs on the device tensor, after ``g1_check``: an invalid point gives False.  r_b in [1, r) comes
    from ``secrets`` when ``seed`` is None, else from (seed, b) as ``proof_layout.derive_randomizer`` makes it.
    ``pairing="device"`` runs that one pairing check on the GPU (``device_pairing``): the same boolean."""
    from .proof_layout import derive_randomizer

    k = params.k if k is None else int(k)
    idx = [int(i) for i in indices]
    ys = [_scalar_int(v) for v in values]
    if not _is_tensor(proofs):
        raise TypeError("verify_openings: proofs must be a GPU tensor of (B, 8) words")
    b_count = _tensor_rows(proofs, 8, "proofs")
    if len(idx) != b_count or len(ys) != b_count:
        raise ValueError("verify_openings: one index and one value per proof")
    if any(not 0 <= i < (1 << k) for i in idx):
        raise ValueError("verify_openings: an index outside the domain")
    c = _point(commitment)
    if not g1_on_curve(c):
        return False
    if b_count == 0:
        return True
    try:
        g1_check(proofs)
    except InvalidPointError:
        return False
    rs = [secrets.randbelow(R - 1) + 1 if seed is None else derive_randomizer(seed, b) for b in range(b_count)]
    omega = domain_omega(k)
    handle = register_bases(proofs, plain=True)
    try:
        left = g1_ints(best_multiexp(fr_array(rs), handle))
        moved = g1_ints(best_multiexp(fr_array([r * pow(omega, i, R) % R for r, i in zip(rs, idx)]), handle))
    finally:
        release_bases(handle)
    right = g1_add(g1_add(g1_mul(sum(rs) % R, c), g1_neg(g1_mul(sum(r * y for r, y in zip(rs, ys)) % R, G1_GEN))), moved)
    return device_pairing.check([(left, g2_from_bytes(params.s_g2)), (g1_neg(right), g2_from_bytes(params.g2))], pairing)


# ---- the twin on host integers -------------------------------------------------------------------------------------------------------------
def _g1_dft_ints(points, omega: int):
    """out[t] = sum_j [omega^(t j)] points[j], by the definition (tiny sizes only)"""
    m = len(points)
    return [_sum_ints(g1_mul(pow(omega, t * j, R), p) for j, p in enumerate(points)) for t in range(m)]


def _sum_ints(points):
    acc = None
    for p in points:
        acc = g1_add(acc, p)
    return acc


def open_all_ints(g, coeffs, route: str = "definition"):
    """``open_all`` on ``pairing``'s integer G1 for tiny n: ``g`` the first n monomial points as (x, y) integers, ``coeffs`` n integers;
    returns the n proofs (None = the identity).  ``route="definition"``: h_m by its sum, then the DFT of h.  ``route="circulant"``: the
    arrangement of the module's docstring, every transform by its definition -- what the kernels compute, index for index."""
    n = len(coeffs)
    k = _log2_exact(n, "open_all_ints")
    if len(g) < n:
        raise ValueError("open_all_ints: fewer points than coefficients")
    f = [int(c) % R for c in coeffs]
    if route == "definition":
        h = [_sum_ints(g1_mul(f[m + 1 + i], g[i]) for i in range(n - 1 - m)) for m in range(n)]
    elif route == "circulant":
        w2 = domain_omega(k + 1)
        x = [g[n - 2 - i] if i <= n - 2 else None for i in range(2 * n)]
        y = [0] * (2 * n)
        y[0] = f[n - 1]
        for j in range(1, n - 1):
            y[n + 1 + j] = f[j]
        s_hat = _g1_dft_ints(x, w2)
        c_hat = [sum(y[j] * pow(w2, i * j, R) for j in range(2 * n)) % R for i in range(2 * n)]
        inv = pow(2 * n, -1, R)
        u_hat = [g1_mul(c_hat[i] * inv % R, s_hat[i]) for i in range(2 * n)]
        h = _g1_dft_ints(u_hat, pow(w2, -1, R))[:n]
    else:
        raise ValueError(f"open_all_ints: unknown route {route!r} (definition or circulant)")
    return _g1_dft_ints(h, domain_omega(k))
