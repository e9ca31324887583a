"""``keygen_vk`` / ``keygen_pk`` of ``halo2_proofs::plonk`` for a constraint system of ``circuits`` and a layout of ``synthesis``, with
``permutation::keygen::Assembly`` on the GPU (csrc/keygen.inc): the copy constraints go up as pairs of cell
ids, a lock-free union-find joins them, a sort orders every class and one launch links it into a cycle; one more launch turns the
cells into the sigma columns.  The fixed columns, ``l0`` / ``l_last`` / ``l_active``, the coefficient forms and the extended cosets come
from the ``EvaluationDomain`` calls, the commitments from the batch MSM.  Everything a key holds is a device tensor except the
commitments.  ``synthesis.permutation_cells`` / ``permutation_columns`` are the CPU twins the tests compare against.

Not here: selector compression.  ``create_proof`` / ``verify_proof``: ``prover`` / ``verifier`` (section 17)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _is_tensor, _ptr, _stream_ptr, _u32p
from .arithmetic import best_multiexp_batch
from .circuits import ConstraintSystem
from .domain import FR_GENERATOR, FR_MODULUS, FR_S, EvaluationDomain, fr_words
from .kzg import ParamsKZG
from .poseidon import ints_to_words

R = FR_MODULUS
FR_DELTA = pow(FR_GENERATOR, 1 << FR_S, R)          # ``Fr::DELTA``: generates the cosets the permutation argument's columns stand on


def _u32(t):
    return _dev_ptr(t, _u32p)


def copy_pairs(cs: ConstraintSystem, layout) -> np.ndarray:
    """``layout.copies()`` as an (m, 2) uint32 array of cell ids: cell (column j of ``cs.equality``, row i) is j * n + i."""
    index = {col: j for j, col in enumerate(cs.equality)}
    n = layout.n
    if len(index) * n > 1 << 32:
        raise ValueError("copy_pairs: more than 2^32 cells")
    out = []
    for (ka, ca, ra), (kb, cb, rb) in layout.copies():
        if (ka, ca) not in index or (kb, cb) not in index:
            raise ValueError(f"permutation_cells: a copy touches a column without equality: {(ka, ca)} / {(kb, cb)}")
        out.append((index[(ka, ca)] * n + ra, index[(kb, cb)] * n + rb))
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def permutation_cells_dev(pairs, P: int, k: int, device=None, return_dropped: bool = False):
    """sigma as cells: the uint32 device tensor of P * 2^k ids that ``hm_permutation_assemble_dev`` makes of the copies ``pairs``,
    cell for cell ``synthesis.permutation_cells``.  A host array is validated (every id below P * 2^k) and uploaded; a device tensor
    ((m, 2) uint32) is taken as it is, and a pair with an id out of range is dropped on the device.  ``return_dropped``: also the
    one-word device tensor that counts those."""
    import torch

    cells = P << k
    if P < 1 or cells > 1 << 32:
        raise ValueError("permutation_cells_dev: need 1 <= P and P * 2^k <= 2^32")
    if _is_tensor(pairs):
        if not pairs.is_cuda or pairs.dtype != torch.uint32 or not pairs.is_contiguous() or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError("permutation_cells_dev: a device tensor of pairs must be a contiguous (m, 2) uint32 GPU tensor")
        d_pairs = pairs
    else:
        host = np.asarray(pairs)
        if host.size and (host.min() < 0 or host.max() >= cells):
            raise ValueError(f"permutation_cells_dev: a cell id is not below P * 2^k = {cells}")
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1, 2)
        d_pairs = torch.from_numpy(host).to(device or torch.device("cuda", torch.cuda.current_device()))
    m = d_pairs.shape[0]
    if 2 * m > 1 << 31:
        raise ValueError("permutation_cells_dev: more than 2^30 copies")
    out = torch.empty(cells, dtype=torch.uint32, device=d_pairs.device)
    dropped = torch.empty(1, dtype=torch.uint32, device=d_pairs.device) if return_dropped else None
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().hm_permutation_assemble_dev(_u32(d_pairs) if m else None, m, P, k, _u32(out),
                                                           _u32(dropped) if return_dropped else None, ctypes.c_void_p(_stream_ptr(out))))
    return (out, dropped) if return_dropped else out


def permutation_columns_from_cells(sigma_cells, P: int, k: int, omega: int, delta: int):
    """The (P, 2^k, 4) sigma columns of a uint32 device tensor of P * 2^k cell ids: cell j * 2^k + i stands for delta^j * omega^i."""
    import torch

    if not (_is_tensor(sigma_cells) and sigma_cells.is_cuda and sigma_cells.dtype == torch.uint32 and sigma_cells.is_contiguous()
            and sigma_cells.numel() == P << k):
        raise ValueError("permutation_columns_from_cells: need a contiguous uint32 GPU tensor of P * 2^k cell ids")
    out = torch.empty((P, 1 << k, 4), dtype=torch.int64, device=sigma_cells.device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().hm_permutation_columns_bn256_fr_dev(_u32(sigma_cells), P, k, _ptr(fr_words(omega)), _ptr(fr_words(delta)),
                                                                   ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(_stream_ptr(out))))
    return out


def permutation_columns_dev(cs: ConstraintSystem, layout, omega: int, delta: int, device=None):
    """The sigma columns as a (P, n, 4) int64 device tensor, word for word ``synthesis.permutation_columns``, assembled on the GPU."""
    P, k = len(cs.equality), layout.k
    return permutation_columns_from_cells(permutation_cells_dev(copy_pairs(cs, layout), P, k, device=device), P, k, omega, delta)


@dataclass
class VerifyingKey:
    domain: EvaluationDomain
    cs: ConstraintSystem
    fixed_commitments: np.ndarray              # (num_fixed, 12) words: (x, y, 1), or zeros for the identity
    permutation_commitments: np.ndarray        # (len(cs.equality), 12)


@dataclass
class ProvingKey:
    vk: VerifyingKey
    l0: "object"                               # (n, 4) Lagrange values, as the three below
    l_last: "object"
    l_active: "object"
    fixed_values: "object"                     # (num_fixed, n, 4)
    fixed_polys: "object"
    fixed_cosets: Optional["object"]           # (num_fixed, 2^extended_k, 4); None with cosets=False
    permutation_values: "object"               # (len(cs.equality), n, 4)
    permutation_polys: "object"
    permutation_cosets: Optional["object"]


def _key_columns(params: ParamsKZG, cs: ConstraintSystem, layout, who: str):
    """the domain, the fixed columns and the sigma columns in Lagrange form on the current device"""
    import torch

    if params.k != layout.k:
        raise ValueError(f"{who}: the parameters are for k = {params.k}, the layout for k = {layout.k}")
    layout.check_constraint_system(cs)
    dom = EvaluationDomain(cs.degree(), layout.k)
    device = torch.device("cuda", torch.cuda.current_device())
    # the fixed columns are Python integers with few distinct values (selectors, round constants per hash): convert each value once
    distinct: dict = {}
    index = np.fromiter((distinct.setdefault(v, len(distinct)) for col in layout.fixed_columns() for v in col), dtype=np.int64,
                        count=cs.num_fixed * layout.n)
    words = ints_to_words(list(distinct))[index]
    fixed = torch.from_numpy(words.view(np.int64)).to(device).reshape(cs.num_fixed, layout.n, 4)
    sigma = permutation_columns_dev(cs, layout, dom.omega, FR_DELTA, device=device)
    return dom, fixed, sigma


def keygen_vk(params: ParamsKZG, cs: ConstraintSystem, layout) -> VerifyingKey:
    """``keygen_vk``: the commitments to the fixed columns and to the sigma columns, ``commit_lagrange`` through one batch MSM."""
    dom, fixed, sigma = _key_columns(params, cs, layout, "keygen_vk")
    cols = [fixed[i] for i in range(fixed.shape[0])] + [sigma[j] for j in range(sigma.shape[0])]
    com = best_multiexp_batch(cols, params.g_lagrange_handle)
    return VerifyingKey(dom, cs, com[:fixed.shape[0]].copy(), com[fixed.shape[0]:].copy())


def keygen_pk(params: ParamsKZG, vk: VerifyingKey, cs: ConstraintSystem, layout, cosets: bool = True) -> ProvingKey:
    """``keygen_pk``: the columns of the key in Lagrange form, in coefficient form and (``cosets``) on the extended coset, and the
    three row selectors of the arguments: l0 on row 0, l_last on row n - blinding_factors - 1, l_active on the rows before it."""
    import torch

    dom, fixed, sigma = _key_columns(params, cs, layout, "keygen_pk")
    if (vk.domain.k, vk.domain.extended_k) != (dom.k, dom.extended_k):
        raise ValueError("keygen_pk: the verifying key is of another domain")
    n, usable = layout.n, layout.n - cs.blinding_factors - 1
    one = torch.from_numpy(fr_words(1).view(np.int64)).to(fixed.device)
    l0, l_last, l_active = (torch.zeros((n, 4), dtype=torch.int64, device=fixed.device) for _ in range(3))
    l0[0] = one
    l_last[usable] = one
    l_active[:usable] = one
    fixed_polys, sigma_polys = dom.lagrange_to_coeff(fixed.clone()), dom.lagrange_to_coeff(sigma.clone())
    return ProvingKey(vk, l0, l_last, l_active, fixed, fixed_polys, dom.coeff_to_extended(fixed_polys) if cosets else None,
                      sigma, sigma_polys, dom.coeff_to_extended(sigma_polys) if cosets else None)
