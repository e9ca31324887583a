"""Host-side mirror of ``halo2_proofs::arithmetic`` for BN256 (same names, argument meaning and
error behaviour as the reference's crate, /root/reference/Cargo.toml:10, tag v2023_02_02):

    best_multiexp(coeffs: &[Fr], bases: &[G1Affine]) -> G1      (assert_eq!(coeffs.len(), bases.len()))
    best_fft(a: &mut [Fr], omega: Fr, log_n: u32)               (assert_eq!(a.len(), 1 << log_n))

Arrays are ``numpy.uint64`` in the reference's memory layout (little-endian
Montgomery limbs; Fr = 4, G1Affine = 8, G1 = 12 words) or CUDA/HIP ``torch`` tensors of dtype
int64/uint64 with the same shape, in which case the data never leaves HBM.  Everything goes
through the C ABI of libhalo2_mi355x.so; if that library is missing these functions raise.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Union

import numpy as np

from . import _lib
from ._marshal import _is_tensor, _np, _ptr, _ptr_array, _stream_ptr, _tensor_rows, _u32p
from .bn256 import (FQ_MODULUS, FQ_ONE_MONT, FR_MODULUS, FR_ROOT_OF_UNITY, FR_S, G1_GENERATOR, fq_words,  # noqa: F401  (re-exported)
                    fr_array, fr_words)

class BasesHandle:
    """A device-resident, pre-converted base set (``ParamsKZG::g`` / ``g_lagrange``)."""

    def __init__(self, handle: int, n: int):
        self.handle, self.n = handle, n

    def __len__(self) -> int:
        return self.n


def register_bases(bases, precompute: bool = False, plain: bool = False) -> BasesHandle:
    """Upload + convert a base set once (``ParamsKZG::g`` / ``g_lagrange``: it lives for the whole proving session).

    By default the library chooses the layout: from 2^17 points (``hm_set_fixed_base_threshold``) it also stores
    2^(offset of window j) * P_i for every window -- the fixed-base table, W x the memory, built once (0.22 s at 2^24) --
    so that whole-set MSMs share one bucket set.  ``precompute=True`` asks for the table at any size; ``plain=True``
    for one copy of the points and never a table: the layout for a TRANSIENT set that serves one MSM."""
    if precompute and plain:
        raise ValueError("register_bases: precompute and plain exclude each other")
    lib = _lib.load()
    h = ctypes.c_uint64(0)
    kind = "_precomp" if precompute else "_plain" if plain else ""
    if _is_tensor(bases):
        n = _tensor_rows(bases, 8, "bases")
        fn = getattr(lib, f"hm_register_bases{kind}_dev")
        _lib.check(fn(ctypes.c_void_p(bases.data_ptr()), n, ctypes.c_void_p(_stream_ptr(bases)), ctypes.byref(h)))
    else:
        b = _np(bases, 8, "bases")
        n = b.shape[0]
        fn = getattr(lib, f"hm_register_bases{kind}")
        _lib.check(fn(_ptr(b), n, ctypes.byref(h)))
    return BasesHandle(h.value, n)


def to_host(t) -> np.ndarray:
    """A GPU tensor of Fr / Fq words as a fresh (rows, words) uint64 numpy array, copied by the LIBRARY (``hm_copy_to_host``: its pinned
    staging lanes).  ``tensor.cpu()`` hands the fresh destination to hipMemcpy, which pins it on the fly (csrc/xfer.hip's finding): a
    harness that measures the library's host copies keeps that machinery out of its own process state."""
    if not _is_tensor(t) or not t.is_cuda:
        raise TypeError("to_host: a GPU tensor is expected")
    import torch
    t = t.contiguous()
    out = np.empty(tuple(t.shape), dtype=np.uint64)
    torch.cuda.current_stream(t.device).synchronize()
    _lib.check(_lib.load().hm_copy_to_host(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(t.data_ptr()), out.nbytes))
    return out


def bases_info(handle: BasesHandle) -> dict:
    """``hm_get_bases_info``: which layout the registration ended up with (``table_windows`` == 0: plain), the HBM it
    holds, and how many default registrations of the process fell back to the plain layout for lack of memory."""
    info = _lib.BasesInfo()
    _lib.check(_lib.load().hm_get_bases_info(ctypes.c_uint64(handle.handle), ctypes.byref(info)))
    return {k: getattr(info, k) for k, _ in info._fields_}


def release_bases(handle: BasesHandle) -> None:
    _lib.check(_lib.load().hm_release_bases(ctypes.c_uint64(handle.handle)))


def best_multiexp(coeffs, bases: Union[np.ndarray, BasesHandle, "object"], offset: int = 0) -> np.ndarray:
    """sum_i coeffs[i] * bases[i] -> G1 as 12 words (x, y, 1) Montgomery, or all-zero for the identity.

    ``bases`` may be an array/tensor (converted per call, as the drop-in does: host arrays through the library's
    digest-keyed reuse, GPU tensors as a PLAIN set registered for this one MSM -- never the fixed-base table, whose build
    costs ten MSMs) or a ``BasesHandle`` (then ``coeffs`` pairs with ``bases[offset : offset + len(coeffs)]``)."""
    lib = _lib.load()
    out = np.zeros(12, dtype=np.uint64)
    if isinstance(bases, BasesHandle):
        if _is_tensor(coeffs):
            n = _tensor_rows(coeffs, 4, "coeffs")
            _lib.check(lib.hm_msm_bn256_g1_dev(ctypes.c_uint64(bases.handle), offset, ctypes.c_void_p(coeffs.data_ptr()), n,
                                               ctypes.c_void_p(_stream_ptr(coeffs)), _ptr(out)))
            return out
        c = _np(coeffs, 4, "coeffs")
        xy = np.zeros(8, dtype=np.uint64)
        is_id = ctypes.c_int(0)
        _lib.check(lib.hm_msm_bn256_g1_h(ctypes.c_uint64(bases.handle), offset, _ptr(c), c.shape[0], _ptr(xy),
                                         ctypes.byref(is_id)))
        if not is_id.value:
            out[:8] = xy
            out[8:] = FQ_ONE_MONT
        return out
    if _is_tensor(coeffs) or _is_tensor(bases):
        if not (_is_tensor(coeffs) and _is_tensor(bases)):
            raise TypeError("coeffs and bases must both be host arrays or both be GPU tensors")
        n = _tensor_rows(coeffs, 4, "coeffs")
        if n != _tensor_rows(bases, 8, "bases"):
            raise ValueError("best_multiexp: coeffs.len() != bases.len()")
        h = register_bases(bases, plain=True)
        try:
            return best_multiexp(coeffs, h)
        finally:
            release_bases(h)
    c, b = _np(coeffs, 4, "coeffs"), _np(bases, 8, "bases")
    if c.shape[0] != b.shape[0]:
        raise ValueError("best_multiexp: coeffs.len() != bases.len()")  # upstream: assert_eq! panic
    _lib.check(lib.hm_msm_bn256_g1_jacobian(_ptr(c), _ptr(b), c.shape[0], _ptr(out)))
    return out


def best_multiexp_submit(coeffs, bases: BasesHandle, offset: int = 0) -> int:
    """Asynchronous best_multiexp on device-resident scalars: enqueues the whole MSM on torch's current
    stream and returns a ticket at once (at most 8 in flight); pair with :func:`best_multiexp_wait`."""
    n = _tensor_rows(coeffs, 4, "coeffs")
    t = ctypes.c_uint64(0)
    _lib.check(_lib.load().hm_msm_submit_dev(ctypes.c_uint64(bases.handle), offset, ctypes.c_void_p(coeffs.data_ptr()), n,
                                             ctypes.c_void_p(_stream_ptr(coeffs)), ctypes.byref(t)))
    return t.value


def best_multiexp_batch(columns, bases: BasesHandle, offset: int = 0) -> np.ndarray:
    """The commitments of one prover phase in one call: ``columns`` is a list of (n, 4) GPU tensors (or one (count, n, 4)
    tensor); returns (count, 12) words.  Eight MSMs are kept in flight inside the library."""
    cols = [columns[i] for i in range(columns.shape[0])] if _is_tensor(columns) and columns.dim() == 3 else list(columns)
    out = np.zeros((len(cols), 12), dtype=np.uint64)
    if not cols:
        return out
    if not _is_tensor(cols[0]):                      # host arrays: uploads pipelined behind the other commitments' kernels
        host = [_np(c, 4, "columns") for c in cols]
        n = host[0].shape[0]
        if any(c.shape[0] != n for c in host):
            raise ValueError("best_multiexp_batch: every column must have the same length")
        ptrs = (ctypes.c_void_p * len(host))(*[c.ctypes.data for c in host])
        _lib.check(_lib.load().hm_msm_batch_bn256_g1_h(ctypes.c_uint64(bases.handle), offset, ptrs, n, len(host), _ptr(out)))
        return out
    n = _tensor_rows(cols[0], 4, "columns")
    for c in cols:
        if _tensor_rows(c, 4, "columns") != n:
            raise ValueError("best_multiexp_batch: every column must have the same length")
    ptrs = _ptr_array(cols)
    _lib.check(_lib.load().hm_msm_batch_bn256_g1_dev(ctypes.c_uint64(bases.handle), offset, ptrs, n, len(cols),
                                                     ctypes.c_void_p(_stream_ptr(cols[0])), _ptr(out)))
    return out


def best_multiexp_wait(ticket: int) -> np.ndarray:
    out = np.zeros(12, dtype=np.uint64)
    _lib.check(_lib.load().hm_msm_wait(ctypes.c_uint64(ticket), _ptr(out)))
    return out


def best_fft(a, omega, log_n: int) -> None:
    """In place: a[j] <- sum_i a[i] omega^(ij); natural order, unscaled."""
    lib = _lib.load()
    w = _np(omega, 4, "omega")
    if w.shape[0] != 1:
        raise ValueError("omega must be one field element")
    if _is_tensor(a):
        n = _tensor_rows(a, 4, "a")
        if n != 1 << log_n:
            raise ValueError("best_fft: a.len() != 1 << log_n")
        _lib.check(lib.hm_ntt_bn256_fr_dev(ctypes.c_void_p(a.data_ptr()), _ptr(w), log_n, ctypes.c_void_p(_stream_ptr(a))))
        return
    if not isinstance(a, np.ndarray):
        raise TypeError("best_fft transforms in place: pass a numpy array or a GPU tensor")
    arr = _np(a, 4, "a", writable=True)
    if arr.shape[0] != 1 << log_n:
        raise ValueError("best_fft: a.len() != 1 << log_n")  # upstream: assert_eq! panic
    _lib.check(lib.hm_ntt_bn256_fr(_ptr(arr), _ptr(w), log_n))


def eval_polynomial(polys, points, poly_index=None) -> np.ndarray:
    """``halo2_proofs::arithmetic::eval_polynomial`` for device-resident coefficient arrays: ``polys`` is a
    (n, 4) or (batch, n, 4) GPU tensor, ``points`` (q, 4) Montgomery words; query j evaluates polynomial
    ``poly_index[j]`` (default j) at ``points[j]``.  Returns (q, 4) words."""
    lib = _lib.load()
    if not _is_tensor(polys):
        raise TypeError("eval_polynomial: polys must be a GPU tensor (coefficients stay in HBM)")
    pts = _np(points, 4, "points")
    q = pts.shape[0]
    n = polys.shape[-2] if polys.dim() >= 2 else _tensor_rows(polys, 4, "polys")
    batch = _tensor_rows(polys, 4, "polys") // max(n, 1) if n else 0
    idx = None
    if poly_index is not None:
        idx = np.ascontiguousarray(poly_index, dtype=np.uint32)
        if idx.shape[0] != q or (q and int(idx.max()) >= batch):
            raise ValueError("eval_polynomial: poly_index must name one existing polynomial per point")
    elif q > batch:
        raise ValueError("eval_polynomial: more points than polynomials (pass poly_index)")
    out = np.zeros((q, 4), dtype=np.uint64)
    _lib.check(lib.hm_eval_polynomial_bn256_fr_dev(
        ctypes.c_void_p(polys.data_ptr()), n, idx.ctypes.data_as(_u32p) if idx is not None else None,
        _ptr(pts), q, _ptr(out), ctypes.c_void_p(_stream_ptr(polys))))
    return out


def kate_division(poly, z):
    """``halo2_proofs::arithmetic::kate_division``: the quotient of ``poly(X) - poly(z)`` by ``X - z`` for a
    device-resident coefficient tensor (n, 4); returns a new (n - 1, 4) GPU tensor."""
    import torch

    lib = _lib.load()
    if not _is_tensor(poly):
        raise TypeError("kate_division: poly must be a GPU tensor (coefficients stay in HBM)")
    n = _tensor_rows(poly, 4, "poly")
    if n == 0:
        raise ValueError("kate_division: empty polynomial")        # upstream: a.len() - 1 underflows and panics
    out = torch.empty((n - 1, 4), dtype=torch.int64, device=poly.device)
    zz = _np(z, 4, "z").reshape(4)
    _lib.check(lib.hm_kate_division_bn256_fr_dev(ctypes.c_void_p(poly.data_ptr()), n, _ptr(zz), ctypes.c_void_p(out.data_ptr()),
                                                 ctypes.c_void_p(_stream_ptr(poly))))
    return out


def grand_product(factors, start, out=None):
    """The running product of the permutation / lookup arguments: ``out[0] = start``, ``out[i] = out[i-1] *
    factors[i-1]`` for a device-resident (n, 4) tensor; ``out`` may be ``factors`` itself."""
    import torch

    lib = _lib.load()
    if not _is_tensor(factors):
        raise TypeError("grand_product: factors must be a GPU tensor")
    n = _tensor_rows(factors, 4, "factors")
    if out is None:
        out = torch.empty((n, 4), dtype=torch.int64, device=factors.device)
    elif _tensor_rows(out, 4, "out") != n:
        raise ValueError("grand_product: out and factors differ in length")
    st = _np(start, 4, "start").reshape(4)
    _lib.check(lib.hm_fr_grand_product_dev(ctypes.c_void_p(factors.data_ptr()), n, _ptr(st), ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(_stream_ptr(factors))))
    return out


def kate_division_batch(polys, zs):
    """``kate_division`` of several same-length device-resident polynomials, each by its own point, in one launch chain
    (the quotients of one multiopen round are independent of each other).  polys: list of (n, 4) GPU tensors; zs: one
    point per polynomial.  Returns the list of (n - 1, 4) quotient tensors -- the same words as ``kate_division`` gives
    one by one."""
    import torch

    lib = _lib.load()
    polys = list(polys)
    if not polys:
        return []
    if not all(_is_tensor(p) for p in polys):
        raise TypeError("kate_division_batch: polys must be GPU tensors (coefficients stay in HBM)")
    n = _tensor_rows(polys[0], 4, "polys[0]")
    if n == 0:
        raise ValueError("kate_division_batch: empty polynomial")
    if any(_tensor_rows(p, 4, "polys") != n for p in polys):
        raise ValueError("kate_division_batch: polynomials differ in length")
    zz = np.ascontiguousarray(np.stack([_np(z, 4, "z").reshape(4) for z in zs]))
    if zz.shape[0] != len(polys):
        raise ValueError("kate_division_batch: one point per polynomial")
    outs = [torch.empty((n - 1, 4), dtype=torch.int64, device=polys[0].device) for _ in polys]
    _lib.check(lib.hm_kate_division_batch_bn256_fr_dev(_ptr_array(polys), n, _ptr(zz), _ptr_array(outs), len(polys),
                                                       ctypes.c_void_p(_stream_ptr(polys[0]))))
    return outs


def grand_product_batch(factors, start, chain_row=None, outs=None):
    """The z columns of one argument in one launch chain.  factors: list of (n, 4) GPU tensors.  ``chain_row=None``: every
    column starts from ``start`` (the lookup arguments).  ``chain_row=u``: column j + 1 starts from ``out[j][u]`` --
    upstream's ``last_z`` of the permutation argument, u = n - (blinding_factors + 1) -- without reading anything back.
    ``outs[j]`` may be ``factors[j]`` itself.  Returns the list of outputs."""
    import torch

    lib = _lib.load()
    factors = list(factors)
    if not factors:
        return []
    if not all(_is_tensor(f) for f in factors):
        raise TypeError("grand_product_batch: factors must be GPU tensors")
    n = _tensor_rows(factors[0], 4, "factors[0]")
    if any(_tensor_rows(f, 4, "factors") != n for f in factors):
        raise ValueError("grand_product_batch: columns differ in length")
    if outs is None:
        outs = [torch.empty((n, 4), dtype=torch.int64, device=factors[0].device) for _ in factors]
    elif len(outs) != len(factors) or any(_tensor_rows(o, 4, "outs") != n for o in outs):
        raise ValueError("grand_product_batch: outs and factors differ in shape")
    if chain_row is not None and not 0 <= chain_row < n:
        raise ValueError("grand_product_batch: chain_row outside the columns")
    st = _np(start, 4, "start").reshape(4)
    _lib.check(lib.hm_fr_grand_product_batch_dev(_ptr_array(factors), n, _ptr(st), _lib.NO_CHAIN if chain_row is None else chain_row,
                                                 _ptr_array(outs), len(factors), ctypes.c_void_p(_stream_ptr(factors[0]))))
    return outs


def batch_invert(values):
    """``ff::BatchInvert::batch_invert`` in place on a device-resident (n, 4) tensor: zero stays zero."""
    lib = _lib.load()
    if not _is_tensor(values):
        raise TypeError("batch_invert: values must be a GPU tensor")
    n = _tensor_rows(values, 4, "values")
    _lib.check(lib.hm_fr_batch_invert_dev(ctypes.c_void_p(values.data_ptr()), n, ctypes.c_void_p(_stream_ptr(values))))
    return values


def linear_combination(polys, coeffs, out=None):
    """``sum_j coeffs[j] * polys[j]`` (upstream ``Polynomial * scalar`` and ``+``) for a list of device-resident
    (n, 4) tensors; ``out`` may be one of them."""
    import torch

    lib = _lib.load()
    polys = list(polys)
    cs = _np(coeffs, 4, "coeffs") if len(polys) else np.zeros((0, 4), dtype=np.uint64)
    if cs.shape[0] != len(polys):
        raise ValueError("linear_combination: one coefficient per polynomial")
    if not polys and out is None:
        raise ValueError("linear_combination: nothing to combine and no output to clear")
    n = _tensor_rows(polys[0] if polys else out, 4, "polys")
    for p in polys:
        if not _is_tensor(p) or _tensor_rows(p, 4, "polys") != n:
            raise ValueError("linear_combination: polynomials must be GPU tensors of one length")
    ref = polys[0] if polys else out
    if out is None:
        out = torch.empty((n, 4), dtype=torch.int64, device=ref.device)
    elif _tensor_rows(out, 4, "out") != n:
        raise ValueError("linear_combination: out differs in length")
    ptrs = (ctypes.c_void_p * max(len(polys), 1))(*[p.data_ptr() for p in polys])
    _lib.check(lib.hm_fr_linear_combination_dev(ptrs, _ptr(cs) if len(polys) else None, len(polys), n, ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(_stream_ptr(ref))))
    return out


def linear_combination_batch(polys, coeffs, outs=None):
    """``linear_combination`` for a batch of independent proofs in one launch chain (``hm_fr_linear_combination_batch_dev``):
    ``polys[b]`` the list of proof b's (n, 4) GPU tensors -- the same count for every proof, the same tensor allowed in several proofs
    -- ``coeffs[b]`` its integers; ``outs[b]`` may be one of proof b's own inputs, never another proof's input or output.  Returns
    the list of outputs (new tensors when ``outs`` is None), word for word the loop of ``linear_combination``."""
    import torch

    polys = [list(p) for p in polys]
    proofs = len(polys)
    if proofs == 0:
        return []
    count = len(polys[0])
    if any(len(p) != count for p in polys) or len(coeffs) != proofs or any(len(c) != count for c in coeffs):
        raise ValueError("linear_combination_batch: every proof needs the same number of polynomials and one coefficient for each")
    if count == 0 and outs is None:
        raise ValueError("linear_combination_batch: nothing to combine and no output to clear")
    ref = polys[0][0] if count else outs[0]
    n = _tensor_rows(ref, 4, "polys")
    for p in (q for row in polys for q in row):
        if not _is_tensor(p) or _tensor_rows(p, 4, "polys") != n:
            raise ValueError("linear_combination_batch: polynomials must be GPU tensors of one length")
    if outs is None:
        outs = list(torch.empty((proofs, n, 4), dtype=torch.int64, device=ref.device))
    elif len(outs) != proofs or any(not _is_tensor(o) or _tensor_rows(o, 4, "outs") != n for o in outs):
        raise ValueError("linear_combination_batch: one output of the polynomials' length per proof")
    flat = [p for row in polys for p in row]
    cs = fr_array([int(c) % FR_MODULUS for row in coeffs for c in row]) if count else None
    ptrs = (ctypes.c_void_p * max(len(flat), 1))(*[p.data_ptr() for p in flat])
    _lib.check(_lib.load().hm_fr_linear_combination_batch_dev(ptrs, _ptr(cs) if count else None, count, n, _ptr_array(list(outs)), proofs,
                                                              ctypes.c_void_p(_stream_ptr(ref))))
    return list(outs)


def permute_expression_pair(input_column, table_column, usable_rows: int, blinding_seed: int = 0):
    """``plonk::lookup::prover::permute_expression_pair``: the sorted input column and the arranged table column of one
    lookup argument, from device-resident (n, 4) columns.  Rows [usable_rows, n) -- upstream's random blinding rows --
    are drawn on the device from ``blinding_seed``.  Raises ``Halo2Mi355xError`` (code NOT_FOUND) when an input value is
    missing from the table (upstream: ``Error::ConstraintSystemFailure``)."""
    import torch

    lib = _lib.load()
    if not (_is_tensor(input_column) and _is_tensor(table_column)):
        raise TypeError("permute_expression_pair: columns must be GPU tensors")
    n = _tensor_rows(input_column, 4, "input_column")
    if _tensor_rows(table_column, 4, "table_column") != n:
        raise ValueError("permute_expression_pair: columns differ in length")
    if not 0 <= usable_rows <= n:
        raise ValueError("permute_expression_pair: usable_rows out of range")
    out_a = torch.empty((n, 4), dtype=torch.int64, device=input_column.device)
    out_s = torch.empty((n, 4), dtype=torch.int64, device=input_column.device)
    st = ctypes.c_void_p(_stream_ptr(input_column))
    _lib.check(lib.hm_lookup_permute_bn256_fr_dev(ctypes.c_void_p(input_column.data_ptr()), ctypes.c_void_p(table_column.data_ptr()),
                                                  usable_rows, ctypes.c_void_p(out_a.data_ptr()), ctypes.c_void_p(out_s.data_ptr()), st))
    tail = n - usable_rows
    if tail:
        _lib.check(lib.hm_fr_random_dev(ctypes.c_void_p(out_a.data_ptr() + usable_rows * 32), tail, ctypes.c_uint64(blinding_seed), st))
        _lib.check(lib.hm_fr_random_dev(ctypes.c_void_p(out_s.data_ptr() + usable_rows * 32), tail,
                                        ctypes.c_uint64(blinding_seed ^ 0x9E3779B97F4A7C15), st))
    return out_a, out_s


def permute_expression_pairs(input_columns, table_columns, usable_rows: int, blinding_seed: int = 0, blinding_seeds=None):
    """``permute_expression_pair`` for all lookup arguments of a circuit in one call (their sorts run side by side on the
    device).  Returns a list of (permuted_input, permuted_table) tensors.  A lookup whose input holds a value its table
    lacks raises ``Halo2Mi355xError`` (NOT_FOUND) carrying the indices in ``.missing``.  Pair i draws its blinding rows from
    ``blinding_seed + 2 i`` and ``+ 2 i + 1``; ``blinding_seeds`` (one per pair) names the first of the two instead -- the
    lookups of several circuits in one call, each circuit with its own seed."""
    import torch

    lib = _lib.load()
    ins, tabs = list(input_columns), list(table_columns)
    if len(ins) != len(tabs):
        raise ValueError("permute_expression_pairs: one table per input")
    if not ins:
        return []
    n = _tensor_rows(ins[0], 4, "input_columns")
    for c in ins + tabs:
        if not _is_tensor(c) or _tensor_rows(c, 4, "columns") != n:
            raise ValueError("permute_expression_pairs: columns must be GPU tensors of one length")
    if not 0 <= usable_rows <= n:
        raise ValueError("permute_expression_pairs: usable_rows out of range")
    seeds = [blinding_seed + 2 * i for i in range(len(ins))] if blinding_seeds is None else [int(v) for v in blinding_seeds]
    if len(seeds) != len(ins):
        raise ValueError("permute_expression_pairs: one blinding seed per pair")
    outs = [(torch.empty((n, 4), dtype=torch.int64, device=ins[0].device), torch.empty((n, 4), dtype=torch.int64, device=ins[0].device))
            for _ in ins]
    arr = _ptr_array
    missing = (ctypes.c_int * len(ins))()
    st = ctypes.c_void_p(_stream_ptr(ins[0]))
    rc = lib.hm_lookup_permute_batch_bn256_fr_dev(arr(ins), arr(tabs), len(ins), usable_rows, arr([o[0] for o in outs]),
                                                  arr([o[1] for o in outs]), missing, st)
    if rc != _lib.HM_OK:
        err = _lib.Halo2Mi355xError(rc, lib.hm_last_error().decode())
        err.missing = [i for i in range(len(ins)) if missing[i]]
        raise err
    tail = n - usable_rows
    if tail:
        for i, (oa, os_) in enumerate(outs):
            _lib.check(lib.hm_fr_random_dev(ctypes.c_void_p(oa.data_ptr() + usable_rows * 32), tail, ctypes.c_uint64(seeds[i] & 0xFFFFFFFFFFFFFFFF), st))
            _lib.check(lib.hm_fr_random_dev(ctypes.c_void_p(os_.data_ptr() + usable_rows * 32), tail,
                                            ctypes.c_uint64(((seeds[i] + 1) ^ 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF), st))
    return outs


LOGUP_COUNT_BITS = 20              # csrc/logup.inc LU_COUNT_BITS: table keys below 2^this are counted in value bins, nothing is sorted


def logup_multiplicities(table_columns, input_columns, usable_rows: int, outs=None):
    """The multiplicity columns of logUp arguments (``hm_logup_multiplicities_bn256_fr_dev``), all in one call:
    ``table_columns[a]`` the compressed table of argument a, ``input_columns[a]`` the list of its compressed inputs, all (n, 4) GPU
    tensors of which rows [0, usable_rows) are read.  -> one (n, 4) tensor per argument: on row i < usable_rows the number of
    (input, row) pairs holding the table's value of row i if i is the first row holding it, else 0; rows from ``usable_rows`` on are
    zero (the caller's blinding).  An input value its table lacks raises ``Halo2Mi355xError`` (NOT_FOUND) carrying the arguments'
    indices in ``.missing``."""
    import torch

    lib = _lib.load()
    tabs, ins = list(table_columns), [list(c) for c in input_columns]
    if len(tabs) != len(ins):
        raise ValueError("logup_multiplicities: one list of inputs per table")
    if not tabs:
        return []
    n = _tensor_rows(tabs[0], 4, "table_columns")
    for c in tabs + [c for row in ins for c in row]:
        if not _is_tensor(c) or _tensor_rows(c, 4, "columns") != n:
            raise ValueError("logup_multiplicities: columns must be GPU tensors of one length")
    if not 1 <= usable_rows <= n:
        raise ValueError("logup_multiplicities: usable_rows out of range")
    if any(not row for row in ins):
        raise ValueError("logup_multiplicities: an argument without inputs")
    if outs is None:
        outs = list(torch.zeros((len(tabs), n, 4), dtype=torch.int64, device=tabs[0].device))
    elif len(outs) != len(tabs) or any(not _is_tensor(o) or _tensor_rows(o, 4, "outs") != n for o in outs):
        raise ValueError("logup_multiplicities: one output of the columns' length per argument")
    counts = (ctypes.c_uint32 * len(tabs))(*[len(row) for row in ins])
    missing = (ctypes.c_int * len(tabs))()
    rc = lib.hm_logup_multiplicities_bn256_fr_dev(_ptr_array(tabs), _ptr_array([c for row in ins for c in row]), counts, len(tabs), usable_rows,
                                                  _ptr_array(list(outs)), missing, ctypes.c_void_p(_stream_ptr(tabs[0])))
    if rc != _lib.HM_OK:
        err = _lib.Halo2Mi355xError(rc, lib.hm_last_error().decode())
        err.missing = [i for i in range(len(tabs)) if missing[i]]
        raise err
    return list(outs)


def grand_sum_batch(terms, outs=None):
    """The running sums of logUp arguments (``hm_fr_grand_sum_batch_dev``): for every (n, 4) GPU tensor of ``terms``
    out[i] = sum_{j < i} terms[j] mod r -- exclusive, out[0] = 0 -- in one launch chain.  ``outs[j]`` may be ``terms[j]`` itself.
    Returns the list of outputs."""
    import torch

    terms = list(terms)
    if not terms:
        return []
    if not all(_is_tensor(t) for t in terms):
        raise TypeError("grand_sum_batch: terms must be GPU tensors")
    n = _tensor_rows(terms[0], 4, "terms[0]")
    if any(_tensor_rows(t, 4, "terms") != n for t in terms):
        raise ValueError("grand_sum_batch: columns differ in length")
    if outs is None:
        outs = [torch.empty((n, 4), dtype=torch.int64, device=terms[0].device) for _ in terms]
    elif len(outs) != len(terms) or any(_tensor_rows(o, 4, "outs") != n for o in outs):
        raise ValueError("grand_sum_batch: outs and terms differ in shape")
    _lib.check(_lib.load().hm_fr_grand_sum_batch_dev(_ptr_array(terms), n, _ptr_array(list(outs)), len(terms), ctypes.c_void_p(_stream_ptr(terms[0]))))
    return list(outs)


def g1_fixed_base_mul(scalars, base_xy: np.ndarray):
    """out[i] = [scalars[i]] * base, affine (ParamsKZG::setup's per-row G1 work).  GPU tensors only."""
    import torch

    lib = _lib.load()
    n = _tensor_rows(scalars, 4, "scalars")
    out = torch.empty((n, 8), dtype=torch.int64, device=scalars.device)
    b = _np(base_xy, 8, "base")
    _lib.check(lib.hm_g1_fixed_base_mul_dev(ctypes.c_void_p(scalars.data_ptr()), n, _ptr(b), ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(_stream_ptr(scalars))))
    return out


def _fr_one(value, name: str) -> np.ndarray:
    w = _np(value, 4, name)
    if w.shape[0] != 1:
        raise ValueError(f"{name} must be one field element")
    return w


def g1_fft(points, omega, log_n: int, scale=None) -> None:
    """``best_fft::<G1>`` on a GPU tensor of (n, 8) affine Montgomery words ((0, 0) = identity), in place:
    a[i] <- sum_j [omega^(ij)] a[j], then a[i] <- [scale] a[i] when ``scale`` is given.  n = 2^log_n <= 2^24."""
    w = _fr_one(omega, "omega")
    sc = None if scale is None else _fr_one(scale, "scale")
    if not _is_tensor(points):
        raise TypeError("g1_fft: a GPU tensor of (n, 8) words is expected (g1_fft_host takes numpy Jacobian arrays)")
    if _tensor_rows(points, 8, "points") != 1 << log_n:
        raise ValueError("g1_fft: points.len() != 1 << log_n")
    _lib.check(_lib.load().hm_g1_fft_bn256_dev(ctypes.c_void_p(points.data_ptr()), _ptr(w), log_n, None if sc is None else _ptr(sc),
                                               ctypes.c_void_p(_stream_ptr(points))))


def g1_fft_host(xyz: np.ndarray, omega, log_n: int, scale=None) -> None:
    """The drop-in's form (``hm_g1_fft_bn256``): a numpy (n, 12) Jacobian array as bn256::G1 lays it out (z = 0: identity), in
    place; outputs come back as (x, y, 1) / all zero."""
    w = _fr_one(omega, "omega")
    sc = None if scale is None else _fr_one(scale, "scale")
    if not isinstance(xyz, np.ndarray):
        raise TypeError("g1_fft_host transforms in place: pass a numpy array")
    arr = _np(xyz, 12, "xyz", writable=True)
    if arr.shape[0] != 1 << log_n:
        raise ValueError("g1_fft_host: xyz.len() != 1 << log_n")
    _lib.check(_lib.load().hm_g1_fft_bn256(_ptr(arr), _ptr(w), log_n, None if sc is None else _ptr(sc)))


def g_to_lagrange(g, k: int):
    """``halo2_proofs::arithmetic::g_to_lagrange``: the Lagrange basis [L_i(s)]G1 from the monomial points g[i] = [s^i]G1 (a (2^k, 8)
    GPU tensor), as a new tensor.  omega^-1 = ROOT_OF_UNITY_INV squared S - k times, n^-1 = TWO_INV^k, as upstream computes them."""
    r = FR_MODULUS
    omega_inv = pow(FR_ROOT_OF_UNITY, -1, r)
    for _ in range(k, FR_S):
        omega_inv = omega_inv * omega_inv % r
    n_inv = pow(pow(2, -1, r), k, r)
    out = g.clone()
    g1_fft(out, fr_words(omega_inv), k, fr_words(n_inv))
    return out


# ---- SRS point encodings (ParamsKZG.read / write) ----------------------------------------------------------
HM_ERR_INVALID_DATA = _lib.HM_ERR_INVALID_DATA


class InvalidPointError(ValueError):
    """An encoding or point that does not decode to a curve point; ``index`` is the smallest such entry."""

    def __init__(self, message: str, index: int):
        super().__init__(message)
        self.index = index


def _codec_rc(rc: int, bad: ctypes.c_uint64, who: str) -> None:
    if rc == HM_ERR_INVALID_DATA:
        raise InvalidPointError(f"{who}: invalid point at index {bad.value}", bad.value)
    _lib.check(rc)


def _bytes_rows(t, name: str) -> int:
    if not t.is_cuda:
        raise ValueError(f"{name}: torch tensors must live on the GPU (the *_host forms take numpy arrays)")
    if t.element_size() != 1 or not t.is_contiguous() or t.numel() % 32:
        raise ValueError(f"{name}: need a contiguous uint8 tensor of 32-byte encodings")
    return t.numel() // 32


def g1_compress(points):
    """Compressed G1 encodings (32 bytes: canonical x little-endian, bit 7 of byte 31 = parity of y; zeros = identity) of a GPU
    tensor of (n, 8) affine Montgomery words ((0, 0) = identity), as a new (n, 32) uint8 tensor.  The points are not validated."""
    import torch

    if not _is_tensor(points):
        raise TypeError("g1_compress: a GPU tensor of (n, 8) words is expected (g1_compress_host takes numpy arrays)")
    n = _tensor_rows(points, 8, "points")
    out = torch.empty((n, 32), dtype=torch.uint8, device=points.device)
    _lib.check(_lib.load().hm_g1_compress_bn256_dev(ctypes.c_void_p(points.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                                    ctypes.c_void_p(_stream_ptr(points))))
    return out


def g1_decompress(data):
    """The inverse of ``g1_compress`` on a GPU uint8 tensor of n x 32 bytes: a new (n, 8) int64 tensor of affine Montgomery words.
    Raises ValueError naming the smallest index whose x is not canonical or not the x of a curve point."""
    import torch

    if not _is_tensor(data):
        raise TypeError("g1_decompress: a GPU uint8 tensor is expected (g1_decompress_host takes numpy arrays)")
    n = _bytes_rows(data, "data")
    out = torch.empty((n, 8), dtype=torch.int64, device=data.device)
    bad = ctypes.c_uint64(0)
    rc = _lib.load().hm_g1_decompress_bn256_dev(ctypes.c_void_p(data.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), ctypes.byref(bad),
                                                ctypes.c_void_p(_stream_ptr(data)))
    _codec_rc(rc, bad, "g1_decompress")
    return out


def g1_check(points) -> None:
    """``SerdeFormat::RawBytes``' validation of a GPU tensor of (n, 8) affine Montgomery words: every word < p and every point on
    y^2 = x^3 + 3 or (0, 0).  Raises ValueError naming the smallest bad index."""
    if not _is_tensor(points):
        raise TypeError("g1_check: a GPU tensor of (n, 8) words is expected (g1_check_host takes numpy arrays)")
    n = _tensor_rows(points, 8, "points")
    bad = ctypes.c_uint64(0)
    rc = _lib.load().hm_g1_check_bn256_dev(ctypes.c_void_p(points.data_ptr()), n, ctypes.byref(bad), ctypes.c_void_p(_stream_ptr(points)))
    _codec_rc(rc, bad, "g1_check")


def _u8_rows(data, name: str) -> np.ndarray:
    arr = np.asarray(data)
    if arr.dtype != np.uint8:
        raise TypeError(f"{name} must be uint8 bytes, got {arr.dtype}")
    if arr.size % 32:
        raise ValueError(f"{name}: size is not a multiple of 32 bytes")
    return np.ascontiguousarray(arr).reshape(-1, 32)


def g1_compress_host(points: np.ndarray) -> np.ndarray:
    """``g1_compress`` on a numpy (n, 8) uint64 array through the host-pointer form: a new (n, 32) uint8 array."""
    if _is_tensor(points):
        raise TypeError("g1_compress_host takes numpy arrays (g1_compress takes GPU tensors)")
    p = _np(points, 8, "points")
    out = np.zeros((p.shape[0], 32), dtype=np.uint8)
    _lib.check(_lib.load().hm_g1_compress_bn256(_ptr(p), p.shape[0], out.ctypes.data_as(ctypes.c_void_p)))
    return out


def g1_decompress_host(data: np.ndarray) -> np.ndarray:
    """``g1_decompress`` on numpy bytes (n x 32 uint8): a new (n, 8) uint64 array."""
    if _is_tensor(data):
        raise TypeError("g1_decompress_host takes numpy arrays (g1_decompress takes GPU tensors)")
    d = _u8_rows(data, "data")
    out = np.zeros((d.shape[0], 8), dtype=np.uint64)
    bad = ctypes.c_uint64(0)
    rc = _lib.load().hm_g1_decompress_bn256(d.ctypes.data_as(ctypes.c_void_p), d.shape[0], _ptr(out), ctypes.byref(bad))
    _codec_rc(rc, bad, "g1_decompress")
    return out


def g1_check_host(points: np.ndarray) -> None:
    """``g1_check`` on a numpy (n, 8) uint64 array."""
    if _is_tensor(points):
        raise TypeError("g1_check_host takes numpy arrays (g1_check takes GPU tensors)")
    p = _np(points, 8, "points")
    bad = ctypes.c_uint64(0)
    _codec_rc(_lib.load().hm_g1_check_bn256(_ptr(p), p.shape[0], ctypes.byref(bad)), bad, "g1_check")


def random_fr(n: int, seed: int, device=None, shape=None):
    """``n`` field elements uniform over the WHOLE of [0, r) (``Fr::random``) as an (n, 4) int64 device tensor -- ``shape`` reshapes,
    e.g. (columns, rows, 4).  hm_fr_random_dev: one xoshiro256** stream per element seeded from (seed, index), 254-bit candidates
    rejected until one is below r.  (Masking the top four bits of random words instead covers only [0, 2^252), a third of the
    field, and never exercises the conditional subtractions near r: VERDICT r4, weak 3.)"""
    import torch

    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty((n, 4), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().hm_fr_random_dev(ctypes.c_void_p(out.data_ptr()), n, ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF),
                                                ctypes.c_void_p(_stream_ptr(out))))
    return out if shape is None else out.reshape(shape)


def msm_stats() -> dict:
    st = _lib.MsmStats()
    _lib.check(_lib.load().hm_get_msm_stats(ctypes.byref(st)))
    return {k: getattr(st, k) for k, _ in st._fields_}
