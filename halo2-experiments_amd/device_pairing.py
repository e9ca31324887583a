"""Pairing product checks on the GPU (``hm_pairing_check_bn256_dev``, csrc/pairing.inc): many independent checks
prod_i e(P_i, Q_i) == 1 in one launch chain -- one lane per pair for the Miller loops, one lane per check for the product and the
final exponentiation.  Points travel in ``pairing.py``'s integer forms (G1: (x, y), G2: ((x0, x1), (y0, y1)), ``None`` = the
identity) and the GT value comes back in its nesting, bit for bit the value ``pairing.final_exponentiation`` gives.

``pairing.py`` stays the oracle and the default of every verifier; ``check(pairs, pairing="device")`` is what their opt-in keyword
calls."""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _stream_ptr
from .bn256 import fq_array, fq_ints

_vp = ctypes.c_void_p
_u32p = ctypes.POINTER(ctypes.c_uint32)
MODES = ("host", "device")


def _marshal(checks):
    """-> g1 (n, 8) u64, g2 (n, 16) u64 Montgomery words, offsets (n_checks + 1) u32"""
    g1, g2, offsets = [], [], [0]
    for pairs in checks:
        for p, q in pairs:
            g1 += [0, 0] if p is None else [int(p[0]), int(p[1])]
            g2 += [0, 0, 0, 0] if q is None else [int(q[0][0]), int(q[0][1]), int(q[1][0]), int(q[1][1])]
        offsets.append(len(g1) // 2)
    n = offsets[-1]
    w1 = fq_array(g1).reshape(n, 8) if n else np.zeros((0, 8), dtype=np.uint64)
    w2 = fq_array(g2).reshape(n, 16) if n else np.zeros((0, 16), dtype=np.uint64)
    return w1, w2, np.asarray(offsets, dtype=np.uint32)


def run(checks, want_gt: bool = False):
    """One launch chain for all of ``checks`` -> (status list, GT words (n_checks, 48) or None).  status: 1 the product is 1, 0 it is
    not, 2 the check holds a point off its curve."""
    import torch

    checks = [list(pairs) for pairs in checks]
    if not checks:
        return [], (np.zeros((0, 48), dtype=np.uint64) if want_gt else None)
    w1, w2, offsets = _marshal(checks)
    n_pairs, n_checks = int(offsets[-1]), len(checks)
    dev = torch.device("cuda")
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)
    # one row stands in for the arrays of a call without pairs (every check empty): the entry takes no null pointer
    d_g1 = as_dev(w1 if n_pairs else np.zeros((1, 8), dtype=np.uint64))
    d_g2 = as_dev(w2 if n_pairs else np.zeros((1, 16), dtype=np.uint64))
    d_off = as_dev(offsets)
    lib = _lib.load()
    work_bytes = lib.hm_pairing_work_bytes(n_pairs, n_checks)
    if work_bytes == 0:
        raise ValueError("pairing checks: need 1 .. 2^20 checks and at most 2^24 pairs in one call")
    d_work = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device=dev)
    d_status = torch.empty(n_checks, dtype=torch.int32, device=dev)
    d_gt = torch.empty((n_checks, 48), dtype=torch.int64, device=dev) if want_gt else None
    _lib.check(lib.hm_pairing_check_bn256_dev(_vp(d_g1.data_ptr()), _vp(d_g2.data_ptr()), n_pairs, _dev_ptr(d_off, _u32p), n_checks,
                                              _vp(None if d_gt is None else d_gt.data_ptr()), _dev_ptr(d_status, _u32p),
                                              _vp(d_work.data_ptr()), work_bytes, _vp(_stream_ptr(d_work))))
    status = [int(s) for s in d_status.cpu().numpy()]
    gt = d_gt.cpu().numpy().view(np.uint64) if want_gt else None
    return status, gt


def run_device(d_g1, d_g2, d_offsets, n_checks: int):
    """The call of ``run`` on arrays that already lie on the device -- ``d_g1`` (n_pairs, 8) and ``d_g2`` (n_pairs, 16) int64 Montgomery
    words, ``d_offsets`` (n_checks + 1) int32 -- queued on the current stream: -> the (n_checks,) int32 status tensor, not downloaded
    (1 the product is 1, 0 it is not, 2 a point off its curve).  Nothing is marshalled and nothing waits.  The three tensors must be
    contiguous, of these dtypes and shapes, and on one device -- the raw pointers go to the library --; ValueError otherwise."""
    import torch

    for t, dtype, cols, name in ((d_g1, torch.int64, 8, "d_g1"), (d_g2, torch.int64, 16, "d_g2"), (d_offsets, torch.int32, None, "d_offsets")):
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.device == d_g1.device):
            raise ValueError(f"pairing checks: {name} must be a contiguous {dtype} tensor on the device of d_g1")
        if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
            raise ValueError(f"pairing checks: {name} must have the shape (n_pairs, {cols})")
    n_pairs, n_checks = int(d_g1.shape[0]), int(n_checks)
    if d_g2.shape[0] != n_pairs or d_offsets.dim() != 1 or d_offsets.numel() != n_checks + 1:
        raise ValueError("pairing checks: one G2 point per G1 point and n_checks + 1 offsets")
    if n_pairs == 0:
        raise ValueError("pairing checks: the arrays hold no pair (the entry takes no null pointer)")
    lib = _lib.load()
    work_bytes = lib.hm_pairing_work_bytes(n_pairs, n_checks)
    if work_bytes == 0:
        raise ValueError("pairing checks: need 1 .. 2^20 checks and at most 2^24 pairs in one call")
    d_work = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device=d_g1.device)
    d_status = torch.empty(n_checks, dtype=torch.int32, device=d_g1.device)
    _lib.check(lib.hm_pairing_check_bn256_dev(_vp(d_g1.data_ptr()), _vp(d_g2.data_ptr()), n_pairs, _dev_ptr(d_offsets, _u32p), n_checks,
                                              _vp(None), _dev_ptr(d_status, _u32p), _vp(d_work.data_ptr()), work_bytes,
                                              _vp(_stream_ptr(d_work))))
    return d_status


def _raise_on_malformed(status: Sequence[int]) -> None:
    bad = [c for c, s in enumerate(status) if s == 2]
    if bad:
        raise ValueError(f"pairing: a point is not on its curve (check {bad[0]})")


def pairing_checks(checks) -> List[bool]:
    """[prod_i e(P_i, Q_i) == 1 for pairs in checks], all in one launch chain; ValueError where ``pairing.pairing`` raises it"""
    status, _ = run(checks)
    _raise_on_malformed(status)
    return [s == 1 for s in status]


def pairing_check(pairs) -> bool:
    return pairing_checks([pairs])[0]


def pairing_values(checks) -> list:
    """the GT value of every check, in ``pairing.py``'s nesting ((a0, a1, a2), (b0, b1, b2)) of Fq2 pairs"""
    status, gt = run(checks, want_gt=True)
    _raise_on_malformed(status)
    out = []
    for row in gt:
        v = fq_ints(row.reshape(12, 4))
        two = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
        out.append((tuple(two[:3]), tuple(two[3:])))
    return out


def check(pairs, pairing: str = "host") -> bool:
    """``pairing.pairing_check(pairs)`` on the host integers or on the device: the same boolean (a point off its curve gives False)"""
    if pairing not in MODES:
        raise ValueError(f"pairing must be one of {MODES}, got {pairing!r}")
    if pairing == "host":
        from .pairing import pairing_check as host_check

        return host_check(pairs)
    status, _ = run([pairs])
    return status[0] == 1
