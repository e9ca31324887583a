"""What every wrapper of the C ABI does to its arguments before the call: numpy arrays and GPU tensors -> the pointers, row counts
and stream the entry points take (the ctypes types themselves are derived from the header in _lib.py)."""
from __future__ import annotations

import ctypes

import numpy as np

_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_vp = ctypes.c_void_p


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _np(a, cols: int, name: str, writable: bool = False) -> np.ndarray:
    arr = np.asarray(a)
    if arr.dtype != np.uint64:
        raise TypeError(f"{name} must be uint64 limbs, got {arr.dtype}")
    arr = arr.reshape(-1, cols)
    if not arr.flags["C_CONTIGUOUS"]:
        if writable:
            raise ValueError(f"{name} must be C-contiguous to be transformed in place")
        arr = np.ascontiguousarray(arr)
    return arr


def _ptr(arr: np.ndarray):
    return arr.ctypes.data_as(_u64p)


def _dev_ptr(t, ptr_type=_u64p):
    """The device pointer of a tensor as ``T*`` for the arguments the header types (``None``: the null pointer)."""
    return ctypes.cast(_vp(None if t is None else t.data_ptr()), ptr_type)


def _ptr_array(tensors):
    return (_vp * len(tensors))(*[t.data_ptr() for t in tensors])


def _stream_ptr(t) -> int:
    import torch

    return torch.cuda.current_stream(t.device).cuda_stream


def _tensor_rows(t, cols: int, name: str) -> int:
    if not t.is_cuda:
        raise ValueError(f"{name}: torch tensors must live on the GPU (pass numpy arrays for host data)")
    if t.element_size() != 8 or not t.is_contiguous():
        raise ValueError(f"{name}: need a contiguous 64-bit integer tensor")
    if t.numel() % cols:
        raise ValueError(f"{name}: size is not a multiple of {cols} words")
    return t.numel() // cols
