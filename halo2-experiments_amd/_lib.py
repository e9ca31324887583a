"""ctypes binding of libhalo2_mi355x.so (include/halo2_mi355x.h).  No torch types cross the ABI."""
from __future__ import annotations

import ctypes
import os
import subprocess

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# eight commitments in flight need more than the HIP runtime's default of 4 hardware queues (capi.hip sets the same
# default when the library is loaded; here it is set as early as the package import, before torch touches the GPU)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
LIB_PATH = os.environ.get("HALO2_MI355X_LIB") or os.path.join(CSRC, "libhalo2_mi355x.so")   # override: A/B builds
HOSTCHECK_PATH = os.path.join(CSRC, "libhm_hostcheck.so")
DEVCHECK_PATH = os.path.join(CSRC, "libhm_devcheck.so")      # test-only: csrc/unit_ops.h on the device (tests/test_unit_ops_gpu.py)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "halo2_mi355x.h")


class Halo2Mi355xError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libhalo2_mi355x error {code}: {message}")
        self.code = code


# ---- everything the header states, derived from it at import (no library load, no GPU) ----------------------------------------
with open(HEADER_PATH) as _f:
    _FUNCTIONS, _STRUCT_FIELDS, _DEFINES = _header.parse_header(_f.read())

_SCALARS = {"c_int": ctypes.c_int, "c_long": ctypes.c_long, "usize": ctypes.c_size_t, "u64": ctypes.c_uint64, "u32": ctypes.c_uint32,
            "i32": ctypes.c_int32, "u8": ctypes.c_uint8, "f64": ctypes.c_double, "c_char": ctypes.c_char}


_STRUCTS = {}           # canonical base type ('HmStats') -> the ctypes twin of that struct


def _struct(name: str, cname: str, **extra):
    """The ctypes twin of one of the header's structs: field names, order, types and array lengths as declared there."""
    fields = [(f, _SCALARS[base] * count if count else _SCALARS[base]) for f, base, count in _STRUCT_FIELDS[cname]]
    cls = type(name, (ctypes.Structure,), dict(extra, _fields_=fields, __doc__=f"{cname} (include/halo2_mi355x.h)"))
    _STRUCTS[_header.STRUCTS[cname]] = cls
    return cls


def _define(text: str) -> int:
    """'-4' -> -4; '(size_t)-1' -> the value as that type holds it"""
    cast, _, digits = text.rpartition(")")
    return _SCALARS[_header.C_SCALARS[cast[1:]]](int(digits)).value if cast else int(digits)


# every HM_* define is a module constant: HM_OK, HM_ERR_NOT_FOUND, HM_SHPLONK_MAX_POINTS, HM_GRAPH_COLUMNS_INTERNAL, HM_NO_CHAIN ...
globals().update({name: _define(text) for name, text in _DEFINES})
NO_CHAIN = HM_NO_CHAIN      # noqa: F821

MsmStats = _struct("MsmStats", "hm_msm_stats")
BasesInfo = _struct("BasesInfo", "hm_bases_info")
# hm_stats: per-call counters since start / hm_reset_stats; vector_calls[HM_STAT_x] and vector_elements[HM_STAT_x] belong to KINDS[x]
Stats = _struct("Stats", "hm_stats", KINDS=tuple(name[len("HM_STAT_"):].lower() for _, name in sorted(
    (_define(text), name) for name, text in _DEFINES if name.startswith("HM_STAT_"))))


def _ctype(canon: str):
    """The ctypes type of a canonical C type ('u64 c' = const uint64_t*, see _header.py) -- the one statement of the mapping:
    a scalar is its ctypes scalar; void* and uint8_t* (byte buffers have no word type) are c_void_p; char* is c_char_p; T* of a
    scalar or struct T is POINTER(T); any pointer to pointer (a table of addresses) is POINTER(c_void_p)."""
    base, *ptrs = canon.split()
    if not ptrs:
        return _SCALARS[base]
    if len(ptrs) > 1:
        return ctypes.POINTER(ctypes.c_void_p)
    if base in ("c_void", "u8"):
        return ctypes.c_void_p
    if base == "c_char":
        return ctypes.c_char_p
    return ctypes.POINTER(_SCALARS.get(base) or _STRUCTS[base])


_SIGNATURES = {name: (_ctype(ret), [_ctype(t) for t, _ in params]) for name, ret, params in _FUNCTIONS}


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into csrc/libhalo2_mi355x.so (in-tree) with hipcc."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True)
    subprocess.run(args, check=True)
    return LIB_PATH


_lib = None


def _bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Give every entry point of the header its restype and argtypes; a symbol the library lacks raises."""
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load() -> ctypes.CDLL:
    """Load the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the MSM/NTT path)")
        try:
            # torch bundles its own libamdhip64; if ours pulled /opt/rocm's copy in first, torch would
            # later load a second HIP runtime and see no device.  Load torch's first when it exists.
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


FI_LIB_PATH = os.path.join(CSRC, "libhalo2_mi355x_fi.so")
_fi = None


def load_fi() -> ctypes.CDLL:
    """The TEST build of the same sources with the fault points of the C-ABI barrier compiled in (csrc/Makefile:
    -DHM_FAULT_INJECTION) and hm_test_arm_fault(point, after) exported.  Used by tests/test_capi_faults.py only; a second,
    independent copy of the library in the process (its own contexts, its own handles)."""
    global _fi
    if _fi is None:
        load()                                   # torch's HIP runtime first, as for the product library
        lib = _bind(ctypes.CDLL(FI_LIB_PATH))
        lib.hm_test_arm_fault.restype = ctypes.c_int
        lib.hm_test_arm_fault.argtypes = [ctypes.c_char_p, ctypes.c_long]
        _fi = lib
    return _fi


def check(rc: int) -> None:
    if rc != HM_OK:      # noqa: F821
        raise Halo2Mi355xError(rc, load().hm_last_error().decode())
