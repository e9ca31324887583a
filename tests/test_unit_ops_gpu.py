"""GPU suite: the device compile of csrc/ff29.h and csrc/g1.h, op by op on raw limbs (libhm_devcheck.so over csrc/unit_ops.h), against
Python integers (ff29_model.py) -- the same case tables and the same comparison as test_unit_ops_host.py: operands at the class
maxima, lazy limbs up to 2^31 - 1, column sums at the last admissible value, every exceptional branch of the addition laws under
every representative.  One launch per op; a few thousand lanes each."""
import ctypes
import os

import numpy as np
import pytest

import ff29_model as m
import unit_ops_cases as uc
from halo2_experiments_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    assert os.path.exists(_lib.DEVCHECK_PATH), f"{_lib.DEVCHECK_PATH} is missing: run __graft_entry__.build()"
    _lib.load()                                   # torch's HIP runtime first, as for the product library
    lib = ctypes.CDLL(_lib.DEVCHECK_PATH)
    lib.dc_field_ops.restype = lib.dc_curve_ops.restype = ctypes.c_int
    lib.dc_field_ops.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.dc_curve_ops.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def run_op(dc, table, op, ins, out_words):
    """one launch over the records of one op: (n, in words) uint32 -> (n, out words) uint32"""
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(ins).view(np.int32)).cuda()
    d_out = torch.zeros((ins.shape[0], out_words), dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if table == 2:
        rc = dc.dc_curve_ops(op, d_in.data_ptr(), d_out.data_ptr(), ins.shape[0], stream)
    else:
        rc = dc.dc_field_ops(table, op, d_in.data_ptr(), d_out.data_ptr(), ins.shape[0], stream)
    assert rc == _lib.HM_OK, rc
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("field", m.FIELDS, ids=lambda f: f.name)
def test_field_ops_match_the_model(dc, field):
    total = compared = 0
    for name, ins in uc.field_tables(field).items():
        outs = run_op(dc, field.index, uc.OPS[name], ins, uc.FIELD_OUT)
        compared += uc.check_field(field, name, ins, outs)
        total += ins.shape[0]
    assert compared == total and total > 0, "a generated case was not compared"


def test_curve_ops_match_the_model(dc):
    tables = uc.curve_tables()
    outs = {name: run_op(dc, 2, uc.OPS[name], ins, uc.CURVE_OUT) for name, (ins, _) in tables.items()}
    total = compared = 0
    for name, (ins, meta) in tables.items():
        compared += uc.check_curve(name, ins, meta, outs[name], outs)
        total += ins.shape[0]
    assert compared == total and total > 0, "a generated case was not compared"


def test_arguments_are_checked_before_any_launch(dc):
    import torch
    buf = torch.zeros(256, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    assert dc.dc_field_ops(2, 0, p, p, 1, None) == _lib.HM_ERR_BAD_ARG              # no such field
    assert dc.dc_field_ops(0, uc.OPS["UF_OP_END"], p, p, 1, None) == _lib.HM_ERR_BAD_ARG
    assert dc.dc_field_ops(0, 18, p, p, 1, None) == _lib.HM_ERR_BAD_ARG             # the gap in the numbering
    assert dc.dc_field_ops(0, 0, None, p, 1, None) == _lib.HM_ERR_BAD_ARG
    assert dc.dc_field_ops(0, 0, p, p + 4, 1, None) == _lib.HM_ERR_BAD_ARG          # not 16-byte aligned
    assert dc.dc_curve_ops(uc.OPS["UC_OP_END"], p, p, 1, None) == _lib.HM_ERR_BAD_ARG
    assert dc.dc_curve_ops(0, p + 8, p, 1, None) == _lib.HM_ERR_BAD_ARG
    assert dc.dc_curve_ops(0, p, None, 1, None) == _lib.HM_ERR_BAD_ARG
    assert dc.dc_curve_ops(0, p, p, 0, None) == _lib.HM_OK                          # nothing to do
