"""GPU suite of hm_graph_evaluate_proofs_dev: ``CompiledGraph.evaluate_proofs`` -- several independent proofs,
each with its own per-call constants, columns and values, in one launch -- against the loop of ``CompiledGraph.evaluate`` calls it
replaces, word for word.  Shapes (log_size, segments, proofs): (4, 1, 5) a wave spans four proofs inside one partly filled workgroup;
(9, 2, 3); (6, 1, 1) the single entry; (12, 1, 81) 331 776 lanes, above the 1 280 x 256 of the grid cap, so the stride loop takes a
second trip.  Both column formats, shared and per-proof columns mixed and at strides of their own, PreviousValue chained through
two calls, a rotation at the last row of a proof, spot rows against oracle/graph_ref, and every argument error with the values
untouched."""
import ctypes
import random

import numpy as np
import pytest
import torch

import graph_circuits_common as gc
import graph_programs as gp
import halo2_experiments_amd as h
from halo2_experiments_amd import _lib
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words

pytestmark = pytest.mark.gpu

N_COLS = gp.NF + gp.NA + gp.NI
SHAPES = [(4, 1, 5), (9, 2, 3), (6, 1, 1), (12, 1, 81)]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def per_proof_constants() -> gp.Program:
    """Horner(PreviousValue, [a0(+1) * beta + ch0, f0(-1) * gamma - f2, i1(+3) * theta + ch1], y): every per-call constant is read, with
    rotations that wrap and the short column Fixed(2)"""
    b = gp.Builder("per_proof_constants", "hand-made: all six per-call constants")
    t0 = b.add(b.mul(gp._col("Advice", 0, 1), ("Beta",)), ("Challenge", 0))
    t1 = b.sub(b.mul(gp._col("Fixed", 0, -1), ("Gamma",)), gp._col("Fixed", 2, 0))
    t2 = b.add(b.mul(gp._col("Instance", 1, 3), ("Theta",)), ("Challenge", 1))
    b.horner(gp.PREV, [t0, t1, t2], ("Y",))
    return b.finish()


PROGRAMS = {"three_terms": gc.three_terms, "per_proof_constants": per_proof_constants, "random_7003": lambda: gp.random_program(7003)}


@pytest.fixture(scope="module", params=list(PROGRAMS))
def program(request):
    p = PROGRAMS[request.param]()
    prog = p.compile()
    yield p, prog
    prog.destroy()


@pytest.fixture(scope="module")
def constants_program():
    p = per_proof_constants()
    prog = p.compile()
    yield p, prog
    prog.destroy()


def scalars_for(rng, proofs):
    out = [dict(challenges=[rng.randrange(R) for _ in range(gp.NCH)], beta=rng.randrange(R), gamma=rng.randrange(R), theta=rng.randrange(R),
                y=rng.randrange(R)) for _ in range(proofs)]
    assert len({tuple(s["challenges"]) + (s["beta"], s["gamma"], s["theta"], s["y"]) for s in out}) == proofs
    return out


def random_inputs(seed, size, proofs, shared=()):
    """-> (columns, previous (proofs, size, 4), per-proof scalars): the short columns and those listed are (rows, 4), shared; the others
    (proofs, rows, 4)"""
    cols = []
    for i in range(N_COLS):
        rows = (1 << gp.SHORT[i]) if i in gp.SHORT else size
        if i in gp.SHORT or i in shared:
            cols.append(h.random_fr(rows, seed + i, "cuda"))
        else:
            cols.append(h.random_fr(proofs * rows, seed + i, "cuda", shape=(proofs, rows, 4)))
    return cols, h.random_fr(proofs * size, seed + 99, "cuda", shape=(proofs, size, 4)), scalars_for(random.Random(seed), proofs)


def loop_of_single_calls(prog, cols, values, scalars, internal, segments):
    """the loop evaluate_proofs replaces, in place on values[b]"""
    for b, sc in enumerate(scalars):
        prog.evaluate([c[b] if c.dim() == 3 else c for c in cols], values[b], columns_internal=internal, segments=segments, **sc)
    return values


@pytest.mark.parametrize("log_size,segments,proofs", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("internal", [False, True], ids=["external", "internal"])
def test_the_entry_equals_the_loop_of_single_evaluations(program, log_size, segments, proofs, internal):
    p, prog = program
    size = segments << log_size
    cols, prev, scalars = random_inputs(100 * log_size + proofs, size, proofs)
    want = loop_of_single_calls(prog, cols, prev.clone(), scalars, internal, segments)
    values = prev.clone()
    prog.evaluate_proofs(cols, values, scalars, columns_internal=internal, segments=segments)
    assert np.array_equal(host(values), host(want)), p.name
    assert not np.array_equal(host(values), host(prev))


def test_one_proof_equals_the_single_entry(constants_program):
    """(6, 1, 1) through the C entry with a values stride of 0: whatever the stride says, one proof is hm_graph_evaluate_segments_dev"""
    p, prog = constants_program
    cols, prev, scalars = random_inputs(61, 64, 1)
    want = loop_of_single_calls(prog, cols, prev.clone(), scalars, False, 1)
    values = prev.clone()
    sc = scalars[0]
    dyn = np.stack([fr_words(v) for v in sc["challenges"] + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]]])
    flat = [c[0] if c.dim() == 3 else (c if c.shape[0] > 1 else c.expand(2, 4).contiguous()) for c in cols]
    ptrs = (ctypes.c_void_p * N_COLS)(*[c.data_ptr() for c in flat])
    strides = (ctypes.c_uint64 * N_COLS)(*([0] * N_COLS))
    rc = _lib.load().hm_graph_evaluate_proofs_dev(ctypes.c_uint64(prog.handle), ptrs, strides, N_COLS, 1, dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                  dyn.shape[0], 6, 1, ctypes.c_void_p(values.data_ptr()), 0, 0, None)
    assert rc == _lib.HM_OK
    assert np.array_equal(host(values), host(want))


@pytest.mark.parametrize("internal", [False, True], ids=["external", "internal"])
def test_mixed_strides_with_shared_columns(program, internal):
    """Fixed(0) and Advice(1) shared (stride 0); Advice(0) a slice of a wider tensor, so that its stride is not its length; Instance(1)
    named by (proof 0's column, stride in words)"""
    p, prog = program
    size, proofs = 128, 4
    cols, prev, scalars = random_inputs(7, size, proofs, shared=(0, gp.NF + 1))
    wide = h.random_fr(proofs * 3 * size, 8, "cuda", shape=(proofs, 3, size, 4))
    cols[gp.NF] = wide[:, 1]
    want = loop_of_single_calls(prog, [c.contiguous() if c.dim() == 3 else c for c in cols], prev.clone(), scalars, internal, 2)
    given = list(cols)
    last = gp.NF + gp.NA + 1
    given[last] = (cols[last][0], size * 8)
    values = prev.clone()
    prog.evaluate_proofs(given, values, scalars, columns_internal=internal, segments=2)
    assert np.array_equal(host(values), host(want)), p.name


def test_values_inside_a_wider_tensor(constants_program):
    """the values of proof b at a stride larger than its rows: what lies between stays as it was"""
    p, prog = constants_program
    size, proofs = 16, 5
    cols, prev, scalars = random_inputs(17, size, proofs)
    want = loop_of_single_calls(prog, cols, prev.clone(), scalars, False, 1)
    wide = h.random_fr(proofs * 2 * size, 18, "cuda", shape=(proofs, 2 * size, 4))
    wide[:, :size] = prev
    before = host(wide).copy().reshape(proofs, 2 * size, 4)
    prog.evaluate_proofs(cols, wide[:, :size], scalars)
    after = host(wide).reshape(proofs, 2 * size, 4)
    assert np.array_equal(after[:, :size], host(want).reshape(proofs, size, 4))
    assert np.array_equal(after[:, size:], before[:, size:])


def test_previous_value_chains_through_two_calls(program):
    p, prog = program
    size, proofs = 1 << 9, 3
    cols, prev, scalars = random_inputs(23, size, proofs)
    second = scalars_for(random.Random(24), proofs)
    want = loop_of_single_calls(prog, cols, loop_of_single_calls(prog, cols, prev.clone(), scalars, False, 1), second, False, 1)
    values = prev.clone()
    prog.evaluate_proofs(cols, values, scalars)
    prog.evaluate_proofs(cols, values, second)
    assert np.array_equal(host(values), host(want)), p.name


def test_a_rotation_at_the_last_row_stays_inside_its_proof():
    """value = a0(+1) + a0: at the last row of proof b it reads proof b's FIRST row, not proof b + 1's"""
    b = gp.Builder("next_row")
    b.add(gp._col("Advice", 0, 1), gp._col("Advice", 0, 0))
    p = b.finish()
    prog = p.compile()
    try:
        size, proofs = 16, 3
        rng = random.Random(5)
        a0 = [[rng.randrange(R) for _ in range(size)] for _ in range(proofs)]
        cols, prev, scalars = random_inputs(29, size, proofs)
        cols[gp.NF] = gp.to_device(gp.words([v for col in a0 for v in col])).reshape(proofs, size, 4)
        prog.evaluate_proofs(cols, prev, scalars)
        got = host(prev).reshape(proofs, size, 4)
        for q in range(proofs):
            assert np.array_equal(got[q, size - 1], gp.words([(a0[q][0] + a0[q][size - 1]) % R])[0]), q
            assert a0[q][0] != a0[(q + 1) % proofs][0]
            assert np.array_equal(got[q, 3], gp.words([(a0[q][4] + a0[q][3]) % R])[0])
    finally:
        prog.destroy()


def test_spot_rows_against_the_oracle(program):
    """one proof = one gp.Data with its own scalars and previous values: both ends and the middle of every proof by oracle/graph_ref"""
    p, prog = program
    seg, proofs = 16, 5
    rng = random.Random(31)
    data = [gp.make_data(rng, seg, 1) for _ in range(proofs)]
    for d in data[1:]:                                                       # the short columns are proof 0's for all
        d.table = [data[0].table[i] if i in gp.SHORT else c for i, c in enumerate(d.table)]
    rows = [0, 7, seg - 1]
    for internal in (False, True):
        cols = []
        for i in range(N_COLS):
            per = [gp.column_words(d, internal)[i] for d in data]
            cols.append(gp.to_device(per[0]) if i in gp.SHORT else gp.to_device(np.concatenate(per)).reshape(proofs, seg, 4))
        values = gp.to_device(gp.words([v for d in data for v in d.previous])).reshape(proofs, seg, 4)
        prog.evaluate_proofs(cols, values, [d.scalars() for d in data], columns_internal=internal)
        got = host(values).reshape(proofs, seg, 4)
        for q, d in enumerate(data):
            assert np.array_equal(got[q][rows], gp.words(gp.oracle_rows(p, d, rows))), (p.name, q, internal)


def test_argument_errors_launch_nothing(constants_program):
    p, prog = constants_program
    lib = _lib.load()
    fn = lib.hm_graph_evaluate_proofs_dev
    size, proofs = 64, 2
    cols, prev, scalars = random_inputs(41, size, proofs)
    flat = [c[0] if c.dim() == 3 else (c if c.shape[0] > 1 else c.expand(2, 4).contiguous()) for c in cols]
    strides = [size * 8 if c.dim() == 3 else 0 for c in cols]
    values = prev.clone()
    before = host(values).copy()                                             # the sentinel: whatever a refused call would overwrite
    dyn = np.stack([fr_words(v) for sc in scalars for v in sc["challenges"] + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]]])
    dynp = dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    n_dyn = dyn.shape[0] // proofs

    def call(handle=prog.handle, ptrs=None, strd=None, n_columns=N_COLS, count=proofs, dyn_ptr=dynp, n_dynamic=n_dyn, log_size=6, segments=1,
             vals=values.data_ptr(), vstride=size * 8, flags=0, null_columns=False, null_strides=False):
        ptrs = [t.data_ptr() for t in flat] if ptrs is None else ptrs
        strd = strides if strd is None else strd
        pa = None if null_columns else (ctypes.c_void_p * len(ptrs))(*ptrs)
        sa = None if null_strides else (ctypes.c_uint64 * len(strd))(*strd)
        rc = fn(ctypes.c_uint64(handle), pa, sa, n_columns, count, dyn_ptr, n_dynamic, log_size, segments, ctypes.c_void_p(vals), vstride, flags, None)
        assert np.array_equal(host(values), before), "the values changed"
        return rc

    BAD, NOT_FOUND = _lib.HM_ERR_BAD_ARG, _lib.HM_ERR_NOT_FOUND
    assert call(null_columns=True) == BAD and call(null_strides=True) == BAD and call(dyn_ptr=None) == BAD and call(vals=None) == BAD
    assert call(count=0) == BAD                                                                           # proofs == 0
    assert call(vstride=size * 8 - 4) == BAD and call(vstride=0) == BAD                                   # below the rows of one proof
    assert call(vstride=size * 8 + 2) == BAD                                                              # off 4 words
    assert call(ptrs=[flat[0].data_ptr()] * 257, strd=[0] * 257, n_columns=257) == BAD                     # > GE_MAX_COLUMNS
    assert call(ptrs=[flat[0].data_ptr() + 8] + [t.data_ptr() for t in flat[1:]]) == BAD                  # a base off 16 bytes
    assert call(vals=values.data_ptr() + 8) == BAD
    odd = list(strides)
    odd[gp.NF] = size * 8 + 2
    assert call(strd=odd) == BAD                                                                          # a stride off 4 words
    assert call(count=(1 << 32) // 64 + 1) == BAD                                                         # proofs * rows > 2^32
    assert call(ptrs=[t.data_ptr() for t in flat[:-1]], strd=strides[:-1], n_columns=N_COLS - 1) == BAD   # another column count
    assert call(n_dynamic=n_dyn - 1) == BAD                                                               # another constant count
    assert call(flags=2) == BAD and call(segments=0) == BAD and call(log_size=31) == BAD
    assert b"graph:" in lib.hm_last_error()
    assert call(handle=1 << 40) == NOT_FOUND
    with pytest.raises(ValueError, match="evaluate_proofs"):
        prog.evaluate_proofs(cols[:-1], values, scalars)
    with pytest.raises(ValueError, match="evaluate_proofs"):
        prog.evaluate_proofs(cols, values[0], scalars)
    with pytest.raises(ValueError, match="evaluate_proofs"):
        prog.evaluate_proofs(cols, values, scalars[:1])
    with pytest.raises(ValueError, match="evaluate_proofs"):
        prog.evaluate_proofs(cols, values, [dict(s, x=1) for s in scalars])
    assert np.array_equal(host(values), before)
    # the same arguments without a fault are accepted, and a program the circuits entry refuses is admitted here
    prog.evaluate_proofs(cols, values, scalars)
    assert not np.array_equal(host(values), before)
    other = gc.not_admitted()[0].compile()
    try:
        values2 = prev.clone()
        other.evaluate_proofs(cols, values2, scalars)
        assert np.array_equal(host(values2), host(loop_of_single_calls(other, cols, prev.clone(), scalars, False, 1)))
    finally:
        other.destroy()


def test_a_good_call_on_a_second_stream_follows_a_refused_one(constants_program):
    """64 rows, 2 proofs: a call refused on one stream leaves no stream slot behind it -- the same call without the fault, on another
    stream, gives what it gives on the default stream"""
    p, prog = constants_program
    size, proofs = 64, 2
    cols, prev, scalars = random_inputs(43, size, proofs)
    flat = [c[0] if c.dim() == 3 else (c if c.shape[0] > 1 else c.expand(2, 4).contiguous()) for c in cols]
    strides = [size * 8 if c.dim() == 3 else 0 for c in cols]
    dyn = np.stack([fr_words(v) for sc in scalars for v in sc["challenges"] + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]]])
    want = prev.clone()
    prog.evaluate_proofs(cols, want, scalars)
    values = prev.clone()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    good = [t.data_ptr() for t in flat]
    for ptrs, vals, vstride in (([good[0] + 8] + good[1:], values.data_ptr(), size * 8), (good, values.data_ptr() + 8, size * 8),
                                (good, values.data_ptr(), size * 8 - 4)):
        rc = _lib.load().hm_graph_evaluate_proofs_dev(
            ctypes.c_uint64(prog.handle), (ctypes.c_void_p * N_COLS)(*ptrs), (ctypes.c_uint64 * N_COLS)(*strides), N_COLS, proofs,
            dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dyn.shape[0] // proofs, 6, 1, ctypes.c_void_p(vals), vstride, 0,
            ctypes.c_void_p(sa.cuda_stream))
        assert rc == _lib.HM_ERR_BAD_ARG and b"graph:" in _lib.load().hm_last_error()
        sa.synchronize()
        assert np.array_equal(host(values), host(prev))
        again = prev.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(sb):
            prog.evaluate_proofs(cols, again, scalars)
        sb.synchronize()
        assert np.array_equal(host(again), host(want))
    assert not np.array_equal(host(want), host(prev))
