"""GPU suite: the programs of tests/graph_programs.py -- the shapes ``GraphEvaluator.add_expression`` never emits -- through
``CompiledGraph.evaluate`` on the device, external and internal columns, against oracle/graph_ref AND against the host replay of the
same lowered program (hc_graph_replay restates the kernel's switch; equality with the device word for word is what keeps the
restatement honest).  tests/test_graph_lowering_host.py holds the third side, host replay == oracle, for the same seeds."""
import random

import numpy as np
import pytest

import graph_programs as gp
from test_graph_lowering_host import HAND_SIZES, SWEEP_SEEDS, sweep_size

R = gp.R
DEVICE_SEEDS = list(SWEEP_SEEDS)[:72]            # a subset of the host sweep: the same seed is the same program, size and inputs
LANES = 1280 * 256                               # csrc/graph.hip: at most 1280 workgroups of 256 lanes


@pytest.fixture(scope="module")
def hc():
    return gp.hostcheck()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [p.name for p in gp.hand_written()])
def test_hand_written_program_on_device(hc, name):
    """1 x 1, 2 x 8 and 64 x 2 rows (1 row, and 2^7 rows: fewer than one workgroup), both formats, two chained calls."""
    p = next(q for q in gp.hand_written() if q.name == name)
    for i, (seg, segments) in enumerate(HAND_SIZES):
        d = gp.make_data(random.Random(100 + i), seg, segments)
        bad = gp.device_against_oracle_and_replay(hc, p, d, random.Random(900 + i))
        assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("first", DEVICE_SEEDS[::12])
def test_random_programs_on_device(hc, first):
    """Twelve seeds of the host sweep a case: every (segment, segments) combination once."""
    for seed in range(first, first + 12):
        p = gp.random_program(seed)
        seg, segments = sweep_size(seed, len(p.lower()["calcs"]))
        d = gp.make_data(random.Random(seed), seg, segments)
        bad = gp.device_against_oracle_and_replay(hc, p, d, random.Random(seed + 1))
        assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("seg,segments", [(1, 1), (64, 2), (128, 8), (1024, 1)])
@pytest.mark.parametrize("which", ["many_live_then_recycled", 7003, 7010])
def test_scratch_geometry_row_counts(hc, which, seg, segments):
    """The scratch layout [slot][word][lane] at 1, 2^7 and 2^10 rows (in one and in eight segments): the lane count, and with it the
    stride between a slot's words, follows the row count."""
    p = next(q for q in gp.hand_written() if q.name == which) if isinstance(which, str) else gp.random_program(which)
    d = gp.make_data(random.Random(seg * 31 + segments), seg, segments)
    bad = gp.device_against_oracle_and_replay(hc, p, d, random.Random(5))
    assert not bad, "\n".join(bad)


class _LazyColumn:
    """A column of the device as the oracle indexes it: words are converted to integers on demand."""

    def __init__(self, word_rows, internal):
        self.w, self.scale = word_rows, pow(1 << (261 if internal else 256), -1, R)

    def __len__(self):
        return self.w.shape[0]

    def __getitem__(self, i):
        return int.from_bytes(self.w[i].tobytes(), "little") * self.scale % R


@pytest.mark.gpu
@pytest.mark.parametrize("internal", [False, True])
def test_more_rows_than_lanes(internal):
    """2^19 rows (8 segments of 2^16) against 1280 x 256 lanes: the grid-stride loop runs a second row in 196 608 of the lanes, on
    slots that hold the first row's values.  Spot rows through evaluate_graph_rows: the first and last row, both sides of the lane
    count, both sides of a segment boundary."""
    import torch
    from halo2_experiments_amd.arithmetic import random_fr
    seg, segments = 1 << 16, 8
    size = seg * segments
    assert size > LANES
    for p in (next(q for q in gp.hand_written() if q.name == "many_live_then_recycled"), gp.random_program(7003)):
        rng = random.Random(19)
        seeds = iter(range(1900, 2000))
        cols = [random_fr((1 << gp.SHORT[i]) if i in gp.SHORT else size, next(seeds), "cuda") for i in range(gp.NF + gp.NA + gp.NI)]
        for c in cols[3:5]:                                     # adversarial cells where the spot rows and their rotations read
            for row in (0, 1, LANES - 1, LANES, LANES + 1, size - 1):
                c[row] = gp.to_device(gp.words([rng.choice(gp.SPECIAL)]))[0]
        values = random_fr(size, next(seeds), "cuda")
        host_cols = [_LazyColumn(c.cpu().numpy().view(np.uint64), False) for c in cols]
        previous = _LazyColumn(values.cpu().numpy().view(np.uint64), False)
        if internal:                                            # the same values, stored as 32 x value
            from halo2_experiments_amd.domain import fr_words
            import halo2_experiments_amd as h
            cols = [h.linear_combination([c.contiguous()], np.stack([fr_words(32)])) for c in cols]
        sc = gp.other_scalars(rng)
        d = gp.Data(seg, segments, host_cols, previous, **sc)
        rows = [0, 1, seg - 1, seg, LANES - 2, LANES - 1, LANES, LANES + 1, LANES + seg, size - seg, size - 2, size - 1]
        exp = gp.oracle_rows(p, d, rows)
        prog = p.compile()
        try:
            prog.evaluate(cols, values, columns_internal=internal, segments=segments, **sc)
            got = gp.device_values(values)
        finally:
            prog.destroy()
        for row, want in zip(rows, exp):
            assert np.array_equal(got[row], gp.words([want])[0]), (p.name, row)
        del cols, values
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_two_handles_alternating_on_two_streams(hc):
    """Two programs, each on its own stream with its own scratch, launched alternately without a synchronisation in between."""
    import torch
    pa, pb = gp.random_program(7005), next(q for q in gp.hand_written() if q.name == "many_live_then_recycled")
    da, db = gp.make_data(random.Random(1), 256, 8), gp.make_data(random.Random(2), 64, 8)
    ea, eb = gp.oracle_values(pa, da), gp.oracle_values(pb, db)
    ha, hb = pa.compile(), pb.compile()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for internal in (False, True):
            ca, cb = gp.device_columns(da, internal), gp.device_columns(db, internal)
            torch.cuda.synchronize()
            outs = []
            for _ in range(4):
                with torch.cuda.stream(sa):
                    va = gp.to_device(gp.words(da.previous))
                    ha.evaluate(ca, va, columns_internal=internal, segments=da.segments, **da.scalars())
                with torch.cuda.stream(sb):
                    vb = gp.to_device(gp.words(db.previous))
                    hb.evaluate(cb, vb, columns_internal=internal, segments=db.segments, **db.scalars())
                outs.append((va, vb))
            sa.synchronize()
            sb.synchronize()
            for va, vb in outs:
                assert np.array_equal(gp.device_values(va), gp.words(ea)), internal
                assert np.array_equal(gp.device_values(vb), gp.words(eb)), internal
            assert np.array_equal(gp.host_replay(hc, pa, da, internal).values, gp.words(ea))
    finally:
        ha.destroy()
        hb.destroy()


@pytest.mark.gpu
def test_argument_errors_of_the_single_entry_launch_nothing(hc):
    """hm_graph_evaluate_segments_dev on a 64-row program: the values or one column base 8 bytes off 16, an unknown flag, no segments,
    log_size 31, another column count and a null column are refused on the host with HM_ERR_BAD_ARG and a ``graph:`` reason, the values
    bit for bit as before (nothing misaligned is ever launched); the same arguments without the fault are accepted and give the host
    replay's words."""
    import ctypes
    from halo2_experiments_amd import _lib
    p = gp.random_program(7003)
    d = gp.make_data(random.Random(64), 64, 1)
    cols = [c if c.shape[0] > 1 else c.expand(2, 4).contiguous() for c in gp.device_columns(d, False)]     # the one-row column twice
    values = gp.to_device(gp.words(d.previous))
    before = gp.device_values(values).copy()
    sc = d.scalars()
    dyn = gp.words(list(sc["challenges"]) + [sc["beta"], sc["gamma"], sc["theta"], sc["y"]])
    lib = _lib.load()
    prog = p.compile()

    def call(ptrs=None, n_columns=len(cols), log_size=6, segments=1, vals=values.data_ptr(), flags=0):
        ptrs = [c.data_ptr() for c in cols] if ptrs is None else ptrs
        return lib.hm_graph_evaluate_segments_dev(ctypes.c_uint64(prog.handle), (ctypes.c_void_p * len(ptrs))(*ptrs), n_columns,
                                                  dyn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dyn.shape[0], log_size, segments,
                                                  ctypes.c_void_p(vals), flags, None)

    try:
        good = [c.data_ptr() for c in cols]
        for fault in (dict(vals=values.data_ptr() + 8), dict(ptrs=good[:gp.NF] + [good[gp.NF] + 8] + good[gp.NF + 1:]), dict(flags=2),
                      dict(segments=0), dict(log_size=31), dict(ptrs=good[:-1], n_columns=len(cols) - 1),
                      dict(ptrs=good[:gp.NF] + [None] + good[gp.NF + 1:])):
            assert call(**fault) == _lib.HM_ERR_BAD_ARG, fault
            assert b"graph:" in lib.hm_last_error(), fault
            assert np.array_equal(gp.device_values(values), before), fault
        assert call() == _lib.HM_OK
        assert np.array_equal(gp.device_values(values), gp.host_replay(hc, p, d, False).values)
        assert not np.array_equal(gp.device_values(values), before)
    finally:
        prog.destroy()
