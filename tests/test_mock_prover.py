"""``halo2_experiments_amd.mock_prover`` without a GPU: what the constructor refuses, how failures are worded, how a record buffer is
decoded, the three new entry points' argument checks, and the rules the checker's kernels share with the host (csrc/mock_check.h
through libhm_hostcheck.so): the key search against ``bisect``, the value key against Python integers, the record packing."""
import bisect
import ctypes
import random
import subprocess

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, circuits, mock_prover as mp, poseidon as ps, synthesis as sy
from halo2_experiments_amd.circuits import ConstraintSystem
from halo2_experiments_amd.evaluation import Advice, Fixed

R = mp.R
NEW_ENTRIES = ("hm_mock_gates_dev", "hm_mock_copies_dev", "hm_mock_lookup_dev")


def tiny_cs(lookups=None, equality=(("advice", 0), ("fixed", 0), ("instance", 0))):
    gates = [("product", [Fixed(0) * (Advice(0) * Advice(1) - Advice(2))])]
    return ConstraintSystem("tiny", "test", 2, 3, 1, gates, lookups or [], list(equality), blinding_factors=5)


def fixed_ints(n, count=2):
    return [[(7 * c + r) % 11 for r in range(n)] for c in range(count)]


def test_the_module_is_public_and_imports_without_a_gpu():
    assert h.MockProver is mp.MockProver and h.MockResult is mp.MockResult and h.NotSatisfied is mp.NotSatisfied
    prover = mp.MockProver(tiny_cs(), k=4, fixed=fixed_ints(16), copies=[(("advice", 0, 1), ("fixed", 0, 2))])
    assert (prover.k, prover.n, prover.usable, prover.blinding_rows) == (4, 16, 10, 6)
    assert prover._pairs.tolist() == [[1, 16 + 2]]               # cell ids as keygen's: equality column * n + row
    assert prover._perm.tolist() == [2, 0, 5]                     # the table is fixed | advice | instance
    assert [(name, pi) for name, pi, _ in prover.polynomials] == [("product", 0)]


def test_a_layout_gives_k_fixed_columns_and_copies():
    spec = ps.default_spec(5)
    lay = sy.MerkleSumTreeLayout(1, 9, spec)
    prover = mp.MockProver(circuits.merkle_sum_tree(spec), lay)
    assert (prover.k, prover.usable) == (9, 512 - sy.BLINDING_ROWS)
    assert prover.copies == [tuple(map(tuple, c)) for c in lay.copies()] and len(prover._pairs) == len(lay.copies())
    assert np.array_equal(prover._fixed_words, sy.columns_to_words(lay.fixed_columns()))
    with pytest.raises(ValueError, match="not both"):
        mp.MockProver(circuits.merkle_sum_tree(spec), lay, k=9)
    with pytest.raises(ValueError, match="not the circuit's"):
        mp.MockProver(circuits.merkle_v3(), lay)


def test_constructor_refuses_wrong_shapes():
    cs = tiny_cs()
    with pytest.raises(ValueError, match="3 fixed columns given, the constraint system has 2"):
        mp.MockProver(cs, k=4, fixed=fixed_ints(16, 3))
    with pytest.raises(ValueError, match="k too small"):
        mp.MockProver(cs, k=3, fixed=fixed_ints(16))              # columns of 16 rows do not fit k = 3
    with pytest.raises(ValueError, match="k too small"):
        mp.MockProver(cs, k=4, fixed=fixed_ints(16), copies=[(("advice", 0, 16), ("advice", 1, 0))])
    with pytest.raises(ValueError, match="no usable row"):
        mp.MockProver(cs, k=2, fixed=fixed_ints(4))               # 4 rows, 6 of them blinding
    with pytest.raises(ValueError, match="in no column"):
        mp.MockProver(cs, k=4, fixed=fixed_ints(16), copies=[(("advice", 3, 0), ("advice", 0, 0))])
    with pytest.raises(ValueError, match="without equality"):
        mp.MockProver(cs, k=4, fixed=fixed_ints(16), copies=[(("advice", 1, 0), ("advice", 0, 0))])
    with pytest.raises(ValueError, match=r"\(2, 16, 4\) words"):
        mp.MockProver(cs, k=4, fixed=np.zeros((2, 8, 4), dtype=np.uint64))
    with pytest.raises(ValueError, match="need a layout"):
        mp.MockProver(cs, k=4)
    words = sy.columns_to_words(fixed_ints(16))
    assert np.array_equal(mp.MockProver(cs, k=4, fixed=words)._fixed_words, mp.MockProver(cs, k=4, fixed=fixed_ints(16))._fixed_words)


def test_tuple_lookups_are_not_implemented():
    cs = tiny_cs(lookups=[([Advice(0), Advice(1)], [Fixed(0), Fixed(1)])])
    with pytest.raises(NotImplementedError, match="lookup 0 is over a tuple of 2"):
        mp.MockProver(cs, k=4, fixed=fixed_ints(16))
    mp.MockProver(tiny_cs(lookups=[([Advice(0)], [Fixed(1)])]), k=4, fixed=fixed_ints(16))


def test_failures_are_worded_as_upstream_words_them():
    cs = circuits.merkle_v3()
    assert mp.format_failure(("gate", 3, "swap constraint", 0, 17), cs) == \
        "user 3: Constraint 0 in gate 1 ('swap constraint') is not satisfied outside any region, on row 17"
    assert mp.format_failure(("lookup", 0, 5, 202)) == "user 0: Lookup 5 is not satisfied outside any region, on row 202"
    assert mp.format_failure(("copy", 9, ("advice", 2, 4), ("instance", 0, 1))) == \
        ("user 9: Equality constraint not satisfied by cell (Column('Advice', 2), outside any region, on row 4) and cell "
         "(Column('Instance', 0), outside any region, on row 1)")
    with pytest.raises(ValueError):
        mp.format_failure(("nothing", 0))
    res = mp.MockResult(False, {"gate": 1, "copy": 0, "lookup": 0}, [("gate", 0, "g", 0, 1)], [0])
    assert isinstance(mp.NotSatisfied("text", res), AssertionError) and mp.NotSatisfied("text", res).result is res


def test_records_are_decoded_and_sorted():
    pairs = [(0, 0), (0, 9), (1, 0), (2, 5), (2, 0xFFFFFFFF), (0x7FFFFFFF, 3), (0xFFFFFFFF, 1)]
    rec = np.array([(u << 32) | i for u, i in pairs], dtype=np.uint64)
    shuffled = rec[np.random.default_rng(5).permutation(len(rec))]
    assert mp.decode_records(shuffled) == pairs                   # by user, then by row: u64 order, not i64 order
    assert mp.decode_records(shuffled.view(np.int64)) == pairs    # as a torch int64 tensor hands them over
    assert mp.decode_records(np.zeros(0, dtype=np.uint64)) == []


@pytest.fixture(scope="module")
def hostcheck():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_mock_record.restype = ctypes.c_uint64
    lib.hc_mock_record.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    return lib


def _key_words(values):
    return np.array([[(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for v in values], dtype=np.uint32).reshape(-1, 8)


def _search(lib, table, queries):
    tw, qw = _key_words(table), _key_words(queries)
    found, at = np.zeros(len(queries), dtype=np.uint8), np.zeros(len(queries), dtype=np.uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert lib.hc_mock_key_search(tw.ctypes.data_as(u32p), ctypes.c_uint64(len(table)), qw.ctypes.data_as(u32p), ctypes.c_size_t(len(queries)),
                                  found.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), at.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 0
    return found.astype(bool).tolist(), at.tolist()


@pytest.mark.parametrize("case", ["top word only", "bottom word only", "random", "u8", "one key"])
def test_key_search_matches_bisect(hostcheck, case):
    rng = random.Random(len(case))
    if case == "top word only":                                   # equal in words 0 .. 6: only the word that is compared FIRST tells them apart
        low = rng.getrandbits(224)
        table = sorted({(rng.getrandbits(32) << 224) | low for _ in range(300)})
        queries = table[::7] + [(rng.getrandbits(32) << 224) | low for _ in range(200)] + [low, (0xFFFFFFFF << 224) | low]
    elif case == "bottom word only":                              # equal in words 1 .. 7: only the word that is compared LAST does
        high = rng.getrandbits(224) << 32
        table = sorted({high | rng.getrandbits(32) for _ in range(300)})
        queries = table[::7] + [high | rng.getrandbits(32) for _ in range(200)] + [high, high | 0xFFFFFFFF]
    elif case == "random":
        table = sorted(rng.randrange(R) for _ in range(257))
        queries = table[::3] + [rng.randrange(R) for _ in range(100)] + [0, R - 1]
    elif case == "u8":                                            # the reference's table, with the zeros of the unused rows repeated
        table = sorted(list(range(256)) + [0] * 250)
        queries = list(range(300)) + [1 << 32, 255 + (1 << 224), R - 1]
    else:
        table, queries = [5], [4, 5, 6]
    found, at = _search(hostcheck, table, queries)
    assert at == [bisect.bisect_left(table, q) for q in queries]
    assert found == [q in set(table) for q in queries]
    assert any(found) and not all(found)


def test_value_key_is_the_canonical_integer(hostcheck):
    rng = random.Random(11)
    values = [0, 1, 2, 255, 256, R - 1, R - 2, (1 << 253) + 5] + [rng.randrange(R) for _ in range(40)]
    words = ps.ints_to_words(values).view(np.uint32).reshape(-1, 8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for v, w in zip(values, words):
        key = np.zeros(8, dtype=np.uint32)
        assert hostcheck.hc_mock_value_key(np.ascontiguousarray(w).ctypes.data_as(u32p), key.ctypes.data_as(u32p)) == 0
        assert sum(int(x) << (32 * j) for j, x in enumerate(key)) == v


def test_record_packing(hostcheck):
    for user, index in [(0, 0), (1, 2), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (0x80000000, 0x80000001)]:
        u, i = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rec = hostcheck.hc_mock_record(user, index, ctypes.byref(u), ctypes.byref(i))
        assert rec == (user << 32) | index and (u.value, i.value) == (user, index)
        assert mp.decode_records(np.array([rec], dtype=np.uint64)) == [(user, index)]


def test_entry_points_are_declared_bound_and_check_their_arguments():
    lib = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    rust = open(_lib.HEADER_PATH.replace("include/halo2_mi355x.h", "rust/halo2-mi355x-sys/src/lib.rs")).read()
    for name in NEW_ENTRIES:
        assert name in _lib._SIGNATURES and f"int {name}(" in header and f"pub fn {name}(" in rust
    out = ctypes.c_uint64(77)
    a = np.zeros(64, dtype=np.uint64)                                                    # stands for device memory: never dereferenced
    base = a.ctypes.data + (-a.ctypes.data) % 16
    bases, strides, rows = (ctypes.c_void_p * 1)(base), (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(16)
    vp = ctypes.c_void_p
    u64 = lambda addr: ctypes.cast(vp(addr), ctypes.POINTER(ctypes.c_uint64))       # the record and counter arguments are uint64_t*
    u32 = lambda addr: ctypes.cast(vp(addr), ctypes.POINTER(ctypes.c_uint32))
    good = dict(graph=ctypes.c_uint64(1), bases=bases, strides=strides, rows=rows, n=1, k=4, usable=10, m=1, rec=u64(base), cap=4, counter=u64(base + 64),
                flags=vp(base + 128))

    def gates(**kw):
        g = dict(good, **kw)
        return lib.hm_mock_gates_dev(g["graph"], g["bases"], g["strides"], g["rows"], g["n"], None, 0, g["k"], g["usable"], g["m"], None, 0,
                                     g["rec"], g["cap"], g["counter"], g["flags"], ctypes.byref(out), None)

    refused = [dict(m=0), dict(cap=0), dict(rows=(ctypes.c_uint32 * 1)(17)), dict(bases=(ctypes.c_void_p * 1)(base + 8)), dict(k=31),
               dict(usable=0), dict(usable=17), dict(rec=u64(base + 4)), dict(counter=None), dict(n=0), dict(n=257),
               dict(strides=(ctypes.c_uint64 * 1)(2)), dict(bases=None)]
    for kw in refused:
        assert gates(**kw) == -1, kw
        assert b"hm_mock_gates_dev" in lib.hm_last_error()
    perm = (ctypes.c_uint32 * 1)(0)
    assert lib.hm_mock_copies_dev(bases, strides, rows, 1, perm, 1, u32(base), 0, 4, 1, u64(base), 4, u64(base + 64), vp(base + 128), ctypes.byref(out), None) == -1
    assert lib.hm_mock_copies_dev(bases, strides, rows, 1, (ctypes.c_uint32 * 1)(1), 1, u32(base), 3, 4, 1, u64(base), 4, u64(base + 64), vp(base + 128),
                                  ctypes.byref(out), None) == -1
    assert lib.hm_mock_lookup_dev(ctypes.c_uint64(1), bases, strides, rows, 1, None, 0, 4, 10, 1, 0, None, u64(base), 4, u64(base + 64), vp(base + 128),
                                  ctypes.byref(out), None) == -1
    assert out.value == 77 and not a.any()
    if lib.hm_device_count() == 0:                                                       # valid-looking arguments: no device, no fallback
        assert gates() == -2
