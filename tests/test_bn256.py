"""CPU suite: halo2_experiments_amd.bn256, the one host statement of the ABI's word format (4 x u64 little-endian Montgomery words,
radix 2^256), against the golden vectors and the big-integer oracle; the public names that used to restate it; and what the
host-only modules may import."""
import ast
import os

import numpy as np
import pytest

from halo2_experiments_amd import arithmetic, bn256, domain, poseidon, shplonk, synthesis

HERE = os.path.dirname(os.path.abspath(bn256.__file__))


def _old_words(v, p):
    """the formula every module used to restate"""
    m = (v % p) * (1 << 256) % p
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def test_constants_are_the_oracles(pyref):
    o = pyref
    assert (bn256.FR_MODULUS, bn256.FQ_MODULUS) == (o.R, o.P)
    assert (bn256.FR_S, bn256.FR_GENERATOR, bn256.FR_ROOT_OF_UNITY, bn256.FR_ZETA) == (o.FR_S, o.FR_GENERATOR, o.FR_ROOT_OF_UNITY, o.FR_ZETA)
    assert pow(bn256.FR_ROOT_OF_UNITY, 1 << 28, o.R) == 1 != pow(bn256.FR_ROOT_OF_UNITY, 1 << 27, o.R)
    assert pow(bn256.FR_ZETA, 3, o.R) == 1 != bn256.FR_ZETA
    assert bn256.FR_RADIX == o.MONT % o.R
    assert bn256.FQ_ONE_MONT.tolist() == o.to_limbs(o.MONT % o.P)


def test_words_and_integers_round_trip(pyref, golden):
    o, g = pyref, golden["field"]
    for name, p, words, array, ints, one, to_mont in (("fr", o.R, bn256.fr_words, bn256.fr_array, bn256.fr_ints, bn256.fr_int, o.fr_to_mont),
                                                      ("fq", o.P, bn256.fq_words, bn256.fq_array, bn256.fq_ints, bn256.fq_int, o.fq_to_mont)):
        # gen_golden.py: rows 0, 1, 3 of *_a are the Montgomery words of 0, 1 and modulus - 1; *_canon the canonical limbs of every row
        canon = [o.from_limbs(row.tolist()) for row in g[f"{name}_canon"]]
        assert canon[:2] == [0, 1] and canon[3] == p - 1
        for v in (0, 1, p - 1, o.R - 1):
            w = words(v)
            assert w.dtype == np.uint64 and w.shape == (4,) and w.tolist() == o.to_limbs(to_mont(v % p))
            assert one(w) == v % p and ints(w) == [v % p]
        assert ints(g[f"{name}_a"]) == canon                                        # all 64 rows, edge values first
        assert np.array_equal(array(canon), g[f"{name}_a"])
        assert np.array_equal(array(canon[:6]).reshape(2, 3, 4), array([canon[:3], canon[3:6]]))     # any nesting
        assert ints(g[f"{name}_a"].view(np.int64).reshape(8, 8, 4)) == canon         # signed views and leading shapes, as tensors give them
        assert array([]).shape == (0, 4) and array([]).dtype == np.uint64 and ints(np.zeros((0, 4), dtype=np.uint64)) == []
        assert words(p).tolist() == [0, 0, 0, 0] and words(-1).tolist() == words(p - 1).tolist()      # reduced, never rejected
    assert np.array_equal(bn256.fr_array(canon_fr := [3, o.R - 1]), o.fr_array(canon_fr))
    assert bn256.fr_ints(o.fr_array([5, o.R - 2])) == o.fr_from_array(o.fr_array([5, o.R - 2])) == [5, o.R - 2]


def test_g1_words_and_integer_pairs(pyref, golden):
    o, g = pyref, golden["curve"]
    gen = g["points"][0]                                                            # gen_golden.py: scalar 1, the generator
    assert g["scalars"][0].tolist() == bn256.fr_words(1).tolist()
    assert np.array_equal(bn256.G1_GENERATOR, gen) and np.array_equal(bn256.g1_words((1, 2)), gen) and o.G1_GEN == (1, 2)
    assert bn256.g1_ints(gen) == (1, 2)
    assert bn256.g1_ints(np.concatenate([gen, bn256.FQ_ONE_MONT])) == (1, 2)         # 12 words: (x, y, 1)
    identity = g["add_sum"][3]                                                      # P + (-P)
    assert not identity.any() and np.array_equal(bn256.g1_words(None), identity)
    assert bn256.g1_ints(identity) is None and bn256.g1_ints(np.zeros(12, dtype=np.uint64)) is None
    assert bn256.g1_ints(np.concatenate([gen, np.zeros(4, dtype=np.uint64)])) is None      # z = 0 whatever x and y hold
    for words, point in zip(g["points"], o.g1_affine_from_array(g["points"])):
        assert bn256.g1_ints(words) == point and np.array_equal(bn256.g1_words(point), words)
    assert np.array_equal(o.g1_affine_array([(1, 2), None]), np.stack([bn256.g1_words((1, 2)), bn256.g1_words(None)]))


def test_the_old_public_names_return_what_they_returned(pyref):
    o = pyref
    for v in (0, 1, o.P - 1, o.R - 1):
        assert np.array_equal(domain.fr_words(v), _old_words(v, o.R)) and domain.fr_words(v).dtype == np.uint64
        assert np.array_equal(arithmetic.fq_words(v), _old_words(v, o.P)) and arithmetic.fq_words(v).dtype == np.uint64
    values = [0, 1, o.P - 1, o.R - 1]
    old_fr = np.stack([_old_words(v, o.R) for v in values])
    got = poseidon.ints_to_words(values)
    assert np.array_equal(got, old_fr) and got.dtype == np.uint64 and got.flags["C_CONTIGUOUS"] and got.flags["WRITEABLE"]
    assert poseidon.ints_to_words([]).shape == (0, 4) and poseidon.ints_to_words([]).dtype == np.uint64
    assert poseidon.ints_to_words(np.array([7, 9], dtype=np.uint64)).tolist() == [_old_words(7, o.R).tolist(), _old_words(9, o.R).tolist()]
    assert poseidon.words_to_ints(old_fr) == [v % o.R for v in values] == poseidon.words_to_ints(old_fr.view(np.int64).reshape(2, 2, 4))
    cols = synthesis.columns_to_words([values, values[::-1]])
    assert np.array_equal(cols, np.stack([old_fr, old_fr[::-1]])) and cols.dtype == np.uint64 and cols.shape == (2, 4, 4)
    assert np.array_equal(arithmetic.FQ_ONE_MONT, _old_words(1, o.P))
    assert np.array_equal(arithmetic.G1_GENERATOR, np.concatenate([_old_words(1, o.P), _old_words(2, o.P)]))
    assert shplonk.g1_words_to_int(arithmetic.G1_GENERATOR) == (1, 2) and shplonk.g1_words_to_int(np.zeros(8, dtype=np.uint64)) is None
    assert shplonk.g1_words_to_int(np.zeros(12, dtype=np.uint64)) is None
    assert shplonk.g1_words_to_int(np.concatenate([_old_words(o.P - 1, o.P), _old_words(o.R - 1, o.P), arithmetic.FQ_ONE_MONT])) == (o.P - 1, o.R - 1)
    assert (domain.FR_MODULUS, domain.FR_ROOT_OF_UNITY, arithmetic.FQ_MODULUS) == (o.R, o.FR_ROOT_OF_UNITY, o.P)


@pytest.mark.parametrize("module", ["bn256", "_header", "pairing", "transcript"])
def test_host_only_modules_do_not_import_the_binding(module):
    tree = ast.parse(open(os.path.join(HERE, module + ".py")).read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            imported.add((node.module or "").split(".")[0])
            if not node.module:                                                      # from . import x
                imported |= {a.name for a in node.names}
    assert not imported & {"ctypes", "torch", "_lib", "arithmetic", "_marshal"}, imported
    if module in ("bn256", "_header"):                                               # and nothing of the package at all
        assert not any(isinstance(n, ast.ImportFrom) and n.level for n in ast.walk(tree))
