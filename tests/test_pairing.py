"""pairing.py on the CPU: bilinearity, non-degeneracy, the order of the target group, and pairing_check on a KZG-shaped pair."""
import pytest

from halo2_experiments_amd import pairing as pr
from halo2_experiments_amd.kzg import G2_GENERATOR, g2_mul


@pytest.fixture(scope="module")
def e_gen():
    return pr.pairing(pr.G1_GEN, G2_GENERATOR)


@pytest.mark.parametrize("a,b", [(1, 2), (2, 1), (3, 5), (7, 11)])
def test_bilinear(e_gen, a, b):
    assert pr.pairing(pr.g1_mul(a), g2_mul(b)) == pr.f12_pow(e_gen, a * b)


def test_inverse_and_order(e_gen):
    assert e_gen != pr.F12_ONE
    assert pr.f12_mul(e_gen, pr.pairing(pr.g1_neg(pr.G1_GEN), G2_GENERATOR)) == pr.F12_ONE
    assert pr.f12_pow(e_gen, pr.R) == pr.F12_ONE
    assert pr.f12_mul(e_gen, pr.f12_inv(e_gen)) == pr.F12_ONE
    assert pr.pairing(None, G2_GENERATOR) == pr.F12_ONE


def test_pairing_check():
    s = 0x5EED5EED5EED5EED0123456789ABCDEF % pr.R
    assert pr.pairing_check([(pr.g1_mul(s), G2_GENERATOR), (pr.g1_neg(pr.G1_GEN), g2_mul(s))])
    assert not pr.pairing_check([(pr.g1_mul(s + 1), G2_GENERATOR), (pr.g1_neg(pr.G1_GEN), g2_mul(s))])
    assert not pr.pairing_check([((1, 3), G2_GENERATOR)])                 # off the curve: refused, not an exception
    with pytest.raises(ValueError):
        pr.pairing((1, 3), G2_GENERATOR)


def test_g1_integers():
    assert pr.g1_mul(pr.R) is None and pr.g1_on_curve(pr.g1_mul(12345))
    assert pr.g1_msm([3, 4], [pr.G1_GEN, pr.g1_mul(5)]) == pr.g1_mul(23)
    assert pr.g1_add(pr.g1_mul(9), pr.g1_neg(pr.g1_mul(9))) is None
