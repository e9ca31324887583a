"""CPU checks of the SRS point encodings (ParamsKZG.read / write formats): the six entry points are exported and
bound, their argument checks answer before any device is needed, the kernels' per-point formulas (csrc/g1_codec.inc, built on the host
with bound tracking) agree with a big-integer restatement of the decoding rule, and the G2 encoding round-trips in host integers."""
import ctypes
import io
import os
import random
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib
import halo2_experiments_amd as h
from halo2_experiments_amd import kzg
from oracle import bn256_ref as o

P = o.P
HM_ERR_BAD_ARG, HM_ERR_NO_DEVICE = -1, -2
NAMES = {"hm_g1_compress_bn256_dev": 4, "hm_g1_decompress_bn256_dev": 5, "hm_g1_check_bn256_dev": 4,
         "hm_g1_compress_bn256": 3, "hm_g1_decompress_bn256": 4, "hm_g1_check_bn256": 3}


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def encode(pt) -> bytes:
    """The compressed rule restated: canonical x little-endian, bit 7 of byte 31 = parity of y; the identity is zeros."""
    if pt is None:
        return bytes(32)
    b = bytearray(pt[0].to_bytes(32, "little"))
    b[31] |= (pt[1] & 1) << 7
    return bytes(b)


def decode(b: bytes):
    """-> (valid, point or None)."""
    sign = b[31] >> 7
    x = int.from_bytes(b[:31] + bytes([b[31] & 0x7F]), "little")
    if x >= P:
        return False, None
    if x == 0 and not sign:
        return True, None
    rhs = (x ** 3 + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return False, None
    if (y & 1) != sign:
        y = P - y
    return True, (x, y)


def test_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NAMES.items():
        assert hasattr(lib, name) and len(_lib._SIGNATURES[name][1]) == arity
    for name in ("g1_compress", "g1_decompress", "g1_check", "g1_compress_host", "g1_decompress_host", "g1_check_host"):
        assert callable(getattr(h, name)) and name in h.__all__
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define HM_ERR_INVALID_DATA (-7)" in hdr


def test_argument_errors_come_before_the_device():
    lib = _lib.load()
    pts, enc, bad = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 32), dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    fake = ctypes.c_void_p(0x1000)                       # never dereferenced: the checks answer first
    big = (1 << 30) + 1
    assert lib.hm_g1_compress_bn256_dev(None, 2, fake, None) == HM_ERR_BAD_ARG and b"null" in lib.hm_last_error()
    assert lib.hm_g1_compress_bn256_dev(fake, 2, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_compress_bn256_dev(fake, big, fake, None) == HM_ERR_BAD_ARG and b"n > 2^30" in lib.hm_last_error()
    assert lib.hm_g1_decompress_bn256_dev(fake, 2, fake, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_decompress_bn256_dev(fake, big, fake, _u64(bad), None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_check_bn256_dev(None, 2, _u64(bad), None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_check_bn256_dev(fake, 2, None, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_check_bn256_dev(fake, big, _u64(bad), None) == HM_ERR_BAD_ARG and b"n > 2^30" in lib.hm_last_error()
    assert lib.hm_g1_compress_bn256(_u64(pts), 2, None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_decompress_bn256(_vp(enc), 2, None, _u64(bad)) == HM_ERR_BAD_ARG
    assert lib.hm_g1_decompress_bn256(_vp(enc), 2, _u64(pts), None) == HM_ERR_BAD_ARG
    assert lib.hm_g1_check_bn256(None, 2, _u64(bad)) == HM_ERR_BAD_ARG
    assert lib.hm_g1_check_bn256(_u64(pts), big, _u64(bad)) == HM_ERR_BAD_ARG
    assert not pts.any() and not enc.any()


def test_no_device_means_error_not_fallback():
    lib = _lib.load()
    if lib.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = ctypes.c_void_p(0x1000)
    bad = np.zeros(1, dtype=np.uint64)
    assert lib.hm_g1_compress_bn256_dev(fake, 2, fake, None) == HM_ERR_NO_DEVICE
    assert lib.hm_g1_decompress_bn256_dev(fake, 2, fake, _u64(bad), None) == HM_ERR_NO_DEVICE
    assert lib.hm_g1_check_bn256_dev(fake, 2, _u64(bad), None) == HM_ERR_NO_DEVICE
    pts = o.g1_affine_array([(1, 2), (1, P - 2)])
    for call in (lambda: h.g1_compress_host(pts), lambda: h.g1_check_host(pts),
                 lambda: h.g1_decompress_host(np.frombuffer(encode((1, 2)), dtype=np.uint8))):
        with pytest.raises(_lib.Halo2Mi355xError) as e:
            call()
        assert e.value.code == HM_ERR_NO_DEVICE


# ---- the kernels' per-point code on the host (libhm_hostcheck.so, -DHM_BOUNDS) ---------------------------------------------------

@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    return ctypes.CDLL(_lib.HOSTCHECK_PATH)


def _hc(hc, op, arr):
    n = arr.shape[0]
    out = np.zeros((n, 16 if op == 1 else 8), dtype=np.uint32)
    valid = np.zeros(n, dtype=np.int32)
    hc.hc_g1_codec(op, _vp(np.ascontiguousarray(arr)), _vp(out), _vp(valid), ctypes.c_size_t(n))
    return out, valid.astype(bool)


def test_host_build_of_the_kernel_formulas_matches_the_rule(hc):
    """Every input enters at the 2^256 class bound, so this run (both y parities, identities, invalid x) is also the bound proof."""
    rng = random.Random(31)
    pts = [o.g1_mul(rng.randrange(1, o.R), (1, 2)) for _ in range(64)] + [(1, 2), (1, P - 2), None]
    aff = o.g1_affine_array(pts)
    assert {p[1] & 1 for p in pts if p} == {0, 1}
    words = aff.view(np.uint32).reshape(len(pts), 16)
    comp, ok = _hc(hc, 0, words)
    assert ok.all() and comp.tobytes() == b"".join(encode(p) for p in pts)
    back, ok = _hc(hc, 1, comp)
    assert ok.all() and np.array_equal(back.view(np.uint64).reshape(-1, 8), aff)
    _, ok = _hc(hc, 2, words)
    assert ok.all()

    x_nr = next(x for x in range(1, 100) if pow(x ** 3 + 3, (P - 1) // 2, P) != 1)
    bad = [P.to_bytes(32, "little"), ((1 << 254) - 1).to_bytes(32, "little"), x_nr.to_bytes(32, "little"),
           bytes(31) + b"\x80"]                                              # x = 0 with the sign set: 3 is a non-residue
    rows = np.frombuffer(b"".join(bad), dtype=np.uint32).reshape(len(bad), 8)
    out, ok = _hc(hc, 1, rows)
    assert [decode(b)[0] for b in bad] == [False] * 4 and not ok.any() and not out.any()

    y1 = o.g1_affine_array([(1, 3)]).view(np.uint32).reshape(1, 16)          # off the curve
    over = words[:1].copy()
    over.view(np.uint64)[0, :4] = [int(w) for w in o.to_limbs(P)]             # a coordinate word = p
    _, ok = _hc(hc, 2, np.concatenate([y1, over, np.zeros((1, 16), dtype=np.uint32)]))
    assert list(ok) == [False, False, True]


# ---- G2 in host integers, formats -----------------------------------------------------------------------------------------------

def test_g2_round_trips_and_known_bytes():
    gen = kzg.G2_GENERATOR
    (x0, x1), (y0, _) = gen
    want = bytearray(x0.to_bytes(32, "little") + x1.to_bytes(32, "little"))
    want[63] |= (y0 & 1) << 7
    assert kzg.g2_compress(gen) == bytes(want)
    s = random.Random(2).randrange(2, o.R)
    for p in (gen, kzg.g2_mul(s), kzg._g2_add(gen, gen)):
        assert kzg.g2_on_curve(p) and kzg.g2_decompress(kzg.g2_compress(p)) == p
        neg = (p[0], (-p[1][0] % P, -p[1][1] % P))
        assert kzg.g2_decompress(kzg.g2_compress(neg)) == neg
    assert kzg.g2_compress(None) == bytes(64) and kzg.g2_decompress(bytes(64)) is None
    assert kzg.g2_from_bytes(kzg.g2_bytes(gen), check=True) == gen


def test_g2_rejects_bad_encodings():
    with pytest.raises(ValueError, match=">= p"):
        kzg.g2_decompress(P.to_bytes(32, "little") + bytes(32))
    x = next(x for x in range(1, 50) if kzg._fq2_sqrt(kzg._g2_rhs((x, 0))) is None)
    with pytest.raises(ValueError, match="not on the curve"):
        kzg.g2_decompress(x.to_bytes(32, "little") + bytes(32))
    off = bytearray(kzg.g2_bytes(kzg.G2_GENERATOR))
    off[64] ^= 1
    with pytest.raises(ValueError, match="not on the curve"):
        kzg.g2_from_bytes(bytes(off), check=True)


def test_unknown_format_raises():
    with pytest.raises(ValueError, match="unknown format"):
        kzg.ParamsKZG.read(io.BytesIO(b"\x00" * 4), format="compressed")
    with pytest.raises(ValueError, match="unknown format"):
        kzg.ParamsKZG.write_points(io.BytesIO(), 0, np.zeros((1, 8), np.uint64), np.zeros((1, 8), np.uint64), bytes(128), bytes(128),
                                   format="RawBytes")
    assert kzg.FORMATS == ("raw_unchecked", "raw", "processed")


def test_default_write_is_unchanged_bytes():
    g = o.g1_affine_array([(1, 2), (1, P - 2)])
    gl = o.g1_affine_array([None, (1, 2)])
    f1, f2 = io.BytesIO(), io.BytesIO()
    kzg.ParamsKZG.write_points(f1, 1, g, gl, bytes(range(128)), bytes(128))
    kzg.ParamsKZG.write_points(f2, 1, g, gl, bytes(range(128)), bytes(128), format="raw")
    assert f1.getvalue() == f2.getvalue() == b"\x01\x00\x00\x00" + g.tobytes() + gl.tobytes() + bytes(range(128)) + bytes(128)
