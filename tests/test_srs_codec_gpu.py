"""SRS point encodings on the MI355X (hm_g1_compress / decompress / check, device and host forms; ParamsKZG.read / write formats).

The decoding rule is restated here in big integers (tests/test_srs_codec.py: encode / decode) and every device answer is compared with
it: known answers, 4096 points of both parities with planted identities and invalid entries, round trips at every size to 2^12 and on a
setup(k=20) SRS, the checked raw format, the host forms and their fault points, and the KZG files in every format."""
import ctypes
import io
import random

import numpy as np
import pytest

import halo2_experiments_amd as h
from halo2_experiments_amd import _lib, kzg
from halo2_experiments_amd.arithmetic import G1_GENERATOR
from halo2_experiments_amd.domain import FR_MODULUS as R
from oracle import bn256_ref as o
from test_srs_codec import decode, encode

pytestmark = pytest.mark.gpu

P = o.P
HM_ERR_INTERNAL, HM_ERR_INVALID_DATA = -5, -7


def _dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda")


def _np(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _bytes(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 32).copy()


def _x_non_residue():
    return next(x for x in range(1, 100) if pow(x ** 3 + 3, (P - 1) // 2, P) != 1)


def test_known_answers():
    pts = [(1, 2), (1, P - 2), None]
    comp = _np(h.g1_compress(_dev(o.g1_affine_array(pts))))
    assert comp[0].tobytes() == b"\x01" + bytes(31)
    assert comp[1].tobytes() == b"\x01" + bytes(30) + b"\x80"
    assert not comp[2].any()
    assert np.array_equal(_np(h.g1_decompress(_dev(comp))), o.g1_affine_array(pts))


def test_parity_against_the_rule_on_4096_points():
    n = 4096
    rng = random.Random(4096)
    aff = _np(h.g1_fixed_base_mul(h.random_fr(n, 409), G1_GENERATOR)).copy()
    for i in rng.sample(range(n), 40):
        aff[i] = 0                                                      # planted identities
    pts = [None if not r.any() else (o.from_limbs(r[:4]) * pow(1 << 256, -1, P) % P, o.from_limbs(r[4:]) * pow(1 << 256, -1, P) % P)
           for r in aff]
    assert {p[1] & 1 for p in pts if p} == {0, 1}
    comp = _np(h.g1_compress(_dev(aff)))
    assert comp.tobytes() == b"".join(encode(p) for p in pts)
    assert np.array_equal(_np(h.g1_decompress(_dev(comp))), aff)
    # a planted x = 0 with the sign bit set: the rule says invalid (3 is not a square mod p), and so must the device
    planted = comp.copy()
    planted[777] = 0
    planted[777, 31] = 0x80
    assert decode(planted[777].tobytes()) == (False, None)
    with pytest.raises(ValueError, match="index 777"):
        h.g1_decompress(_dev(planted))


def test_invalid_inputs_and_the_smallest_index():
    good = encode((1, 2))
    for bad in (P.to_bytes(32, "little"), ((1 << 254) - 1).to_bytes(32, "little"), _x_non_residue().to_bytes(32, "little")):
        assert not decode(bad)[0]
        with pytest.raises(ValueError, match="index 1") as e:
            h.g1_decompress(_dev(_bytes([good, bad, good])))
        assert e.value.index == 1
    rows = [good] * 300
    for i in (250, 37, 129):
        rows[i] = _x_non_residue().to_bytes(32, "little")
    import torch
    lib = _lib.load()
    src, out = _dev(_bytes(rows)), torch.zeros((300, 8), dtype=torch.int64, device="cuda")
    bad = ctypes.c_uint64(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.hm_g1_decompress_bn256_dev(ctypes.c_void_p(src.data_ptr()), 300, ctypes.c_void_p(out.data_ptr()), ctypes.byref(bad), st) \
        == HM_ERR_INVALID_DATA
    assert bad.value == 37 and b"index 37" in lib.hm_last_error()
    got = _np(out)
    assert not got[[37, 129, 250]].any() and np.array_equal(got[0], o.g1_affine_array([(1, 2)])[0])
    assert lib.hm_g1_decompress_bn256_dev(ctypes.c_void_p(src.data_ptr()), 30, ctypes.c_void_p(out.data_ptr()), ctypes.byref(bad), st) == 0
    assert bad.value == 30


def test_round_trips_at_every_size():
    for log_n in range(13):
        n = 1 << log_n
        pts = h.g1_fixed_base_mul(h.random_fr(n, 100 + log_n), G1_GENERATOR)
        if n >= 4:
            pts[n // 2] = 0
        import torch
        assert torch.equal(h.g1_decompress(h.g1_compress(pts)), pts), log_n


def test_setup_srs_round_trip_and_check():
    import torch
    from halo2_experiments_amd.kzg import ParamsKZG
    params = ParamsKZG.setup(20, random.Random(20).randrange(2, R), keep_points=True)
    try:
        for pts in (params.g_points, params.g_lagrange_points):
            assert torch.equal(h.g1_decompress(h.g1_compress(pts)), pts)
            h.g1_check(pts)
    finally:
        params.release()


def test_check_accepts_and_rejects():
    aff = _np(h.g1_fixed_base_mul(h.random_fr(64, 64), G1_GENERATOR)).copy()
    aff[5] = 0
    h.g1_check(_dev(aff))                                               # (0, 0) is the identity
    y1 = aff.copy()
    y = o.from_limbs(y1[9, 4:]) * pow(1 << 256, -1, P) % P
    y1[9, 4:] = o.to_limbs((y + 1) * (1 << 256) % P)                    # y + 1: off the curve
    with pytest.raises(ValueError, match="index 9"):
        h.g1_check(_dev(y1))
    over = aff.copy()
    over[12, 0:4] = o.to_limbs(P)                                       # a coordinate word = p (x = 0 in value, not canonical)
    with pytest.raises(ValueError, match="index 12"):
        h.g1_check(_dev(over))
    with pytest.raises(ValueError, match="index 9"):
        h.g1_check_host(np.concatenate([y1[:12], over[12:]]))


def test_host_forms_equal_device_forms():
    aff = _np(h.g1_fixed_base_mul(h.random_fr(1000, 1000), G1_GENERATOR)).copy()
    aff[3] = 0
    comp = h.g1_compress_host(aff)
    assert np.array_equal(comp, _np(h.g1_compress(_dev(aff))))
    assert np.array_equal(h.g1_decompress_host(comp), aff)
    h.g1_check_host(aff)
    comp[500] = np.frombuffer(_x_non_residue().to_bytes(32, "little"), dtype=np.uint8)
    with pytest.raises(ValueError, match="index 500"):
        h.g1_decompress_host(comp)


def test_host_forms_leave_the_output_untouched_on_a_fault():
    fi = _lib.load_fi()
    aff = _np(h.g1_fixed_base_mul(h.random_fr(256, 256), G1_GENERATOR)).copy()
    comp = h.g1_compress_host(aff)
    u64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out8, out32, bad = np.full((256, 8), 7, dtype=np.uint64), np.full((256, 32), 7, dtype=np.uint8), ctypes.c_uint64(0)
    try:
        for point in (b"g1_codec_upload", b"g1_codec_download"):
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_g1_compress_bn256(u64(aff), 256, vp(out32)) == HM_ERR_INTERNAL and point in fi.hm_last_error()
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_g1_decompress_bn256(vp(comp), 256, u64(out8), ctypes.byref(bad)) == HM_ERR_INTERNAL
            assert point in fi.hm_last_error()
            assert (out8 == 7).all() and (out32 == 7).all()
        fi.hm_test_arm_fault(None, 0)
        assert fi.hm_g1_compress_bn256(u64(aff), 256, vp(out32)) == 0
        assert fi.hm_g1_decompress_bn256(vp(comp), 256, u64(out8), ctypes.byref(bad)) == 0 and bad.value == 256
    finally:
        fi.hm_test_arm_fault(None, 0)
    assert np.array_equal(out32, comp) and np.array_equal(out8, aff)


# ---- ParamsKZG files ------------------------------------------------------------------------------------------------------------

def _fs_commit(s, coeffs):
    """[f(s)]G for f's coefficients (Fr Montgomery words), as the 12-word output of best_multiexp."""
    from halo2_experiments_amd.arithmetic import FQ_ONE_MONT
    c = o.fr_from_array(_np(coeffs))
    v = 0
    for a in reversed(c):
        v = (v * s + a) % R
    out = np.zeros(12, dtype=np.uint64)
    pt = o.g1_mul(v, (1, 2))
    if pt is not None:
        out[:8] = o.g1_affine_array([pt])[0]
        out[8:] = FQ_ONE_MONT
    return out


def test_params_processed_round_trip_and_commitments():
    import torch
    from halo2_experiments_amd.kzg import ParamsKZG
    k = 10
    n = 1 << k
    s = random.Random(1010).randrange(2, R)
    ref = ParamsKZG.setup(k, s, keep_points=True)
    back = None
    try:
        f = io.BytesIO()
        ref.write(f, format="processed")
        assert len(f.getvalue()) == 4 + 64 * n + 128
        f.seek(0)
        back = ParamsKZG.read(f, format="processed")
        assert torch.equal(back.g_points, ref.g_points) and torch.equal(back.g_lagrange_points, ref.g_lagrange_points)
        assert back.g2 == ref.g2 and back.s_g2 == ref.s_g2
        poly = h.random_fr(n, 1011)
        want = ref.commit(poly)
        assert np.array_equal(back.commit(poly), want) and np.array_equal(want, _fs_commit(s, poly))
        # commit_lagrange of evaluations equals commit of the coefficients they interpolate
        evals = poly.clone()
        from halo2_experiments_amd.domain import EvaluationDomain
        coeffs = EvaluationDomain(2, k).lagrange_to_coeff(evals.clone())
        assert np.array_equal(back.commit_lagrange(evals), ref.commit_lagrange(evals))
        assert np.array_equal(back.commit_lagrange(evals), _fs_commit(s, coeffs))
        f2 = io.BytesIO()
        back.write(f2, format="processed")
        assert f2.getvalue() == f.getvalue()
    finally:
        for p in (ref, back):
            if p is not None:
                p.release()


def test_checked_raw_read_names_the_bad_point_and_the_default_still_loads():
    from halo2_experiments_amd.kzg import ParamsKZG
    k = 8
    n = 1 << k
    ref = ParamsKZG.setup(k, 12345, keep_points=True)
    loaded = []
    try:
        f = io.BytesIO()
        ref.write(f, format="raw")
        good = f.getvalue()
        assert good == _default_bytes(ref)
        loaded.append(ParamsKZG.read(io.BytesIO(good), format="raw"))
        data = bytearray(good)
        off = 4 + n * 64 + 77 * 64 + 32                                   # g_lagrange[77].y, lowest byte
        data[off] ^= 1
        with pytest.raises(ValueError, match="g_lagrange at index 77"):
            ParamsKZG.read(io.BytesIO(bytes(data)), format="raw")
        loaded.append(ParamsKZG.read(io.BytesIO(bytes(data))))            # the default reads it as before, unchecked
        assert loaded[-1].g_lagrange_points.tobytes() == bytes(data[4 + n * 64: 4 + n * 128])
        fp = io.BytesIO()
        ref.write(fp, format="processed")
        comp = bytearray(fp.getvalue())
        comp[4 + 5 * 32: 4 + 6 * 32] = _x_non_residue().to_bytes(32, "little")
        with pytest.raises(ValueError, match=r"in g at index 5"):
            ParamsKZG.read(io.BytesIO(bytes(comp)), format="processed")
    finally:
        ref.release()
        for p in loaded:
            p.release()


def _default_bytes(params):
    f = io.BytesIO()
    params.write(f)
    return f.getvalue()


def _pcie_bytes():
    st = _lib.Stats()
    _lib.check(_lib.load().hm_get_stats(ctypes.byref(st)))
    return np.array([st.h2d_bytes, st.d2h_bytes], dtype=np.int64)


def test_host_forms_count_the_bytes_they_move():
    """hm_get_stats' h2d_bytes / d2h_bytes per host form at n = 3: 64-byte points one way, 32-byte encodings the other; the check
    downloads nothing."""
    aff = _np(h.g1_fixed_base_mul(h.random_fr(3, 3), G1_GENERATOR)).copy()
    b0 = _pcie_bytes()
    comp = h.g1_compress_host(aff)
    assert (_pcie_bytes() - b0).tolist() == [3 * 64, 3 * 32]
    b0 = _pcie_bytes()
    assert np.array_equal(h.g1_decompress_host(comp), aff)
    assert (_pcie_bytes() - b0).tolist() == [3 * 32, 3 * 64]
    b0 = _pcie_bytes()
    h.g1_check_host(aff)
    assert (_pcie_bytes() - b0).tolist() == [3 * 64, 0]
