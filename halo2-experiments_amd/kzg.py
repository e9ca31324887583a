"""Host-side mirror of ``halo2_proofs::poly::kzg::commitment::ParamsKZG<Bn256>`` (upstream
``halo2_proofs/src/poly/kzg/commitment.rs`` at the tag pinned by /root/reference/Cargo.toml:10; the reference
calls ``ParamsKZG::<Bn256>::setup(k, OsRng)`` at /root/reference/src/circuits/utils.rs:28 on every run).

    setup(k, s)            g[i] = [s^i]G1, g_lagrange[i] = [L_i(s)]G1, g2 = G2, s_g2 = [s]G2
    commit(poly)           best_multiexp(poly, g[..len])           (coefficient form)
    commit_lagrange(poly)  best_multiexp(poly, g_lagrange[..len])  (evaluation form)
    write(f) / read(f)     the SRS on disk, so that it is loaded instead of regenerated every run
    from_monomial(k, g)    g alone (a powers-of-tau SRS): g_lagrange = g_to_lagrange(g, k), an inverse FFT over G1
    downsize(k)            truncate g, recompute g_lagrange, re-register both sets

All G1 work runs on the GPU through the C ABI: the scalar ladder (``hm_fr_powers_dev``), the Lagrange scalars
(one scaled inverse NTT of the ladder: L_i(s) = n^-1 sum_j s^j omega^(-ij)), the 2 n fixed-base multiplications
(``hm_g1_fixed_base_mul_dev``), and the two base sets stay registered on the device.  The single G2 scalar
multiplication of ``s_g2`` is host integer arithmetic (one point, a few milliseconds).

On-disk layouts (little-endian; the field order of upstream's ``ParamsKZG::write``), ``format=`` of read / write:
    "raw_unchecked" (default)  u32 k | n x 64 B g | n x 64 B g_lagrange | 128 B g2 | 128 B s_g2
                               exactly the bytes the Rust types hold: Montgomery limbs, G2Affine = x.c0, x.c1, y.c0, y.c1
    "raw"                      the same bytes; read() rejects a coordinate >= p or a point off the curve
    "processed"                u32 k | n x 32 B g | n x 32 B g_lagrange | 64 B g2 | 64 B s_g2   (compressed points)
[UPSTREAM-RECALLED: later PSE releases name them ``SerdeFormat::RawBytesUnchecked`` / ``RawBytes`` / ``Processed``; the pinned
tag's own ``write`` / ``read`` use the compressed form.]  Compressed G1: canonical x little-endian, bit 7 of byte 31 = parity of
canonical y, the identity 32 zero bytes; G2 likewise over x.c0 | x.c1 with the parity of y.c0 in bit 7 of byte 63.  G1 points
are compressed and decompressed on the GPU (``g1_compress`` / ``g1_decompress``); G2 (two points) in host integers.
"""
from __future__ import annotations

import ctypes
import struct
from typing import BinaryIO, Optional

import numpy as np

from . import _lib
from ._marshal import _is_tensor, _ptr, _stream_ptr
from .arithmetic import (BasesHandle, InvalidPointError, best_multiexp,
                         best_multiexp_submit, best_multiexp_wait, g1_check_host, g1_compress, g1_compress_host, g1_decompress,
                         g1_fixed_base_mul, g_to_lagrange, register_bases, release_bases)
from .bn256 import FQ_MODULUS, FR_MODULUS, G1_GENERATOR, fq_ints, fq_words, fr_words
from .domain import EvaluationDomain

_P = FQ_MODULUS
# bn256::G2Affine::generator() (the alt_bn128 G2 generator of EIP-197), x = x0 + x1 u, y = y0 + y1 u, u^2 = -1
G2_GENERATOR = (
    (0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED,
     0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2),
    (0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA,
     0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B),
)


def _fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % _P, (a[0] * b[1] + a[1] * b[0]) % _P)


def _fq2_sub(a, b):
    return ((a[0] - b[0]) % _P, (a[1] - b[1]) % _P)


def _fq2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, _P)
    return (a[0] * d % _P, -a[1] * d % _P)


def _g2_add(p, q):
    """Affine addition on y^2 = x^3 + 3 / (9 + u) over Fq2 (None = identity)."""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == (0, 0):
            return None
        three_x2 = _fq2_mul((3, 0), _fq2_mul(p[0], p[0]))
        lam = _fq2_mul(three_x2, _fq2_inv(_fq2_mul((2, 0), p[1])))
    else:
        lam = _fq2_mul(_fq2_sub(q[1], p[1]), _fq2_inv(_fq2_sub(q[0], p[0])))
    x3 = _fq2_sub(_fq2_sub(_fq2_mul(lam, lam), p[0]), q[0])
    return (x3, _fq2_sub(_fq2_mul(lam, _fq2_sub(p[0], x3)), p[1]))


def g2_mul(k: int, p=G2_GENERATOR):
    acc = None
    for bit in bin(k % FR_MODULUS)[2:]:
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return acc


def _fq_mont_bytes(v: int) -> bytes:
    return fq_words(v).tobytes()


def g2_bytes(p) -> bytes:
    """G2Affine as the 128 bytes Rust holds: x.c0, x.c1, y.c0, y.c1 (the identity is all-zero)."""
    if p is None:
        return bytes(128)
    return b"".join(_fq_mont_bytes(c) for c in (p[0][0], p[0][1], p[1][0], p[1][1]))


# ---- G2 encodings (two points per SRS: host integers) -----------------------------------------------------------------------------
_B2 = _fq2_mul((3, 0), _fq2_inv((9, 1)))           # the twist's b = 3 / (9 + u)


def _g2_rhs(x):
    x3 = _fq2_mul(_fq2_mul(x, x), x)
    return ((x3[0] + _B2[0]) % _P, (x3[1] + _B2[1]) % _P)


def g2_on_curve(p) -> bool:
    return p is None or _fq2_mul(p[1], p[1]) == _g2_rhs(p[0])


def _fq_sqrt(a: int):
    r = pow(a, (_P + 1) // 4, _P)                  # p = 3 mod 4
    return r if r * r % _P == a % _P else None


def _fq2_sqrt(a):
    """A square root in Fq2 = Fq[u] / (u^2 + 1) by the complex method, or None for a non-residue."""
    a0, a1 = a[0] % _P, a[1] % _P
    if a1 == 0:
        r = _fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = _fq_sqrt(-a0 % _P)
        return None if r is None else (0, r)
    alpha = _fq_sqrt((a0 * a0 + a1 * a1) % _P)     # the norm's root
    if alpha is None:
        return None
    half = (_P + 1) // 2
    x0 = _fq_sqrt((a0 + alpha) * half % _P)
    if x0 is None:
        x0 = _fq_sqrt((a0 - alpha) * half % _P)
        if x0 is None:
            return None
    return (x0, a1 * pow(2 * x0, -1, _P) % _P)


def g2_compress(p) -> bytes:
    """64 bytes: x.c0 | x.c1 canonical little-endian, bit 7 of byte 63 = parity of canonical y.c0; the identity (None) is zeros."""
    if p is None:
        return bytes(64)
    out = bytearray(p[0][0].to_bytes(32, "little") + p[0][1].to_bytes(32, "little"))
    out[63] |= (p[1][0] & 1) << 7
    return bytes(out)


def g2_decompress(data: bytes):
    """The inverse of ``g2_compress``: the affine point, or None for the identity.  Raises ValueError for a coordinate >= p or an x
    that is not on the curve."""
    if len(data) != 64:
        raise ValueError("g2_decompress: 64 bytes expected")
    sign = data[63] >> 7
    b = bytearray(data)
    b[63] &= 0x7F
    x = (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little"))
    if x[0] >= _P or x[1] >= _P:
        raise ValueError("g2_decompress: coordinate >= p")
    if x == (0, 0) and not sign:
        return None
    rhs = _g2_rhs(x)
    y = _fq2_sqrt(rhs)
    if y is None or _fq2_mul(y, y) != rhs:
        raise ValueError("g2_decompress: not on the curve")
    if (y[0] & 1) != sign:
        y = (-y[0] % _P, -y[1] % _P)
    return (x, y)


def g2_from_bytes(data: bytes, check: bool = False):
    """The inverse of ``g2_bytes`` (Montgomery limbs); ``check``: reject a coordinate word >= p or a point off the curve."""
    if len(data) != 128:
        raise ValueError("g2_from_bytes: 128 bytes expected")
    words = [int.from_bytes(data[32 * i: 32 * i + 32], "little") for i in range(4)]
    if check and any(w >= _P for w in words):
        raise ValueError("g2_from_bytes: coordinate >= p")
    if not any(words):
        return None
    c = fq_ints(np.frombuffer(data, dtype=np.uint64))
    p = ((c[0], c[1]), (c[2], c[3]))
    if check and not g2_on_curve(p):
        raise ValueError("g2_from_bytes: not on the curve")
    return p


FORMATS = ("raw_unchecked", "raw", "processed")


def _check_format(fmt: str, who: str) -> None:
    if fmt not in FORMATS:
        raise ValueError(f"{who}: unknown format {fmt!r} (one of {', '.join(FORMATS)})")


class ParamsKZG:
    def __init__(self, k: int, g, g_lagrange, g2: bytes, s_g2: bytes, precompute: bool = False):
        """``g`` / ``g_lagrange``: (n, 8) GPU tensors or numpy arrays of affine Montgomery words."""
        self.k, self.n = k, 1 << k
        self.g2, self.s_g2 = g2, s_g2
        self._precompute = precompute
        self._g_h = register_bases(g, precompute=precompute)
        self._gl_h = register_bases(g_lagrange, precompute=precompute)
        if len(self._g_h) != self.n or len(self._gl_h) != self.n:
            self.release()
            raise ValueError("ParamsKZG: g and g_lagrange must hold 2^k points")

    # -- ParamsKZG::setup / unsafe_setup_with_s --------------------------------------------------
    @classmethod
    def setup(cls, k: int, s: int, device=None, precompute: bool = False, keep_points: bool = False) -> "ParamsKZG":
        """The reference draws s from OsRng (utils.rs:28); here the caller provides it (tests know it)."""
        import torch

        device = device or torch.device("cuda", torch.cuda.current_device())
        n = 1 << k
        lib = _lib.load()
        ladder = torch.empty((n, 4), dtype=torch.int64, device=device)
        _lib.check(lib.hm_fr_powers_dev(ctypes.c_void_p(ladder.data_ptr()), n, _ptr(fr_words(s)), ctypes.c_void_p(_stream_ptr(ladder))))
        g = g1_fixed_base_mul(ladder, G1_GENERATOR)
        lag = EvaluationDomain(2, k).lagrange_to_coeff(ladder)          # in place: n^-1 * NTT_{omega^-1}(ladder) = L_i(s)
        g_lagrange = g1_fixed_base_mul(lag, G1_GENERATOR)
        params = cls(k, g, g_lagrange, g2_bytes(G2_GENERATOR), g2_bytes(g2_mul(s)), precompute=precompute)
        if keep_points:
            params.g_points, params.g_lagrange_points = g, g_lagrange
        return params

    # -- from a universal SRS / ParamsKZG::downsize -------------------------------------------------------
    @staticmethod
    def _device_points(points, device=None):
        import torch

        if _is_tensor(points):
            return points.contiguous()
        device = device or torch.device("cuda", torch.cuda.current_device())
        arr = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        return torch.from_numpy(arr.view(np.int64)).to(device)

    @classmethod
    def from_monomial(cls, k: int, g, g2: bytes, s_g2: bytes, precompute: bool = False) -> "ParamsKZG":
        """Parameters from the monomial points g[i] = [s^i]G1 alone (a powers-of-tau SRS, s unknown): g_lagrange is derived on the
        GPU by ``g_to_lagrange`` (one inverse FFT over G1), and both sets are registered as the constructor does."""
        g = cls._device_points(g)
        if g.shape[0] != 1 << k:
            raise ValueError("ParamsKZG.from_monomial: g must hold 2^k points")
        g_lagrange = g_to_lagrange(g, k)
        params = cls(k, g, g_lagrange, g2, s_g2, precompute=precompute)
        params.g_points, params.g_lagrange_points = g, g_lagrange
        return params

    def downsize(self, k: int) -> None:
        """``ParamsKZG::downsize``: keep the first 2^k monomial points, recompute g_lagrange from them, and replace both registered
        sets.  Needs the affine points (setup(..., keep_points=True), read() or from_monomial())."""
        if k > self.k:
            raise ValueError("ParamsKZG.downsize: k exceeds the current size")
        if not hasattr(self, "g_points"):
            raise ValueError("ParamsKZG.downsize: the affine points were not kept (setup(..., keep_points=True))")
        n = 1 << k
        g = self._device_points(self.g_points)[:n].contiguous()
        g_lagrange = g_to_lagrange(g, k)
        g_h, gl_h = register_bases(g, precompute=self._precompute), register_bases(g_lagrange, precompute=self._precompute)
        self.release()
        self._g_h, self._gl_h = g_h, gl_h
        self.k, self.n = k, n
        self.g_points, self.g_lagrange_points = g, g_lagrange

    def release(self) -> None:
        for name in ("_g_h", "_gl_h"):
            hd = getattr(self, name, None)
            if hd is not None:
                release_bases(hd)
                setattr(self, name, None)

    @property
    def g_handle(self) -> BasesHandle:
        return self._g_h

    @property
    def g_lagrange_handle(self) -> BasesHandle:
        return self._gl_h

    # -- commit / commit_lagrange ------------------------------------------------------------------
    def commit(self, poly) -> np.ndarray:
        return best_multiexp(poly, self._g_h)

    def commit_lagrange(self, poly) -> np.ndarray:
        return best_multiexp(poly, self._gl_h)

    def commit_submit(self, poly) -> int:
        return best_multiexp_submit(poly, self._g_h)

    def commit_lagrange_submit(self, poly) -> int:
        return best_multiexp_submit(poly, self._gl_h)

    commit_wait = staticmethod(best_multiexp_wait)

    # -- write / read --------------------------------------------------------------------------------
    @staticmethod
    def write_points(f: BinaryIO, k: int, g, g_lagrange, g2: bytes, s_g2: bytes, format: str = "raw_unchecked") -> None:
        """``g`` / ``g_lagrange``: (n, 8) numpy arrays, or GPU tensors for ``format="processed"`` (compressed on the device)."""
        _check_format(format, "ParamsKZG.write")
        n = 1 << k
        if format == "processed":
            f.write(struct.pack("<I", k))
            for pts in (g, g_lagrange):
                if _is_tensor(pts):
                    if pts.shape[0] != n:
                        raise ValueError("ParamsKZG.write: g and g_lagrange must hold 2^k points")
                    f.write(g1_compress(pts.contiguous()).cpu().numpy().tobytes())
                else:
                    f.write(g1_compress_host(np.ascontiguousarray(pts, dtype=np.uint64).reshape(n, 8)).tobytes())
            f.write(g2_compress(g2_from_bytes(g2)))
            f.write(g2_compress(g2_from_bytes(s_g2)))
            return
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(n, 8)
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(n, 8)
        f.write(struct.pack("<I", k))
        f.write(g.tobytes())
        f.write(gl.tobytes())
        f.write(g2)
        f.write(s_g2)

    def write(self, f: BinaryIO, format: str = "raw_unchecked") -> None:
        """Needs the affine points (setup(..., keep_points=True), read() or from_monomial())."""
        _check_format(format, "ParamsKZG.write")
        if not hasattr(self, "g_points"):
            raise ValueError("ParamsKZG.write: the affine points were not kept (setup(..., keep_points=True))")
        if format == "processed":
            self.write_points(f, self.k, self.g_points, self.g_lagrange_points, self.g2, self.s_g2, format=format)
            return
        to_np = lambda t: t.cpu().numpy().view(np.uint64) if hasattr(t, "cpu") else np.asarray(t)
        self.write_points(f, self.k, to_np(self.g_points), to_np(self.g_lagrange_points), self.g2, self.s_g2, format=format)

    @classmethod
    def read(cls, f: BinaryIO, precompute: bool = False, format: str = "raw_unchecked") -> "ParamsKZG":
        """``format="raw"`` rejects a coordinate >= p or a point off the curve; ``"processed"`` decodes the compressed points on the
        GPU and registers the device tensors.  An invalid point raises ValueError naming its set (g / g_lagrange / g2 / s_g2) and index."""
        _check_format(format, "ParamsKZG.read")
        head = f.read(4)
        if len(head) != 4:
            raise ValueError("ParamsKZG.read: truncated header")
        (k,) = struct.unpack("<I", head)
        if k > 28:
            raise ValueError("ParamsKZG.read: k out of range")
        n = 1 << k
        if format == "processed":
            return cls._read_processed(f, k, precompute)
        raw = f.read(n * 128 + 256)
        if len(raw) != n * 128 + 256:
            raise ValueError("ParamsKZG.read: truncated file")
        pts = np.frombuffer(raw, dtype=np.uint64, count=n * 16).reshape(2, n, 8)
        g2, s_g2 = raw[n * 128: n * 128 + 128], raw[n * 128 + 128:]
        if format == "raw":
            for name, set_ in (("g", pts[0]), ("g_lagrange", pts[1])):
                try:
                    g1_check_host(set_)
                except InvalidPointError as e:
                    raise InvalidPointError(f"ParamsKZG.read: invalid point in {name} at index {e.index}", e.index) from None
            for name, b in (("g2", g2), ("s_g2", s_g2)):
                try:
                    g2_from_bytes(b, check=True)
                except ValueError as e:
                    raise ValueError(f"ParamsKZG.read: invalid {name}: {e}") from None
        params = cls(k, pts[0], pts[1], g2, s_g2, precompute=precompute)
        params.g_points, params.g_lagrange_points = pts[0], pts[1]
        return params

    @classmethod
    def _read_processed(cls, f: BinaryIO, k: int, precompute: bool) -> "ParamsKZG":
        import torch

        n = 1 << k
        body = np.empty(n * 64, dtype=np.uint8)
        if f.readinto(memoryview(body)) != body.size:
            raise ValueError("ParamsKZG.read: truncated file")
        tail = f.read(128)
        if len(tail) != 128:
            raise ValueError("ParamsKZG.read: truncated file")
        dev = torch.from_numpy(body).to(torch.device("cuda", torch.cuda.current_device()))
        sets = []
        for i, name in enumerate(("g", "g_lagrange")):
            try:
                sets.append(g1_decompress(dev[i * n * 32: (i + 1) * n * 32]))
            except InvalidPointError as e:
                raise InvalidPointError(f"ParamsKZG.read: invalid point in {name} at index {e.index}", e.index) from None
        del dev
        g2s = []
        for name, b in (("g2", tail[:64]), ("s_g2", tail[64:])):
            try:
                g2s.append(g2_bytes(g2_decompress(b)))
            except ValueError as e:
                raise ValueError(f"ParamsKZG.read: invalid {name}: {e}") from None
        params = cls(k, sets[0], sets[1], g2s[0], g2s[1], precompute=precompute)
        params.g_points, params.g_lagrange_points = sets[0], sets[1]
        return params
