"""Blake2b-512 and the verifier's transcripts on the GPU (``hm_blake2b512_dev`` / ``hm_verify_transcript_dev``, csrc/transcript.inc):
one lane per message, and one lane per proof of a batch that absorbs the proof's records in the order of ``verifier._verify`` and
leaves the eight challenges, reduced mod r, in the records ``hm_verify_terms_dev`` reads -- nothing comes back to the host.
For proofs in the "evm" encoding the same with Keccak-256 (``hm_keccak256_dev`` / ``hm_verify_transcript_evm_dev``, csrc/keccak.inc).

``proof_layout.transcript_challenges`` (``hashlib``) stays the oracle and the default; ``BatchVerifier(transcript="device")`` is
what calls ``challenges``."""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _stream_ptr
from .transcript import check_encoding

_vp = ctypes.c_void_p
_u32p = ctypes.POINTER(ctypes.c_uint32)
MODES = ("host", "device")


def blake2b(messages: Sequence[bytes], person: bytes = b"") -> List[bytes]:
    """``hashlib.blake2b(m, digest_size=64, person=person).digest()`` of every message, in one launch"""
    import torch

    messages = [bytes(m) for m in messages]
    if len(person) > 16:
        raise ValueError("blake2b: the personalisation holds 16 bytes at most")
    if not messages:
        return []
    stride = max(4, -(-max(len(m) for m in messages) // 4) * 4)
    raw = np.zeros((len(messages), stride), dtype=np.uint8)
    for i, m in enumerate(messages):
        raw[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_msgs = torch.from_numpy(raw).to(dev)
    d_lens = torch.tensor([len(m) for m in messages], dtype=torch.int32, device=dev)
    d_out = torch.empty((len(messages), 64), dtype=torch.uint8, device=dev)
    personal = (ctypes.c_uint8 * 16)(*person.ljust(16, b"\0")) if person else None
    _lib.check(_lib.load().hm_blake2b512_dev(_vp(d_msgs.data_ptr()), stride, _dev_ptr(d_lens, _u32p), len(messages),
                                            ctypes.cast(personal, _vp) if personal is not None else _vp(None), _vp(d_out.data_ptr()),
                                            _vp(_stream_ptr(d_out))))
    return [bytes(row) for row in d_out.cpu().numpy()]


def keccak256(messages: Sequence[bytes]) -> List[bytes]:
    """``transcript.keccak256(m)`` (Keccak-256, the padding byte 0x01) of every message, in one launch"""
    import torch

    messages = [bytes(m) for m in messages]
    if not messages:
        return []
    stride = max(4, -(-max(len(m) for m in messages) // 4) * 4)
    raw = np.zeros((len(messages), stride), dtype=np.uint8)
    for i, m in enumerate(messages):
        raw[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_msgs = torch.from_numpy(raw).to(dev)
    d_lens = torch.tensor([len(m) for m in messages], dtype=torch.int32, device=dev)
    d_out = torch.empty((len(messages), 32), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().hm_keccak256_dev(_vp(d_msgs.data_ptr()), stride, _dev_ptr(d_lens, _u32p), len(messages), _vp(d_out.data_ptr()),
                                           _vp(_stream_ptr(d_out))))
    return [bytes(row) for row in d_out.cpu().numpy()]


def preamble_rows(vk_digest: int, instances, encoding: str = "halo2") -> tuple:
    """What every proof absorbs before its own bytes, as the kernel reads it: ((B, stride, 32) uint8 -- the digest of the verifying key,
    then the instance values column after column, 32 canonical bytes each, little-endian or for "evm" big-endian --, (B,) uint32
    counts)"""
    order = "big" if check_encoding(encoding, "preamble_rows") == "evm" else "little"
    head = int(vk_digest).to_bytes(32, order)
    rows = [head + b"".join(int(v).to_bytes(32, order) for values in inst for v in values) for inst in instances]
    counts = np.array([len(r) // 32 for r in rows], dtype=np.uint32)
    raw = np.zeros((len(rows), int(counts.max()), 32), dtype=np.uint8)
    for b, r in enumerate(rows):
        raw[b, :counts[b]] = np.frombuffer(r, dtype=np.uint8).reshape(-1, 32)
    return raw, counts


def upload_preamble(vk_digest: int, instances, device, encoding: str = "halo2"):
    """``preamble_rows`` on the device: (d_preamble, d_counts)"""
    import torch

    raw, counts = preamble_rows(vk_digest, instances, encoding)
    return torch.from_numpy(raw).to(device), torch.from_numpy(counts.view(np.int32)).to(device)


def challenges(layout, vk_digest: int, instances, d_proofs, d_ybytes, d_bad, d_records, preamble=None, d_table=None) -> None:
    """Queue the transcripts of a batch on the current stream: ``d_proofs`` (B, 32 * slots) uint8 and ``d_ybytes`` (B, points, 32) as
    ``hm_verify_read_proofs_dev`` took and left them, ``instances[b]`` the instance columns of proof b.  Challenge j of proof b --
    theta, beta, gamma, y, x, y', v, u -- goes to ``d_records[b, j]`` ((B, >= 8, 4) int64 Montgomery words; the elements behind the
    eighth are left alone).  A proof with ``d_bad[b]`` set is not hashed and gets zeros.  ``preamble``: what ``upload_preamble``
    returned, when the caller uploaded it earlier; ``d_table``: the layout's slot table on the device.  Nothing is waited for.
    With an "evm" layout the Keccak transcripts (``hm_verify_transcript_evm_dev``): the proofs are absorbed verbatim, so ``d_ybytes``
    and ``d_table`` are not looked at (None will do), and the call may be queued before the read."""
    import torch

    B = d_proofs.shape[0]
    dev = d_proofs.device
    d_pre, d_counts = preamble if preamble is not None else upload_preamble(vk_digest, instances, dev, layout.encoding)
    if layout.encoding == "evm":
        schedule = np.ascontiguousarray(layout.transcript_schedule(), dtype=np.uint32)
        _lib.check(_lib.load().hm_verify_transcript_evm_dev(_vp(d_proofs.data_ptr()), B, layout.slots, _vp(d_pre.data_ptr()),
                                                           _dev_ptr(d_counts, _u32p), d_pre.shape[1], schedule.ctypes.data_as(_u32p),
                                                           len(schedule), _dev_ptr(d_bad, _u32p), _vp(d_records.data_ptr()),
                                                           d_records.shape[1], _vp(_stream_ptr(d_records))))
        return
    if d_table is None:
        d_table = torch.from_numpy(layout.slot_table.view(np.int32)).to(dev)
    schedule = np.ascontiguousarray(layout.transcript_schedule(), dtype=np.uint32)
    _lib.check(_lib.load().hm_verify_transcript_dev(_vp(d_proofs.data_ptr()), B, _dev_ptr(d_table, _u32p), layout.slots, layout.n_points,
                                                   _vp(d_ybytes.data_ptr()), _vp(d_pre.data_ptr()), _dev_ptr(d_counts, _u32p),
                                                   d_pre.shape[1], schedule.ctypes.data_as(_u32p), len(schedule), _dev_ptr(d_bad, _u32p),
                                                   _vp(d_records.data_ptr()), d_records.shape[1], _vp(_stream_ptr(d_records))))
