"""What the tests of the EVM encoding share (tests/test_evm_proofs_host.py, tests/test_evm_proofs_gpu.py): a proof of one encoding
written in the other -- the same points and scalars, other bytes; it reads, and hashes to other challenges, so it does not verify --,
the ways a proof's bytes are tampered with, and the circuits."""
from halo2_experiments_amd import batch_verifier as bvm
from halo2_experiments_amd.bn256 import FQ_MODULUS as P
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.transcript import g1_compress_int

CASES = ["poseidon_k6", "merkle_v3_d5_k8", "merkle_sum_d5_k9"]     # the smallest with lookups, several permutation sets and instances


def to_evm(lay_halo2, proof: bytes) -> bytes:
    """a "halo2" proof's points and scalars in the "evm" encoding, slot for slot"""
    out = bytearray()
    points, scalars = bvm.read_proof_ints(lay_halo2, proof)
    points, scalars = iter(points), iter(scalars)
    for entry in lay_halo2.slot_table:
        if int(entry) & bvm.VR_POINT:
            x, y = next(points)
            out += x.to_bytes(32, "big") + y.to_bytes(32, "big")
        else:
            out += next(scalars).to_bytes(32, "big")
    return bytes(out)


def to_halo2(lay_evm, proof: bytes) -> bytes:
    """the reverse: an "evm" proof's points compressed, its scalars little-endian"""
    out = bytearray()
    points, scalars = bvm.read_proof_ints(lay_evm, proof)
    points, scalars = iter(points), iter(scalars)
    for entry in lay_evm.slot_table:
        if int(entry) & bvm.EVM_POINT:
            out += g1_compress_int(next(points))
        elif not int(entry) & bvm.EVM_SKIP:
            out += next(scalars).to_bytes(32, "little")
    return bytes(out)


def put(proof: bytes, slot: int, value: int) -> bytes:
    """the proof with 32-byte slot `slot` holding `value`, big-endian"""
    return proof[:32 * slot] + value.to_bytes(32, "big") + proof[32 * slot + 32:]


def tampers(lay_evm, proof: bytes) -> dict:
    """name -> a proof the read refuses: x >= p, y >= p, a flipped low bit of y, a zeroed point, a scalar >= r; and the same on the
    tail and on the last own point, where the table's other entries stand"""
    xs, ss = lay_evm.point_slots, lay_evm.scalar_slots
    at = lambda s: int.from_bytes(proof[32 * s:32 * s + 32], "big")
    x1, x2, x3, x4 = xs[0], xs[len(xs) // 2], xs[-1], xs[-2]
    return {
        "x >= p": put(proof, x1, at(x1) + P),
        "y >= p": put(proof, x2 + 1, at(x2 + 1) + P),
        "low bit of y": put(proof, x2 + 1, at(x2 + 1) ^ 1),
        "zero point": put(put(proof, x1, 0), x1 + 1, 0),
        "scalar >= r": put(proof, ss[len(ss) // 2], R),
        "last scalar = 2^256 - 1": put(proof, ss[-1], 2 ** 256 - 1),
        "tail off the curve": put(proof, x3 + 1, at(x3 + 1) ^ 1),
        "[h] x = p": put(proof, x4, P),
    }
