"""Poseidon over BN256 Fr and the Merkle (sum) trees the reference builds from it, on the GPU (csrc/poseidon.inc over the C ABI).

What it mirrors: ``halo2_gadgets::poseidon::primitives::Hash<Fr, Spec, ConstantLength<L>, WIDTH, RATE>`` with L = RATE, as the
reference uses it -- ``MySpec<Fr, 5, 4>`` (8 full + 56 partial rounds, x^5, ``secure_mds() = 0``: src/chips/poseidon/spec.rs:16-31) for
the nodes of its Merkle sum tree (src/circuits/merkle_sum_tree.rs:118-150) and ``MySpec<Fr, 3, 2>`` for merkle_v3's plain tree.

The library takes the constants of a spec as DATA (``hm_poseidon_create``): a Rust caller hands over ``Spec::constants()`` verbatim and
``Spec.from_constants`` does the same here.  ``Spec.constants()`` restates the generator so that this package can be used on its own;
see its docstring for what that restatement rests on.

Field elements cross the GPU boundary as (…, 4) 64-bit Montgomery words, fully reduced, as everywhere in this package; the
host-integer functions (``permute``, ``hash_ints``, ``verify_path``) work on canonical Python integers.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _is_tensor, _np, _ptr, _stream_ptr, _tensor_rows, _u32p
from .arithmetic import to_host
from .bn256 import FR_MODULUS, fr_array, fr_ints

R = FR_MODULUS
words_to_ints = fr_ints          # (…, 4) uint64 Montgomery words -> canonical integers, flattened
ints_to_words = fr_array         # canonical integers -> (n, 4) uint64 Montgomery words


# ---- the constant generator ---------------------------------------------------------------------------------------------------
class _Grain:
    """The 80-bit Grain LFSR of the Poseidon paper's reference script, as halo2_gadgets' ``grain.rs`` restates it."""

    def __init__(self, width: int, r_f: int, r_p: int, field_bits: int = 254):
        bits: List[int] = []
        for value, length in ((1, 2), (0, 4), (field_bits, 12), (width, 12), (r_f, 10), (r_p, 10), ((1 << 30) - 1, 30)):
            bits += [(value >> (length - 1 - i)) & 1 for i in range(length)]        # MSB first
        self.state = bits
        self.field_bits = field_bits
        for _ in range(160):
            self._step()

    def _step(self) -> int:
        s = self.state
        new = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        s.pop(0)
        s.append(new)
        return new

    def bit(self) -> int:
        while True:                      # bits come in pairs: the second is kept when the first is 1
            first, second = self._step(), self._step()
            if first:
                return second

    def _candidate(self) -> int:
        v = 0
        for _ in range(self.field_bits):
            v = (v << 1) | self.bit()    # MSB first
        return v

    def field_element(self) -> int:
        while True:
            v = self._candidate()
            if v < R:
                return v

    def field_element_without_rejection(self) -> int:
        return self._candidate() % R


def _mat_inverse(m: List[List[int]]) -> List[List[int]]:
    n = len(m)
    a = [list(row) + [int(i == j) for j in range(n)] for i, row in enumerate(m)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col] % R)
        a[col], a[piv] = a[piv], a[col]
        inv = pow(a[col][col], -1, R)
        a[col] = [v * inv % R for v in a[col]]
        for r in range(n):
            if r != col and a[r][col]:
                f = a[r][col]
                a[r] = [(v - f * w) % R for v, w in zip(a[r], a[col])]
    return [row[n:] for row in a]


def generate_constants(width: int, r_f: int, r_p: int, secure_mds: int = 0):
    """RECALLED -- a restatement from memory of ``halo2_gadgets::poseidon::primitives::{grain, mds}::generate_constants`` at the tag
    the reference pins; no copy of that crate is at hand to compare with and no published digest of these specs is recorded in the
    reference, so nothing here is pinned against upstream.  As recalled: an 80-bit Grain LFSR seeded MSB-first with field type 1
    (2 bits), S-box 0 (4), field size 254 (12), t (12), R_F (10), R_P (10) and thirty 1-bits; feedback taps 62, 51, 38, 23, 13, 0; the
    first 160 bits discarded; output bits taken in pairs, the second kept when the first is 1; a round constant is 254 bits MSB-first,
    rejected when >= r; the MDS matrix comes from WIDTH x's and then WIDTH y's drawn WITHOUT rejection (reduced mod r), the
    candidate number ``secure_mds`` is the one kept, entry (i, j) = 1 / (x_i + y_j).

    Nothing in the library depends on this being right: the kernels take whatever constants they are given, the tests check them
    against an independent permutation on the SAME constants, and a caller who needs the reference's digests passes
    ``MySpec::constants()`` through ``Spec.from_constants``.  -> (round_constants[r][j], mds[i][j], mds_inv[i][j]) as integers."""
    g = _Grain(width, r_f, r_p)
    rc = [[g.field_element() for _ in range(width)] for _ in range(r_f + r_p)]
    select = secure_mds
    while True:
        vals = [g.field_element_without_rejection() for _ in range(2 * width)]
        xs, ys = vals[:width], vals[width:]
        if select:
            select -= 1
            continue
        break
    if any((x + y) % R == 0 for x in xs for y in ys):
        raise ValueError("generate_constants: x_i + y_j = 0, the Cauchy matrix does not exist")
    mds = [[pow((x + y) % R, -1, R) for y in ys] for x in xs]
    return rc, mds, _mat_inverse(mds)


# ---- spec ---------------------------------------------------------------------------------------------------------------------
class Spec:
    """A Poseidon instance: WIDTH, RATE = WIDTH - 1, R_F full and R_P partial rounds, x^5, and its constants."""

    def __init__(self, width: int, rate: int, r_f: int = 8, r_p: int = 56, secure_mds: int = 0):
        if width not in (3, 5) or rate != width - 1:
            raise ValueError("Spec: width must be 3 or 5 and rate = width - 1")
        if r_f % 2 or r_f + r_p <= 0:
            raise ValueError("Spec: r_f must be even and r_f + r_p positive")
        self.width, self.rate, self.r_f, self.r_p, self.secure_mds = width, rate, r_f, r_p, secure_mds
        self._constants = None
        self._handles = {}           # device index -> library handle

    @classmethod
    def from_constants(cls, width: int, rate: int, r_f: int, r_p: int, round_constants, mds) -> "Spec":
        """A spec with externally supplied constants (integers: round_constants[(r_f + r_p)][width], mds[width][width]) -- what a Rust
        caller does with ``Spec::constants()``."""
        s = cls(width, rate, r_f, r_p)
        rc = [[int(v) for v in row] for row in round_constants]
        m = [[int(v) for v in row] for row in mds]
        if len(rc) != r_f + r_p or any(len(row) != width for row in rc) or len(m) != width or any(len(row) != width for row in m):
            raise ValueError("Spec.from_constants: shapes must be (r_f + r_p, width) and (width, width)")
        if any(not 0 <= v < R for row in rc + m for v in row):
            raise ValueError("Spec.from_constants: a constant is not in [0, r)")
        s._constants = (rc, m, _mat_inverse(m))
        return s

    def constants(self):
        """(round_constants, mds, mds_inv) as integers; generated on first use (``generate_constants``: RECALLED, see there)."""
        if self._constants is None:
            self._constants = generate_constants(self.width, self.r_f, self.r_p, self.secure_mds)
        return self._constants

    def handle(self) -> int:
        """The library's handle of this spec on the current device (created on first use)."""
        lib = _lib.load()
        try:
            import torch
            key = torch.cuda.current_device() if torch.cuda.is_available() else 0
        except ImportError:
            key = 0
        if key not in self._handles:
            rc, mds, _ = self.constants()
            rc_w = ints_to_words([v for row in rc for v in row])
            mds_w = ints_to_words([v for row in mds for v in row])
            out = ctypes.c_uint64(0)
            _lib.check(lib.hm_poseidon_create(self.width, self.rate, self.r_f, self.r_p, _ptr(rc_w), _ptr(mds_w), ctypes.byref(out)))
            self._handles[key] = out.value
        return self._handles[key]

    def call(self, fn, *args) -> None:
        """``fn(handle, *args)`` checked; a handle that died with its context (``hm_shutdown``) is made again once."""
        rc = fn(ctypes.c_uint64(self.handle()), *args)
        if rc == _lib.HM_ERR_NOT_FOUND:
            self._handles = {}
            rc = fn(ctypes.c_uint64(self.handle()), *args)
        _lib.check(rc)

    def release(self) -> None:
        """Destroy the library handles of this spec (call on the device that made them; hm_shutdown frees them too)."""
        for h in self._handles.values():
            _lib.load().hm_poseidon_destroy(ctypes.c_uint64(h))
        self._handles = {}


_DEFAULT: dict = {}


def default_spec(width: int) -> Spec:
    """The reference's ``MySpec<Fr, width, width - 1>``: 8 full and 56 partial rounds, ``secure_mds = 0``."""
    if width not in _DEFAULT:
        _DEFAULT[width] = Spec(width, width - 1)
    return _DEFAULT[width]


# ---- the permutation on host integers -------------------------------------------------------------------------------------------
def permute(spec: Spec, state: Sequence[int]) -> List[int]:
    rc, mds, _ = spec.constants()
    s = [int(v) % R for v in state]
    half = spec.r_f // 2
    for r in range(spec.r_f + spec.r_p):
        s = [(a + b) % R for a, b in zip(s, rc[r])]
        if r < half or r >= half + spec.r_p:
            s = [pow(v, 5, R) for v in s]
        else:
            s[0] = pow(s[0], 5, R)
        s = [sum(m * v for m, v in zip(row, s)) % R for row in mds]
    return s


def hash_ints(spec: Spec, message: Sequence[int]) -> int:
    """``Hash::init().hash(message)`` for ``ConstantLength<RATE>``: one permutation of [message, RATE * 2^64], word 0."""
    if len(message) != spec.rate:
        raise ValueError(f"hash_ints: the message must have {spec.rate} elements")
    return permute(spec, list(message) + [spec.rate << 64])[0]


# ---- hashing on the GPU -------------------------------------------------------------------------------------------------------
def poseidon_hash(spec: Spec, msgs):
    """Digests of n messages: a GPU tensor of (n, RATE, 4) Montgomery words -> a new (n, 4) int64 tensor (asynchronous on the
    tensor's current stream)."""
    import torch

    if not _is_tensor(msgs):
        raise TypeError("poseidon_hash: a GPU tensor of (n, RATE, 4) words is expected (poseidon_hash_host takes numpy arrays)")
    n = _tensor_rows(msgs, 4 * spec.rate, "msgs")
    out = torch.empty((n, 4), dtype=torch.int64, device=msgs.device)
    with torch.cuda.device(msgs.device):
        spec.call(_lib.load().hm_poseidon_hash_bn256_fr_dev, ctypes.c_void_p(msgs.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                  ctypes.c_void_p(_stream_ptr(msgs)))
    return out


def poseidon_hash_host(spec: Spec, msgs: np.ndarray) -> np.ndarray:
    """``poseidon_hash`` on a numpy (n, RATE, 4) uint64 array through the host-pointer form: a new (n, 4) uint64 array."""
    if _is_tensor(msgs):
        raise TypeError("poseidon_hash_host takes numpy arrays (poseidon_hash takes GPU tensors)")
    m = _np(msgs, 4 * spec.rate, "msgs")
    out = np.zeros((m.shape[0], 4), dtype=np.uint64)
    spec.call(_lib.load().hm_poseidon_hash_bn256_fr, _ptr(m), m.shape[0], _ptr(out))
    return out


# ---- the plan of a tree update ------------------------------------------------------------------------------------------------
def update_plan(depth: int, indices) -> List[int]:
    """What ``tree.update(indices, ...)`` does on a tree of ``depth``, as depth + 1 counts: the live entries (distinct indices inside
    [0, 2^depth); an index outside is dropped), then the distinct touched nodes -- the hashes -- at levels 1 .. depth.  Pure host code; the
    device produces the same numbers (``return_counts=True``).  The order of the entries and their repeats do not change the counts."""
    if not 1 <= int(depth) <= 30:
        raise ValueError("update_plan: depth must be 1 .. 30")
    live = {int(i) for i in indices if 0 <= int(i) < (1 << depth)}
    return [len({i >> l for i in live}) for l in range(depth + 1)]


# ---- trees ------------------------------------------------------------------------------------------------------------------
def _depth_of(n: int, who: str) -> int:
    if n < 2 or n & (n - 1):
        raise ValueError(f"{who}: the number of leaves must be a power of two >= 2 (got {n}); pad the leaves yourself")
    return n.bit_length() - 1


class _Tree:
    """Shared by the two trees: ``nodes`` is a GPU tensor of (2n - 1, ELEMS, 4) words, level by level, leaves first, root last."""
    WIDTH = 0
    ELEMS = 0

    def __init__(self, spec: Spec, nodes, depth: int):
        self.spec, self.nodes, self.depth = spec, nodes, depth

    @classmethod
    def _build(cls, leaves, spec: Optional[Spec]):
        import torch

        spec = default_spec(cls.WIDTH) if spec is None else spec
        if spec.width != cls.WIDTH:
            raise ValueError(f"{cls.__name__}: needs a width-{cls.WIDTH} spec")
        if not _is_tensor(leaves):
            arr = _np(leaves, 4 * cls.ELEMS, "leaves")
            leaves = torch.from_numpy(arr.view(np.int64)).cuda()
        n = _tensor_rows(leaves, 4 * cls.ELEMS, "leaves")
        depth = _depth_of(n, cls.__name__)
        nodes = torch.empty((2 * n - 1, cls.ELEMS, 4), dtype=torch.int64, device=leaves.device)
        fn = _lib.load().hm_merkle_sum_tree_build_dev if cls.WIDTH == 5 else _lib.load().hm_merkle_tree_build_dev
        with torch.cuda.device(leaves.device):
            spec.call(fn, ctypes.c_void_p(leaves.data_ptr()), depth, ctypes.c_void_p(nodes.data_ptr()), ctypes.c_void_p(_stream_ptr(leaves)))
        return cls(spec, nodes, depth)

    def level_start(self, level: int) -> int:
        """Index in ``nodes`` of the first node of ``level`` (0 = leaves, depth = the root)."""
        return (2 << self.depth) - (2 << (self.depth - level))

    @property
    def root_words(self) -> np.ndarray:
        return to_host(self.nodes[-1:]).reshape(self.ELEMS, 4)

    def _sibling_words(self, indices) -> Tuple[np.ndarray, List[int]]:
        """(m, depth, ELEMS, 4) uint64 words of the sibling nodes, gathered on the GPU, and the indices as a list"""
        import torch

        idx = [int(i) for i in indices]
        if any(not 0 <= i < (1 << self.depth) for i in idx):
            raise IndexError(f"{type(self).__name__}: a leaf index is outside [0, {1 << self.depth})")
        if not idx:
            return np.zeros((0, self.depth, self.ELEMS, 4), dtype=np.uint64), idx
        d_idx = torch.tensor(idx, dtype=torch.int64, device=self.nodes.device)
        out = torch.empty((len(idx), self.depth, self.ELEMS, 4), dtype=torch.int64, device=self.nodes.device)
        with torch.cuda.device(self.nodes.device):
            _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(self.nodes.data_ptr()), self.depth, self.ELEMS,
                                                       _dev_ptr(d_idx),
                                                       len(idx), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(_stream_ptr(self.nodes))))
        return to_host(out.reshape(-1, 4)).reshape(len(idx), self.depth, self.ELEMS, 4), idx


    def update(self, indices, leaves, return_counts: bool = False):
        """Set leaf ``indices[p]`` to ``leaves[p]`` for every p, in place on ``nodes``, so that the tree equals ``build`` of the changed
        leaves: the entries count in array order (of a repeated index the last one lands) and only the nodes on their paths are hashed,
        ``sum(update_plan(depth, indices)[1:])`` hashes in all.  indices: a sequence or numpy array (an index outside [0, 2^depth)
        raises IndexError) or a GPU int64 tensor (such an index is dropped on the device); leaves: (m, ELEMS, 4) words, a GPU tensor or a
        numpy array that is uploaded, not overlapping ``nodes``.  Asynchronous on the current stream; ``return_counts=True`` synchronises
        and returns the device's depth + 1 counts (``update_plan``).  ``paths``, ``witness`` and ``root`` need no further step.

        ``update`` never switches to a rebuild by itself.  It stays faster than ``build`` while the entries are a small share of the
        leaves: the plan has ~m (depth - log2 m + 2) hashes for m scattered leaves against 2^depth, but sorts the m entries first
        (DESIGN.md section 15 has the crossover); for m near 2^depth call ``build``."""
        import torch

        dev = self.nodes.device
        if _is_tensor(indices):
            if not indices.is_cuda or indices.dtype != torch.int64:
                raise ValueError(f"{type(self).__name__}.update: an index tensor must be int64 on the GPU")
            d_idx = indices.contiguous().reshape(-1)
        else:
            idx = [int(i) for i in np.asarray(indices).reshape(-1)] if isinstance(indices, np.ndarray) else [int(i) for i in indices]
            if any(not 0 <= i < (1 << self.depth) for i in idx):
                raise IndexError(f"{type(self).__name__}.update: a leaf index is outside [0, {1 << self.depth})")
            d_idx = torch.tensor(idx, dtype=torch.int64, device=dev)
        if not _is_tensor(leaves):
            leaves = torch.from_numpy(_np(leaves, 4 * self.ELEMS, "leaves").view(np.int64)).to(dev)
        m = _tensor_rows(leaves, 4 * self.ELEMS, "leaves")
        if m != d_idx.numel():
            raise ValueError(f"{type(self).__name__}.update: {d_idx.numel()} indices but {m} leaves")
        counts = torch.zeros(self.depth + 1, dtype=torch.int32, device=dev) if return_counts else None
        fn = _lib.load().hm_merkle_sum_tree_update_dev if self.WIDTH == 5 else _lib.load().hm_merkle_tree_update_dev
        with torch.cuda.device(dev):
            self.spec.call(fn, self.depth, ctypes.c_void_p(self.nodes.data_ptr()),
                           _dev_ptr(d_idx if m else None),
                           ctypes.c_void_p(leaves.data_ptr() if m else None), m,
                           _dev_ptr(counts, _u32p),
                           ctypes.c_void_p(_stream_ptr(self.nodes)))
        if return_counts:
            return [int(v) for v in counts.cpu().tolist()]
        return None

    @classmethod
    def path_roots(cls, leaves, siblings, indices, spec: Optional[Spec] = None):
        """The roots that m inclusion paths lead to, one GPU lane per path: leaves (m, ELEMS, 4) words, siblings (m, depth, ELEMS, 4) as
        ``hm_merkle_paths_dev`` writes them, indices m integers (bit l = the path's node is the RIGHT child at level l; higher bits are
        ignored) -> (m, ELEMS, 4) words; for the sum tree a root is (hash, balance), the balance summed mod r along the path
        (``verify_path``).  GPU tensors give a GPU tensor, asynchronously on the current stream; numpy arrays go through the host form
        and give a numpy array.  Comparing with an expected root is the caller's business."""
        import torch

        spec = default_spec(cls.WIDTH) if spec is None else spec
        if spec.width != cls.WIDTH:
            raise ValueError(f"{cls.__name__}: needs a width-{cls.WIDTH} spec")
        lib, cols = _lib.load(), 4 * cls.ELEMS
        if _is_tensor(leaves) != _is_tensor(siblings):
            raise TypeError(f"{cls.__name__}.path_roots: leaves and siblings must both be GPU tensors or both numpy arrays")
        if not _is_tensor(leaves):
            lv, sb = _np(leaves, cols, "leaves"), _np(siblings, cols, "siblings")
            m = lv.shape[0]
            ix = np.ascontiguousarray(np.asarray(to_host(indices) if _is_tensor(indices) else indices).reshape(-1).astype(np.uint64))
            if m == 0 or sb.shape[0] % m or ix.shape[0] != m:
                raise ValueError(f"{cls.__name__}.path_roots: need m >= 1 leaves, m x depth siblings and m indices")
            out = np.zeros((m, cls.ELEMS, 4), dtype=np.uint64)
            spec.call(lib.hm_merkle_roots_bn256, sb.shape[0] // m, m, _ptr(lv), _ptr(sb), _ptr(ix), _ptr(out))
            return out
        m = _tensor_rows(leaves, cols, "leaves")
        rows = _tensor_rows(siblings, cols, "siblings")
        if _is_tensor(indices):
            if not indices.is_cuda or indices.dtype != torch.int64:
                raise ValueError(f"{cls.__name__}.path_roots: an index tensor must be int64 on the GPU")
            d_idx = indices.contiguous().reshape(-1)
        else:
            d_idx = torch.from_numpy(np.asarray(indices).reshape(-1).astype(np.uint64).view(np.int64)).to(leaves.device)
        if m == 0 or rows % m or d_idx.numel() != m:
            raise ValueError(f"{cls.__name__}.path_roots: need m >= 1 leaves, m x depth siblings and m indices")
        out = torch.empty((m, cls.ELEMS, 4), dtype=torch.int64, device=leaves.device)
        with torch.cuda.device(leaves.device):
            spec.call(lib.hm_merkle_roots_bn256_dev, rows // m, m, ctypes.c_void_p(leaves.data_ptr()), ctypes.c_void_p(siblings.data_ptr()),
                      _dev_ptr(d_idx), ctypes.c_void_p(out.data_ptr()),
                      ctypes.c_void_p(_stream_ptr(leaves)))
        return out


class MerkleSumTree(_Tree):
    """The reference's Merkle sum tree: a node is (hash, balance); parent.hash = H(l.hash, l.balance, r.hash, r.balance) with the
    width-5 spec, parent.balance = l.balance + r.balance.  ``build`` takes (n, 2, 4) words -- a GPU tensor, or a numpy array that is
    uploaded -- with n a power of two >= 2 (nothing is padded silently); the nodes stay on the GPU."""
    WIDTH = 5
    ELEMS = 2

    @classmethod
    def build(cls, leaves, spec: Optional[Spec] = None) -> "MerkleSumTree":
        return cls._build(leaves, spec)

    @property
    def root(self) -> Tuple[int, int]:
        """(hash, balance) of the root as canonical integers"""
        h, b = words_to_ints(self.root_words)
        return h, b

    def paths(self, indices) -> List[Tuple[List[int], List[int], List[int]]]:
        """For every leaf index: (path_element_hashes, path_element_balances, path_indices), bottom up -- the three vectors
        ``MerkleSumTreeCircuit`` takes; path_indices[l] = 1 when the node on the path is the RIGHT child at level l."""
        words, idx = self._sibling_words(indices)
        out = []
        for p, i in enumerate(idx):
            vals = words_to_ints(words[p])
            out.append((vals[0::2], vals[1::2], [(i >> l) & 1 for l in range(self.depth)]))
        return out

    def path(self, index: int) -> Tuple[List[int], List[int], List[int]]:
        return self.paths([index])[0]

    def witness(self, indices, assets_sum: int, k: int, out=None):
        """The MerkleSumTree circuit's witnesses of the inclusion paths of ``indices`` (``synthesis.merkle_sum_witness`` with the
        path's nodes read from this tree; nothing leaves the device): -> (advice (m, 20, 2^k, 4), instance (m, 4, 4)) tensors."""
        import torch

        from .synthesis import merkle_sum_witness

        idx = [int(i) for i in indices]
        if not idx or any(not 0 <= i < (1 << self.depth) for i in idx):
            raise IndexError(f"MerkleSumTree.witness: leaf indices must lie in [0, {1 << self.depth}) and there must be one at least")
        d_idx = torch.tensor(idx, dtype=torch.int64, device=self.nodes.device)
        sib = torch.empty((len(idx), self.depth, 2, 4), dtype=torch.int64, device=self.nodes.device)
        with torch.cuda.device(self.nodes.device):
            _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(self.nodes.data_ptr()), self.depth, 2,
                                                       _dev_ptr(d_idx),
                                                       len(idx), ctypes.c_void_p(sib.data_ptr()), ctypes.c_void_p(_stream_ptr(self.nodes))))
        leaves = self.nodes[d_idx].contiguous()
        return merkle_sum_witness(self.spec, leaves, sib, d_idx, assets_sum, k, nodes=self.nodes, out=out)

    @staticmethod
    def verify_path(leaf: Tuple[int, int], path, spec: Optional[Spec] = None) -> Tuple[int, int]:
        """``compute_merkle_sum_root`` on host integers: fold (hash, balance) of a leaf up its path; -> (hash, balance) of the root."""
        spec = default_spec(5) if spec is None else spec
        hashes, balances, indices = path
        h, b = int(leaf[0]) % R, int(leaf[1]) % R
        for eh, eb, bit in zip(hashes, balances, indices):
            msg = [h, b, eh, eb] if int(bit) == 0 else [eh, eb, h, b]
            h = hash_ints(spec, msg)
            b = (b + eb) % R
        return h, b


class MerkleTree(_Tree):
    """merkle_v3's plain tree: parent = H(left, right) with the width-3 spec; ``build`` takes (n, 4) words."""
    WIDTH = 3
    ELEMS = 1

    @classmethod
    def build(cls, leaves, spec: Optional[Spec] = None) -> "MerkleTree":
        return cls._build(leaves, spec)

    @property
    def root(self) -> int:
        return words_to_ints(self.root_words)[0]

    def paths(self, indices) -> List[Tuple[List[int], List[int]]]:
        """For every leaf index: (path_elements, path_indices), bottom up."""
        words, idx = self._sibling_words(indices)
        return [(words_to_ints(words[p]), [(i >> l) & 1 for l in range(self.depth)]) for p, i in enumerate(idx)]

    def path(self, index: int) -> Tuple[List[int], List[int]]:
        return self.paths([index])[0]

    def witness(self, indices, k: int, out=None):
        """The MerkleTreeV3 circuit's witnesses of the inclusion paths of ``indices`` (``synthesis.merkle_witness`` with the path's
        nodes read from this tree; nothing leaves the device): -> (advice (m, 7, 2^k, 4), instance (m, 2, 4)) tensors."""
        import torch

        from .synthesis import merkle_witness

        idx = [int(i) for i in indices]
        if not idx or any(not 0 <= i < (1 << self.depth) for i in idx):
            raise IndexError(f"MerkleTree.witness: leaf indices must lie in [0, {1 << self.depth}) and there must be one at least")
        d_idx = torch.tensor(idx, dtype=torch.int64, device=self.nodes.device)
        sib = torch.empty((len(idx), self.depth, 4), dtype=torch.int64, device=self.nodes.device)
        with torch.cuda.device(self.nodes.device):
            _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(self.nodes.data_ptr()), self.depth, 1,
                                                       _dev_ptr(d_idx),
                                                       len(idx), ctypes.c_void_p(sib.data_ptr()), ctypes.c_void_p(_stream_ptr(self.nodes))))
        leaves = self.nodes[d_idx].contiguous()
        return merkle_witness(self.spec, leaves, sib, d_idx, k, nodes=self.nodes, out=out)

    @staticmethod
    def verify_path(leaf: int, path, spec: Optional[Spec] = None) -> int:
        spec = default_spec(3) if spec is None else spec
        elements, indices = path
        h = int(leaf) % R
        for e, bit in zip(elements, indices):
            h = hash_ints(spec, [h, e] if int(bit) == 0 else [e, h])
        return h
