"""Poseidon over BN256 Fr, the Merkle sum tree and the plain Merkle tree on the GPU against the tests' own checker
(tests/poseidon_checker.py: naive rounds on Python integers).  Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest

import poseidon_checker as chk
from halo2_experiments_amd import _lib
from halo2_experiments_amd import poseidon as P

pytestmark = pytest.mark.gpu

R = chk.R
HM_OK, HM_ERR_BAD_ARG, HM_ERR_NOT_FOUND, HM_ERR_INTERNAL = 0, -1, -4, -5


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _gpu(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _messages(rng, n, rate):
    edge = [[0] * rate, [1] * rate, [R - 1] * rate, [R - 1] + [0] * (rate - 1), [0] * (rate - 1) + [R - 1], [1] + [R - 1] * (rate - 1)]
    msgs = [[rng.randrange(R) for _ in range(rate)] for _ in range(n)]
    for i, e in enumerate(edge[:n]):
        msgs[-1 - i] = e
    return msgs


def _words(msgs):
    return chk.to_words([v for m in msgs for v in m]).reshape(len(msgs), -1, 4)


# ---- hashing --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [3, 5])
def test_hash_equals_the_checker_device_and_host_forms(width):
    rng = random.Random(1000 + width)
    spec = P.default_spec(width)
    rc, mds, _ = spec.constants()
    for n in (1, 63, 64, 65, 4097):
        msgs = _messages(rng, n, width - 1)
        exp = [chk.digest(m, rc, mds, 8, 56) for m in msgs]
        w = _words(msgs)
        assert chk.from_words(_host(P.poseidon_hash(spec, _gpu(w)))) == exp, (width, n, "device form")
        assert chk.from_words(P.poseidon_hash_host(spec, w)) == exp, (width, n, "host form")
    assert P.poseidon_hash_host(spec, np.zeros((0, width - 1, 4), dtype=np.uint64)).shape == (0, 4)           # n = 0 is fine


@pytest.mark.parametrize("width", [3, 5])
def test_constants_are_data_a_random_spec_and_the_identity_closed_form(width):
    rng = random.Random(2000 + width)
    r_f, r_p = 6, 11
    rc = [[rng.randrange(R) for _ in range(width)] for _ in range(r_f + r_p)]
    mds = [[rng.randrange(R) for _ in range(width)] for _ in range(width)]
    spec = P.Spec.from_constants(width, width - 1, r_f, r_p, rc, mds)
    msgs = _messages(rng, 200, width - 1)
    assert chk.from_words(_host(P.poseidon_hash(spec, _gpu(_words(msgs))))) == [chk.digest(m, rc, mds, r_f, r_p) for m in msgs]
    spec.release()
    ident = [[int(i == j) for j in range(width)] for i in range(width)]
    spec = P.Spec.from_constants(width, width - 1, 8, 56, [[0] * width for _ in range(64)], ident)
    e = pow(5, 64, R - 1)
    assert chk.from_words(_host(P.poseidon_hash(spec, _gpu(_words(msgs))))) == [pow(m[0], e, R) for m in msgs]   # no hash code involved
    spec.release()


def test_handles_and_argument_errors_with_a_device():
    lib = _lib.load()
    s3, s5 = P.default_spec(3), P.default_spec(5)
    buf = _gpu(np.zeros((16, 4), dtype=np.uint64))
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.hm_merkle_sum_tree_build_dev(ctypes.c_uint64(s3.handle()), p, 1, p, None) == HM_ERR_BAD_ARG      # wrong width
    assert b"width" in lib.hm_last_error()
    assert lib.hm_merkle_tree_build_dev(ctypes.c_uint64(s5.handle()), p, 1, p, None) == HM_ERR_BAD_ARG
    host = np.zeros((8, 4), dtype=np.uint64)
    assert lib.hm_merkle_sum_tree_build(ctypes.c_uint64(s3.handle()), _u64(host), 1, _u64(host), None) == HM_ERR_BAD_ARG
    assert lib.hm_poseidon_hash_bn256_fr_dev(ctypes.c_uint64(1 << 40), p, 1, p, None) == HM_ERR_NOT_FOUND
    assert lib.hm_poseidon_destroy(ctypes.c_uint64(1 << 40)) == HM_ERR_NOT_FOUND
    assert lib.hm_poseidon_hash_bn256_fr_dev(ctypes.c_uint64(s5.handle()), None, 0, None, None) == HM_OK
    assert lib.hm_merkle_paths_dev(None, 3, 2, None, 0, None, None) == HM_OK
    fresh = P.Spec(3, 2)
    h = fresh.handle()
    fresh.release()
    assert lib.hm_poseidon_hash_bn256_fr_dev(ctypes.c_uint64(h), p, 1, p, None) == HM_ERR_NOT_FOUND             # destroyed


# ---- the sum tree ---------------------------------------------------------------------------------------------------------------

def _tree_nodes(tree):
    vals = chk.from_words(_host(tree.nodes))
    return list(zip(vals[0::2], vals[1::2])) if tree.ELEMS == 2 else vals


def test_sum_tree_every_node_depth_1_to_12():
    rng = random.Random(31)
    rc, mds, _ = P.default_spec(5).constants()
    for depth in range(1, 13):
        leaves = [(rng.randrange(R), rng.randrange(R)) for _ in range(1 << depth)]
        if depth == 3:                                                   # balances whose sums wrap around r
            leaves = [(h, R - 1 - i) for i, (h, _) in enumerate(leaves)]
        tree = P.MerkleSumTree.build(_gpu(chk.to_words([v for leaf in leaves for v in leaf]).reshape(-1, 2, 4)))
        assert tree.depth == depth
        exp = [node for level in chk.sum_tree(leaves, rc, mds, 8, 56) for node in level]
        assert _tree_nodes(tree) == exp, depth
        assert tree.root == exp[-1]
        if depth in (1, 5):                                              # the host-pointer form: root alone, then root and nodes
            lib = _lib.load()
            lw = chk.to_words([v for leaf in leaves for v in leaf])
            root = np.zeros((2, 4), dtype=np.uint64)
            nodes = np.zeros(((2 << depth) - 1, 2, 4), dtype=np.uint64)
            assert lib.hm_merkle_sum_tree_build(ctypes.c_uint64(tree.spec.handle()), _u64(lw), depth, _u64(root), None) == HM_OK
            assert tuple(chk.from_words(root)) == exp[-1]
            root[:] = 0
            assert lib.hm_merkle_sum_tree_build(ctypes.c_uint64(tree.spec.handle()), _u64(lw), depth, _u64(root), _u64(nodes)) == HM_OK
            vals = chk.from_words(nodes)
            assert list(zip(vals[0::2], vals[1::2])) == exp and tuple(chk.from_words(root)) == exp[-1]


def _random_leaves(n, elems, seed):
    from halo2_experiments_amd.arithmetic import random_fr
    return random_fr(n * elems, seed, "cuda").reshape(n, elems, 4) if elems > 1 else random_fr(n, seed, "cuda")


def test_sum_tree_depth_20():
    import torch
    rng = random.Random(20)
    depth, n = 20, 1 << 20
    spec = P.default_spec(5)
    rc, mds, _ = spec.constants()
    leaves = _random_leaves(n, 2, 77)
    near_r = chk.to_words([R - 1 - i for i in range(64)])                # balances near r in the first 64 leaves: their sums wrap
    leaves[:64, 1, :] = _gpu(near_r)
    tree = P.MerkleSumTree.build(leaves)
    nodes = _host(tree.nodes).reshape(-1, 2, 4)
    leaf_vals = chk.from_words(nodes[:n].reshape(-1, 4))
    assert tree.root[1] == sum(leaf_vals[1::2]) % R                      # the root balance is the sum of the leaves'

    def node(level, i):
        h, b = chk.from_words(nodes[tree.level_start(level) + i])
        return h, b
    for _ in range(64):                                                  # random nodes recomputed from their children
        level = rng.randrange(1, depth + 1)
        i = rng.randrange(1 << (depth - level))
        (lh, lb), (rh, rb) = node(level - 1, 2 * i), node(level - 1, 2 * i + 1)
        assert node(level, i) == (chk.digest([lh, lb, rh, rb], rc, mds, 8, 56), (lb + rb) % R), (level, i)
    assert node(6, 0)[1] == sum(R - 1 - i for i in range(64)) % R        # the wrapped sums, in closed form

    idx = [0, n - 1] + [rng.randrange(n) for _ in range(998)]
    root = tree.root
    for i, path in zip(idx, tree.paths(idx)):
        assert len(path[0]) == len(path[1]) == len(path[2]) == depth
        assert P.MerkleSumTree.verify_path(node(0, i), path) == root, i
    assert tree.path(idx[5]) == tree.paths(idx[5:6])[0]
    with pytest.raises(IndexError):
        tree.path(n)

    planted = rng.randrange(n)                                           # one changed leaf changes exactly the nodes on its path
    leaves2 = leaves.clone()
    leaves2[planted, 1, :] = _gpu(chk.to_words([12345]))[0]
    nodes2 = _host(P.MerkleSumTree.build(leaves2).nodes).reshape(-1, 2, 4)
    changed = set(np.nonzero((nodes != nodes2).any(axis=(1, 2)))[0].tolist())
    assert changed == {tree.level_start(l) + (planted >> l) for l in range(depth + 1)}
    del leaves2
    torch.cuda.empty_cache()


def test_sum_tree_depth_24_is_the_tree_of_its_depth_16_subtrees():
    import torch
    free, _total = torch.cuda.mem_get_info()
    need = 3 * (1 << 25) * 32 + (1 << 30)                                # leaves (1 GiB), nodes (2 GiB), working room
    if free < need:
        pytest.skip(f"the depth-24 tree needs {need >> 20} MiB of device memory, {free >> 20} MiB are free")
    leaves = _random_leaves(1 << 24, 2, 2424)
    whole = P.MerkleSumTree.build(leaves)
    root = whole.root
    del whole
    torch.cuda.empty_cache()
    roots = torch.empty((256, 2, 4), dtype=torch.int64, device="cuda")
    for s in range(256):
        roots[s] = P.MerkleSumTree.build(leaves[s << 16:(s + 1) << 16]).nodes[-1]
    assert P.MerkleSumTree.build(roots).root == root


# ---- the plain tree ---------------------------------------------------------------------------------------------------------------

def test_plain_tree_every_node_to_depth_12_and_depth_20_spot_checks():
    rng = random.Random(33)
    spec = P.default_spec(3)
    rc, mds, _ = spec.constants()
    for depth in range(1, 13):
        leaves = [rng.randrange(R) for _ in range(1 << depth)]
        tree = P.MerkleTree.build(_gpu(chk.to_words(leaves)))
        exp = [node for level in chk.plain_tree(leaves, rc, mds, 8, 56) for node in level]
        assert _tree_nodes(tree) == exp, depth
        assert tree.root == exp[-1]
    depth, n = 20, 1 << 20
    tree = P.MerkleTree.build(_random_leaves(n, 1, 55))
    nodes = _host(tree.nodes).reshape(-1, 4)

    def node(level, i):
        return chk.from_words(nodes[tree.level_start(level) + i])[0]
    for _ in range(64):
        level = rng.randrange(1, depth + 1)
        i = rng.randrange(1 << (depth - level))
        assert node(level, i) == chk.digest([node(level - 1, 2 * i), node(level - 1, 2 * i + 1)], rc, mds, 8, 56)
    idx = [0, n - 1] + [rng.randrange(n) for _ in range(98)]
    for i, path in zip(idx, tree.paths(idx)):
        assert P.MerkleTree.verify_path(node(0, i), path) == tree.root
    with pytest.raises(ValueError):
        P.MerkleTree.build(_gpu(chk.to_words([1, 2, 3])))                # no silent padding


# ---- fault injection (libhalo2_mi355x_fi.so) ------------------------------------------------------------------------------------

def test_fault_points_leave_the_outputs_as_they_were_and_the_next_call_works():
    fi = _lib.load_fi()
    rng = random.Random(5)
    try:
        spec = P.default_spec(5)
        rc, mds, _ = spec.constants()
        rcw, mdsw = chk.to_words([v for r in rc for v in r]), chk.to_words([v for r in mds for v in r])
        h = ctypes.c_uint64(0)
        assert fi.hm_poseidon_create(5, 4, 8, 56, _u64(rcw), _u64(mdsw), ctypes.byref(h)) == HM_OK
        msgs = _messages(rng, 40, 4)
        w = _words(msgs)
        exp = [chk.digest(m, rc, mds, 8, 56) for m in msgs]
        leaves = [(m[0], m[1]) for m in msgs[:32]]
        lw = chk.to_words([v for leaf in leaves for v in leaf])
        exp_nodes = [node for level in chk.sum_tree(leaves, rc, mds, 8, 56) for node in level]
        for point in (b"poseidon_upload", b"poseidon_download"):
            out = np.full((40, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_poseidon_hash_bn256_fr(h, _u64(w), 40, _u64(out)) == HM_ERR_INTERNAL
            assert b"injected fault at " + point in fi.hm_last_error()
            assert (out == 0xA5A5A5A5A5A5A5A5).all()
            assert fi.hm_poseidon_hash_bn256_fr(h, _u64(w), 40, _u64(out)) == HM_OK
            assert chk.from_words(out) == exp
            root = np.full((2, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            nodes = np.full((63, 2, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_merkle_sum_tree_build(h, _u64(lw), 5, _u64(root), _u64(nodes)) == HM_ERR_INTERNAL
            assert (root == 0x5A5A5A5A5A5A5A5A).all() and (nodes == 0x5A5A5A5A5A5A5A5A).all()
            assert fi.hm_merkle_sum_tree_build(h, _u64(lw), 5, _u64(root), _u64(nodes)) == HM_OK
            vals = chk.from_words(nodes)
            assert list(zip(vals[0::2], vals[1::2])) == exp_nodes and tuple(chk.from_words(root)) == exp_nodes[-1]
        # hm_device_malloc's give-back (an exhausted device: caches are dropped) must not free a live spec
        from halo2_experiments_amd.domain import EvaluationDomain, fr_words
        d = EvaluationDomain(7, 10)
        a = chk.to_words([rng.randrange(R) for _ in range(d.n)])
        assert fi.hm_ntt_bn256_fr(_u64(a), _u64(fr_words(d.omega)), d.k) == HM_OK          # a twiddle set: something to give back
        fi.hm_test_arm_fault(b"device_malloc_oom", 0)
        p = ctypes.c_void_p(0)
        assert fi.hm_device_malloc(1 << 20, ctypes.byref(p)) == HM_OK and p.value          # the retry, after the caches gave back
        out = np.zeros((40, 4), dtype=np.uint64)
        assert fi.hm_poseidon_hash_bn256_fr(h, _u64(w), 40, _u64(out)) == HM_OK
        assert chk.from_words(out) == exp
        assert fi.hm_device_free(p) == HM_OK
        assert fi.hm_poseidon_destroy(h) == HM_OK
    finally:
        fi.hm_test_arm_fault(None, 0)


def _pcie_bytes():
    st = _lib.Stats()
    _lib.check(_lib.load().hm_get_stats(ctypes.byref(st)))
    return np.array([st.h2d_bytes, st.d2h_bytes], dtype=np.int64)


def test_host_forms_count_the_bytes_they_move():
    """hm_get_stats' h2d_bytes / d2h_bytes: hm_poseidon_hash_bn256_fr at n = 3 for both widths, hm_merkle_sum_tree_build at depth 2
    with the root alone (64 bytes come back) and with every node (the root is then counted with them and once more on its own)."""
    lib = _lib.load()
    rng = random.Random(3)
    for width in (3, 5):
        spec = P.default_spec(width)
        rc, mds, _ = spec.constants()
        msgs = _messages(rng, 3, width - 1)
        b0 = _pcie_bytes()
        got = P.poseidon_hash_host(spec, _words(msgs))
        assert (_pcie_bytes() - b0).tolist() == [3 * (width - 1) * 32, 3 * 32]
        assert chk.from_words(got) == [chk.digest(m, rc, mds, 8, 56) for m in msgs]
    spec = P.default_spec(5)
    rc, mds, _ = spec.constants()
    leaves = [(rng.randrange(R), rng.randrange(R)) for _ in range(4)]
    exp = [node for level in chk.sum_tree(leaves, rc, mds, 8, 56) for node in level]
    lw = chk.to_words([v for leaf in leaves for v in leaf])
    root, nodes = np.zeros((2, 4), dtype=np.uint64), np.zeros((7, 2, 4), dtype=np.uint64)
    b0 = _pcie_bytes()
    assert lib.hm_merkle_sum_tree_build(ctypes.c_uint64(spec.handle()), _u64(lw), 2, _u64(root), None) == HM_OK
    assert (_pcie_bytes() - b0).tolist() == [4 * 64, 64] and tuple(chk.from_words(root)) == exp[-1]
    root[:] = 0
    b0 = _pcie_bytes()
    assert lib.hm_merkle_sum_tree_build(ctypes.c_uint64(spec.handle()), _u64(lw), 2, _u64(root), _u64(nodes)) == HM_OK
    assert (_pcie_bytes() - b0).tolist() == [4 * 64, 64 + 7 * 64]
    vals = chk.from_words(nodes)
    assert list(zip(vals[0::2], vals[1::2])) == exp and tuple(chk.from_words(root)) == exp[-1]
