"""``tree.update`` against a rebuild of the changed leaves (existing code, pinned by test_poseidon_gpu.py) and against host integers, and
``path_roots`` against the tree's root and host ``verify_path``, for both trees, their default specs and one spec with other round
numbers.  Every comparison is exact on words."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import poseidon_checker as chk
from halo2_experiments_amd import _lib
from halo2_experiments_amd import poseidon as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = chk.R
HM_OK, HM_ERR_BAD_ARG, HM_ERR_NOT_FOUND = 0, -1, -4
_SPECS = {}


def _spec(width, other):
    """the default spec of the width, or one with 6 full and 10 partial rounds and random constants"""
    if (width, other) not in _SPECS:
        if other:
            rng = random.Random(600 + width)
            rc = [[rng.randrange(R) for _ in range(width)] for _ in range(16)]
            mds = [[rng.randrange(R) for _ in range(width)] for _ in range(width)]
            _SPECS[width, other] = P.Spec.from_constants(width, width - 1, 6, 10, rc, mds)
        else:
            _SPECS[width, other] = P.default_spec(width)
    return _SPECS[width, other]


TREES = [pytest.param(P.MerkleSumTree, False, id="sum"), pytest.param(P.MerkleSumTree, True, id="sum-6-10"),
         pytest.param(P.MerkleTree, False, id="plain"), pytest.param(P.MerkleTree, True, id="plain-6-10")]
DEFAULT_TREES = [pytest.param(P.MerkleSumTree, id="sum"), pytest.param(P.MerkleTree, id="plain")]


def _gpu(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _leaf_ints(rng, n, elems):
    """n leaves of `elems` integers; some balances near r so that sums wrap"""
    out = [[rng.randrange(R) for _ in range(elems)] for _ in range(n)]
    for i in range(0, n, 7):
        out[i][-1] = R - 1 - i
    return out


def _leaf_words(leaves, elems):
    w = chk.to_words([v for leaf in leaves for v in leaf])
    return w.reshape(-1, 2, 4) if elems == 2 else w.reshape(-1, 4)


def _apply(leaves, idx, new):
    out = [list(v) for v in leaves]
    for i, v in zip(idx, new):
        if 0 <= i < len(out):
            out[i] = list(v)
    return out


def _host_nodes(cls, spec, leaves):
    """every node on host integers, level by level (hash_ints)"""
    level, out = [tuple(v) for v in leaves], []
    while True:
        out += level
        if len(level) == 1:
            return out
        if cls.ELEMS == 2:
            level = [(P.hash_ints(spec, [*level[2 * i], *level[2 * i + 1]]), (level[2 * i][1] + level[2 * i + 1][1]) % R)
                     for i in range(len(level) // 2)]
        else:
            level = [(P.hash_ints(spec, [level[2 * i][0], level[2 * i + 1][0]]),) for i in range(len(level) // 2)]


def _node_ints(tree):
    vals = chk.from_words(_host(tree.nodes))
    return list(zip(vals[0::2], vals[1::2])) if tree.ELEMS == 2 else [(v,) for v in vals]


def _check_update(cls, other, depth, idx, seed, as_tensor=False):
    """update == rebuild of the changed leaves, counts == update_plan; depth <= 5: also the host integers"""
    import torch
    rng = random.Random(seed)
    spec = _spec(cls.WIDTH, other)
    leaves = _leaf_ints(rng, 1 << depth, cls.ELEMS)
    new = _leaf_ints(rng, len(idx), cls.ELEMS)
    tree = cls.build(_gpu(_leaf_words(leaves, cls.ELEMS)), spec)
    new_w = _leaf_words(new, cls.ELEMS) if idx else np.zeros((0, cls.ELEMS, 4), dtype=np.uint64)
    arg = torch.tensor(idx, dtype=torch.int64, device="cuda") if as_tensor else idx
    counts = tree.update(arg, new_w if len(idx) % 2 else _gpu(new_w), return_counts=True)      # numpy and GPU leaves alike
    assert counts == P.update_plan(depth, idx), (depth, idx[:8])
    changed = _apply(leaves, idx, new)
    rebuilt = cls.build(_gpu(_leaf_words(changed, cls.ELEMS)), spec)
    assert torch.equal(tree.nodes, rebuilt.nodes), (cls.__name__, depth, idx[:8])
    assert tree.root == rebuilt.root
    if depth <= 5:
        assert _node_ints(tree) == _host_nodes(cls, spec, changed)
    return tree, rebuilt


# ---- update equals a rebuild ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,other", TREES)
def test_update_equals_a_rebuild_small_trees(cls, other):
    _check_update(cls, other, 1, [0], 11)
    _check_update(cls, other, 1, [1], 12)
    _check_update(cls, other, 1, [1, 0], 13)
    _check_update(cls, other, 2, [2, 3], 14)                             # the two leaves of one parent
    _check_update(cls, other, 5, [15, 16], 15)                           # meet only at the root
    _check_update(cls, other, 5, [31, 15], 16)                           # differ in the top bit only
    _check_update(cls, other, 5, [6, 7, 0], 17)


@pytest.mark.parametrize("cls,other", TREES)
def test_update_equals_a_rebuild_depth_10(cls, other):
    rng = random.Random(1010)
    _check_update(cls, other, 10, rng.sample(range(1024), 300), 18)      # more than one 256-thread block, fewer than the leaves
    everyone = list(range(1024))
    rng.shuffle(everyone)
    _check_update(cls, other, 10, everyone, 19)


@pytest.mark.parametrize("cls", DEFAULT_TREES)
def test_more_entries_than_one_sorting_tile(cls):
    """4 500 entries on 4 096 leaves: the sorting network leaves its LDS tile (2 048 keys) and pads to 8 192"""
    rng = random.Random(4500)
    _check_update(cls, False, 12, [rng.randrange(4096) for _ in range(4500)], 20)


@pytest.mark.parametrize("cls,other", TREES)
def test_order_repeats_and_dropped_indices(cls, other):
    import torch
    _check_update(cls, other, 5, [9, 9, 9], 21)                          # the last of the three values lands
    _check_update(cls, other, 5, [9, 4, 9, 4, 9], 22)
    rng = random.Random(23)
    idx = rng.sample(range(1024), 260)
    idx += [rng.choice(idx) for _ in range(40)]                          # 300 entries, 40 of them repeats
    rng.shuffle(idx)
    tree, rebuilt = _check_update(cls, other, 10, idx, 24)
    rng2 = random.Random(24)                                             # the same leaves again, now one entry at a time
    spec = _spec(cls.WIDTH, other)
    leaves = _leaf_ints(rng2, 1024, cls.ELEMS)
    new = _gpu(_leaf_words(_leaf_ints(rng2, 300, cls.ELEMS), cls.ELEMS))
    single = cls.build(_gpu(_leaf_words(leaves, cls.ELEMS)), spec)
    for p, i in enumerate(idx):
        single.update([i], new[p:p + 1])
    assert torch.equal(single.nodes, tree.nodes)
    # an index >= 2^depth among valid ones (a GPU tensor: the host-side check of a sequence refuses it) changes nothing, is not counted
    _check_update(cls, other, 5, [3, 32, 7, (1 << 40) + 3, 33, 7], 25, as_tensor=True)
    _check_update(cls, other, 5, [32, 1 << 62], 26, as_tensor=True)
    with pytest.raises(IndexError):
        tree.update([1024], new[:1])
    with pytest.raises(IndexError):
        tree.update(np.array([-1]), new[:1])
    assert torch.equal(tree.nodes, rebuilt.nodes)


@pytest.mark.parametrize("cls,other", TREES)
def test_locality_only_the_touched_paths_are_written(cls, other):
    import torch
    rng = random.Random(77)
    depth, spec = 10, _spec(cls.WIDTH, other)
    # 300 of the leaves outside [512, 768): both halves of the tree are touched, and that quarter leaves every level up to 8 an
    # untouched node (300 uniform leaves of 1 024 touch every node from about level 4 upwards, which leaves nothing to mark there)
    idx = rng.sample([i for i in range(1024) if not 512 <= i < 768], 300)
    tree = cls.build(_gpu(_leaf_words(_leaf_ints(rng, 1024, cls.ELEMS), cls.ELEMS)), spec)
    marker = _gpu(_leaf_words([[123456789] * cls.ELEMS], cls.ELEMS)).reshape(cls.ELEMS, 4)  # a canonical element: it may become a child that is hashed
    marked = []
    for l in range(1, depth):                                            # one interior node off every touched path, per level
        free = sorted(set(range(1 << (depth - l))) - {i >> l for i in idx})
        if free:
            marked.append(tree.level_start(l) + rng.choice(free))
            tree.nodes[marked[-1]] = marker
    assert len(marked) == 8                                              # levels 1 .. 8; both nodes of level 9 are touched
    before = tree.nodes.clone()
    tree.update(idx, _gpu(_leaf_words(_leaf_ints(rng, 300, cls.ELEMS), cls.ELEMS)))
    touched = {tree.level_start(l) + (i >> l) for i in idx for l in range(depth + 1)}
    differs = set(torch.nonzero((tree.nodes != before).reshape(len(before), -1).any(dim=1)).flatten().tolist())
    assert differs <= touched and all(torch.equal(tree.nodes[n], marker) for n in marked)
    ints = _node_ints(tree)
    for l in range(1, depth + 1):                                        # every touched node is the hash of its children as they stand
        js = sorted({i >> l for i in idx})
        kids = torch.tensor([tree.level_start(l - 1) + 2 * j for j in js], dtype=torch.int64, device="cuda")
        at = torch.tensor([tree.level_start(l) + j for j in js], dtype=torch.int64, device="cuda")
        msgs = torch.cat([tree.nodes[kids], tree.nodes[kids + 1]], dim=1).contiguous()          # (k, RATE, 4): left, right
        assert torch.equal(P.poseidon_hash(spec, msgs), tree.nodes[at][:, 0, :]), l
        if cls.ELEMS == 2:
            for j in js:
                below = tree.level_start(l - 1) + 2 * j
                assert ints[tree.level_start(l) + j][1] == (ints[below][1] + ints[below + 1][1]) % R, (l, j)
    j = idx[0] >> 3                                                      # and one of them on host integers
    a, b = ints[tree.level_start(2) + 2 * j], ints[tree.level_start(2) + 2 * j + 1]
    exp = (P.hash_ints(spec, [*a, *b]), (a[1] + b[1]) % R) if cls.ELEMS == 2 else (P.hash_ints(spec, [a[0], b[0]]),)
    assert ints[tree.level_start(3) + j] == exp


# ---- after an update ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,other", TREES)
def test_paths_after_an_update(cls, other):
    tree, rebuilt = _check_update(cls, other, 5, [3, 17, 18, 3], 31)
    assert tree.paths(range(32)) == rebuilt.paths(range(32))


def test_sum_tree_witness_after_an_update():
    import torch
    tree, rebuilt = _check_update(P.MerkleSumTree, False, 5, [4, 21, 4, 30], 32)         # the reference's test_full_prover shape
    for a, b in zip(tree.witness([4, 30], R - 1, 9), rebuilt.witness([4, 30], R - 1, 9)):
        assert torch.equal(a, b)


def test_plain_tree_witness_after_an_update():
    import torch
    tree, rebuilt = _check_update(P.MerkleTree, False, 5, [4, 21, 4, 30], 33)
    for a, b in zip(tree.witness([21, 0], 10), rebuilt.witness([21, 0], 10)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cls", DEFAULT_TREES)
def test_no_entries_write_nothing(cls):
    import torch
    tree, _ = _check_update(cls, False, 5, [], 34)
    lib = _lib.load()
    before = tree.nodes.clone()
    fn = lib.hm_merkle_sum_tree_update_dev if cls.WIDTH == 5 else lib.hm_merkle_tree_update_dev
    assert fn(ctypes.c_uint64(tree.spec.handle()), 5, None, None, None, 0, None, None) == HM_OK
    wrong = _spec(8 - cls.WIDTH, False)                                  # the other tree's spec
    p = ctypes.c_void_p(tree.nodes.data_ptr())
    assert fn(ctypes.c_uint64(wrong.handle()), 5, p, None, None, 0, None, None) == HM_ERR_BAD_ARG
    assert b"width" in lib.hm_last_error()
    assert fn(ctypes.c_uint64(1 << 40), 5, p, None, None, 0, None, None) == HM_ERR_NOT_FOUND
    with pytest.raises(_lib.Halo2Mi355xError) as e:                      # new leaves that lie inside the nodes
        tree.update([1], tree.nodes[2:3])
    assert e.value.code == HM_ERR_BAD_ARG
    assert torch.equal(tree.nodes, before)


@pytest.mark.parametrize("cls", DEFAULT_TREES)
def test_two_updates_on_a_non_default_stream(cls):
    import torch
    rng = random.Random(35)
    spec = _spec(cls.WIDTH, False)
    leaves = _leaf_ints(rng, 1024, cls.ELEMS)
    idx1, idx2 = rng.sample(range(1024), 70), rng.sample(range(1024), 90)
    idx2[:10] = idx1[:10]                                                # the second update overwrites part of the first
    new1, new2 = _leaf_ints(rng, 70, cls.ELEMS), _leaf_ints(rng, 90, cls.ELEMS)
    tree = cls.build(_gpu(_leaf_words(leaves, cls.ELEMS)), spec)
    w1, w2 = _gpu(_leaf_words(new1, cls.ELEMS)), _gpu(_leaf_words(new2, cls.ELEMS))
    i1, i2 = (torch.tensor(v, dtype=torch.int64, device="cuda") for v in (idx1, idx2))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        tree.update(i1, w1)
        tree.update(i2, w2)
    stream.synchronize()
    rebuilt = cls.build(_gpu(_leaf_words(_apply(_apply(leaves, idx1, new1), idx2, new2), cls.ELEMS)), spec)
    assert torch.equal(tree.nodes, rebuilt.nodes)


# ---- path_roots -----------------------------------------------------------------------------------------------------------------------

def _paths_dev(tree, d_idx):
    """the siblings of the leaves d_idx as hm_merkle_paths_dev writes them, on the device"""
    import torch
    out = torch.empty((d_idx.numel(), tree.depth, tree.ELEMS, 4), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(tree.nodes.data_ptr()), tree.depth, tree.ELEMS,
                                               ctypes.cast(ctypes.c_void_p(d_idx.data_ptr()), ctypes.POINTER(ctypes.c_uint64)), d_idx.numel(),
                                               ctypes.c_void_p(out.data_ptr()), None))
    return out


@pytest.mark.parametrize("cls,other", TREES)
def test_path_roots_of_every_leaf_is_the_root(cls, other):
    import torch
    rng = random.Random(41)
    spec = _spec(cls.WIDTH, other)
    for depth in (10, 1):
        n = 1 << depth
        leaves = _leaf_ints(rng, n, cls.ELEMS)
        tree = cls.build(_gpu(_leaf_words(leaves, cls.ELEMS)), spec)
        d_idx = torch.arange(n, dtype=torch.int64, device="cuda")
        sib = _paths_dev(tree, d_idx)
        roots = cls.path_roots(tree.nodes[:n].contiguous(), sib, d_idx, spec)
        assert roots.shape == (n, cls.ELEMS, 4)
        assert torch.equal(roots, tree.nodes[-1:].expand(n, cls.ELEMS, 4))
        if cls.ELEMS == 2:
            assert chk.from_words(_host(roots[n // 2]))[1] == sum(v[1] for v in leaves) % R
        if depth == 10:
            garbage = d_idx | (torch.arange(n, dtype=torch.int64, device="cuda") << 10) | (1 << 62)      # bits above the depth are ignored
            assert torch.equal(cls.path_roots(tree.nodes[:n].contiguous(), sib, garbage, spec), roots)
            pick = torch.tensor(rng.sample(range(n), 257), dtype=torch.int64, device="cuda")            # m = 257: two blocks, one lane in the second
            got = cls.path_roots(tree.nodes[pick].contiguous(), _paths_dev(tree, pick), pick, spec)
            assert torch.equal(got, roots[:257])
            j = 100                                                      # one changed sibling word in path j: root j changes, no other
            bad = sib.clone()
            bad[j, 3].view(-1)[0] ^= 1
            got = cls.path_roots(tree.nodes[:n].contiguous(), bad, d_idx, spec)
            same = (got == roots).reshape(n, -1).all(dim=1)
            assert not bool(same[j]) and int(same.sum()) == n - 1
            lv, sb = _host(tree.nodes[:300]).reshape(300, cls.ELEMS, 4), _host(sib[:300]).reshape(300, depth, cls.ELEMS, 4)
            host = cls.path_roots(lv, sb, np.arange(300, dtype=np.uint64), spec)                        # the host form
            assert isinstance(host, np.ndarray) and np.array_equal(host, _host(roots[:300]).reshape(300, cls.ELEMS, 4))


@pytest.mark.parametrize("cls,other", TREES)
def test_path_roots_equals_host_verify_path_at_depth_5(cls, other):
    rng = random.Random(43)
    spec = _spec(cls.WIDTH, other)
    m, depth, E = 20, 5, cls.ELEMS
    leaves = _leaf_ints(rng, m, E)
    sibs = [_leaf_ints(rng, depth, E) for _ in range(m)]
    idx = [rng.randrange(32) for _ in range(m)]
    if E == 2 and not other:                                             # the reference's fixture as path 0
        with open(os.path.join(ROOT, "tests", "golden", "merkle_sum_tree_case.json")) as f:
            g = json.load(f)
        leaves[0] = [g["leaf"]["hash"], g["leaf"]["balance"]]
        sibs[0] = [[e["hash"], e["balance"]] for e in g["path_elements"]]
        idx[0] = sum(int(b) << l for l, b in enumerate(g["path_indices"]))
    sw = chk.to_words([v for path in sibs for node in path for v in node]).reshape(m, depth, E, 4)
    got = chk.from_words(_host(cls.path_roots(_gpu(_leaf_words(leaves, E).reshape(m, E, 4)), _gpu(sw), idx, spec)))
    for u in range(m):
        bits = [(idx[u] >> l) & 1 for l in range(depth)]
        if E == 2:
            exp = P.MerkleSumTree.verify_path(tuple(leaves[u]), ([s[0] for s in sibs[u]], [s[1] for s in sibs[u]], bits), spec)
            assert tuple(got[2 * u:2 * u + 2]) == exp, u
        else:
            assert got[u] == P.MerkleTree.verify_path(leaves[u][0], ([s[0] for s in sibs[u]], bits), spec), u
    if E == 2 and not other:
        assert got[1] == (100 + 10 + 50 + 60 + 90 + 90) % R                # the fixture's balances


def _pcie_bytes():
    st = _lib.Stats()
    _lib.check(_lib.load().hm_get_stats(ctypes.byref(st)))
    return np.array([st.h2d_bytes, st.d2h_bytes], dtype=np.int64)


@pytest.mark.parametrize("cls", DEFAULT_TREES)
def test_host_form_of_the_roots_counts_the_bytes_it_moves(cls):
    """hm_get_stats' h2d_bytes / d2h_bytes of hm_merkle_roots_bn256 at m = 3, depth 2: leaves, siblings and 24 bytes of indices up
    (the indices are padded in the staging buffer, not in the count), the roots down."""
    rng = random.Random(32)
    spec, elem = _spec(cls.WIDTH, False), 32 * cls.ELEMS
    leaves = _leaf_ints(rng, 4, cls.ELEMS)
    nodes = _host_nodes(cls, spec, leaves)
    idx = [2, 0, 3]
    sibs = [nodes[i ^ 1] for i in idx], [nodes[4 + ((i >> 1) ^ 1)] for i in idx]
    lv = _leaf_words([leaves[i] for i in idx], cls.ELEMS)
    sb = _leaf_words([sibs[l][p] for p in range(3) for l in range(2)], cls.ELEMS)
    b0 = _pcie_bytes()
    roots = cls.path_roots(lv, sb, np.array(idx, dtype=np.uint64), spec)
    assert (_pcie_bytes() - b0).tolist() == [3 * elem + 6 * elem + 24, 3 * elem]
    assert np.array_equal(roots.reshape(3, -1), np.tile(_leaf_words([nodes[-1]], cls.ELEMS).reshape(1, -1), (3, 1)))
