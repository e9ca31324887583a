"""The MerkleSumTree witness on the GPU (csrc/poseidon.hip: merkle_witness_kernel<2> / merkle_chain_kernel<2>) against
synthesis.assign_ints word for word, against the tests' MockProver, and against the gate polynomials of
circuits.merkle_sum_tree(spec) run by the device GraphEvaluator over every user's columns."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from halo2_experiments_amd import _lib, circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R
from halo2_experiments_amd.evaluation import GraphEvaluator

import mock_prover

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HM_OK, HM_ERR_BAD_ARG, HM_ERR_INTERNAL = 0, -1, -5
FILL = 0x5A5A5A5A5A5A5A5A


def _gpu(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def _columns(t):
    """(columns, n, 4) tensor -> integer columns"""
    return [_ints(c) for c in t]


def golden():
    with open(os.path.join(HERE, "golden", "merkle_sum_tree_case.json")) as f:
        g = json.load(f)
    return (g["leaf"]["hash"], g["leaf"]["balance"]), [(e["hash"], e["balance"]) for e in g["path_elements"]], list(g["path_indices"])


def _path_tensors(leaf, sib, bits):
    leaves = _gpu(ps.ints_to_words(list(leaf)).reshape(1, 2, 4))
    sibs = _gpu(ps.ints_to_words([v for p in sib for v in p]).reshape(1, len(sib), 2, 4))
    idx = torch.tensor([sum(int(b) << l for l, b in enumerate(bits))], dtype=torch.int64, device="cuda")
    return leaves, sibs, idx


class GateCheck:
    """Every gate of the constraint system as a program of its own on the device GraphEvaluator (rotations unscaled, 2^k rows,
    no permutation / lookup argument): rows(...) -> {gate name: usable rows where it does not vanish}."""

    def __init__(self, cs, lay):
        self.cs, self.lay = cs, lay
        self.fixed = [c.contiguous() for c in _gpu(sy.columns_to_words(lay.fixed_columns()))]
        g = GraphEvaluator()
        g.add_custom_gates(cs.polynomials())
        self.all = g.compile(cs.num_fixed, cs.num_advice, cs.num_instance)
        self.per_gate = {}
        for name, polys in cs.gates:
            g = GraphEvaluator()
            g.add_custom_gates(polys)
            self.per_gate[name] = g.compile(cs.num_fixed, cs.num_advice, cs.num_instance)
        self.y = random.Random(99).randrange(R)

    def instance_column(self, inst):
        col = torch.zeros((self.lay.n, 4), dtype=torch.int64, device="cuda")
        col[:4] = inst
        return col

    def _run(self, prog, adv, inst):
        values = torch.zeros((self.lay.n, 4), dtype=torch.int64, device="cuda")
        prog.evaluate(self.fixed + [adv[c] for c in range(sy.N_ADVICE)] + [self.instance_column(inst)], values, y=self.y)
        return values[: self.lay.n - sy.BLINDING_ROWS]

    def satisfied(self, adv, inst) -> bool:
        return not bool(self._run(self.all, adv, inst).any())

    def rows(self, adv, inst):
        out = {}
        for name, prog in self.per_gate.items():
            bad = self._run(prog, adv, inst).ne(0).any(dim=1).nonzero().flatten().tolist()
            if bad:
                out[name] = bad
        return out


@pytest.fixture(scope="module")
def spec():
    return ps.default_spec(5)


def test_golden_case_word_for_word_both_sources_and_host_form(spec):
    leaf, sib, bits = golden()
    lay = sy.MerkleSumTreeLayout(5, 9, spec)
    exp = sy.columns_to_words(lay.assign_ints(leaf, sib, bits, 500))
    root = ps.MerkleSumTree.verify_path(leaf, ([h for h, _ in sib], [b for _, b in sib], bits), spec)
    exp_inst = ps.ints_to_words([leaf[0], leaf[1], root[0], 500])
    leaves, sibs, idx = _path_tensors(leaf, sib, bits)
    out = torch.full((1, sy.N_ADVICE, 512, 4), FILL, dtype=torch.int64, device="cuda")      # every word must be written
    adv, inst = sy.merkle_sum_witness(spec, leaves, sibs, idx, 500, 9, out=out)
    assert adv.data_ptr() == out.data_ptr()
    assert np.array_equal(adv[0].cpu().numpy().view(np.uint64), exp)
    assert np.array_equal(inst[0].cpu().numpy().view(np.uint64), exp_inst)
    h_adv, h_inst = sy.merkle_sum_witness_host(spec, leaves.cpu().numpy().view(np.uint64), sibs.cpu().numpy().view(np.uint64),
                                               idx.cpu().numpy().view(np.uint64), 500, 9)
    assert np.array_equal(h_adv[0], exp) and np.array_equal(h_inst[0], exp_inst)
    # a path with right-hand positions, at depth 1 too
    bits2 = [1, 0, 1, 1, 0]
    leaves, sibs, idx = _path_tensors(leaf, sib, bits2)
    adv, _ = sy.merkle_sum_witness(spec, leaves, sibs, idx, 200, 9)
    assert np.array_equal(adv[0].cpu().numpy().view(np.uint64), sy.columns_to_words(lay.assign_ints(leaf, sib, bits2, 200)))
    lay1 = sy.MerkleSumTreeLayout(1, 9, spec)
    leaves, sibs, idx = _path_tensors(leaf, sib[:1], [1])
    adv, _ = sy.merkle_sum_witness(spec, leaves, sibs, idx, 500, 9)
    assert np.array_equal(adv[0].cpu().numpy().view(np.uint64), sy.columns_to_words(lay1.assign_ints(leaf, sib[:1], [1], 500)))


@pytest.fixture(scope="module")
def batch(spec):
    depth, m, k = 12, 1024, 10
    rng = random.Random(2024)
    n = 1 << depth
    leaves = [(rng.randrange(R), rng.randrange(1 << 40)) for _ in range(n)]
    tree = ps.MerkleSumTree.build(_gpu(ps.ints_to_words([v for leaf in leaves for v in leaf]).reshape(n, 2, 4)), spec)
    idx = [0, n - 1] + [rng.randrange(n) for _ in range(m - 2)]
    assets = 1 << 60
    adv, inst = tree.witness(idx, assets, k)
    torch.cuda.synchronize()
    lay = sy.MerkleSumTreeLayout(depth, k, spec)
    cs = circuits.merkle_sum_tree(spec)
    return dict(depth=depth, m=m, k=k, rng=rng, leaves=leaves, tree=tree, idx=idx, assets=assets, adv=adv, inst=inst, lay=lay, cs=cs,
                check=GateCheck(cs, lay))


def test_batch_every_user_satisfies_the_gates(batch):
    chk = batch["check"]
    bad = [u for u in range(batch["m"]) if not chk.satisfied(batch["adv"][u], batch["inst"][u])]
    assert bad == []
    # the check is not blind: one changed state word of one user is seen
    adv = batch["adv"][7].clone()
    adv[sy.STATE[1], batch["lay"].perm_row(3) + 10, 0] ^= 1
    assert not chk.satisfied(adv, batch["inst"][7])
    assert set(chk.rows(adv, batch["inst"][7])) == {"partial rounds"}


def test_batch_roots_and_lt_bytes(batch):
    lay, adv, inst, tree = batch["lay"], batch["adv"], batch["inst"], batch["tree"]
    root_hash, root_balance = tree.root
    total = sum(b for _, b in batch["leaves"])
    assert root_balance == total and total < batch["assets"]
    kind, col, row = lay.digest_cell(lay.depth - 1)
    assert set(_ints(adv[:, col, row])) == {root_hash}
    assert set(_ints(inst[:, 2])) == {root_hash} and set(_ints(inst[:, 3])) == {batch["assets"]}
    assert _ints(inst[:, 0]) == [batch["leaves"][i][0] for i in batch["idx"]]
    assert _ints(inst[:, 1]) == [batch["leaves"][i][1] for i in batch["idx"]]
    assert set(_ints(adv[:, sy.A, lay.lt_row])) == {total} and set(_ints(adv[:, sy.LT, lay.lt_row])) == {1}
    diff = [_ints(adv[:, c, lay.lt_row]) for c in sy.DIFF]
    for u in range(batch["m"]):
        assert all(0 <= diff[i][u] < 256 for i in range(8))
        assert sum(diff[i][u] << (8 * i) for i in range(8)) == total - batch["assets"] + (1 << 64)


def test_batch_sixteen_users_word_for_word_and_mock_prover(batch):
    lay, cs, tree = batch["lay"], batch["cs"], batch["tree"]
    users = [0, 1] + batch["rng"].sample(range(2, batch["m"]), 14)
    fixed = lay.fixed_columns()
    paths = tree.paths([batch["idx"][u] for u in users])
    for u, (hashes, balances, bits) in zip(users, paths):
        leaf = batch["leaves"][batch["idx"][u]]
        exp = lay.assign_ints(leaf, list(zip(hashes, balances)), bits, batch["assets"])
        assert np.array_equal(batch["adv"][u].cpu().numpy().view(np.uint64), sy.columns_to_words(exp)), u
        got = _columns(batch["adv"][u])
        inst_col = [0] * lay.n
        inst_col[:4] = _ints(batch["inst"][u])
        rows = [r for reg in lay.regions if reg.name != "load u8 range check table" and reg.name != "constants" for r in reg.rows]
        assert mock_prover.verify(cs, fixed, got, [inst_col], lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS,
                                  rows=rows + [lay.used_rows, lay.n - 7]) == [], u


def test_batch_without_the_tree_gives_identical_bytes(batch, spec):
    tree, idx = batch["tree"], batch["idx"]
    d_idx = torch.tensor(idx, dtype=torch.int64, device="cuda")
    sib = torch.empty((len(idx), tree.depth, 2, 4), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().hm_merkle_paths_dev(ctypes.c_void_p(tree.nodes.data_ptr()), tree.depth, 2,
                                               ctypes.cast(ctypes.c_void_p(d_idx.data_ptr()), ctypes.POINTER(ctypes.c_uint64)), len(idx),
                                               ctypes.c_void_p(sib.data_ptr()), None))
    torch.cuda.synchronize()
    adv, inst = sy.merkle_sum_witness(spec, tree.nodes[d_idx].contiguous(), sib, d_idx, batch["assets"], batch["k"])
    assert torch.equal(adv, batch["adv"]) and torch.equal(inst, batch["inst"])


def test_unsatisfiable_inputs_are_filled_and_fail_where_they_should(batch, spec):
    lay5 = sy.MerkleSumTreeLayout(5, 9, spec)
    cs = batch["cs"]
    chk5 = GateCheck(cs, lay5)
    leaf, sib, bits = golden()
    for sibs, assets, must in ((sib, 200, {"check == is_lt"}), ([(1, 1 << 65)] + sib[1:], 500, {"lt gate", "check == is_lt"})):
        leaves, d_sib, idx = _path_tensors(leaf, sibs, bits)
        adv, inst = sy.merkle_sum_witness(spec, leaves, d_sib, idx, assets, 9)
        exp = lay5.assign_ints(leaf, sibs, bits, assets)
        assert np.array_equal(adv[0].cpu().numpy().view(np.uint64), sy.columns_to_words(exp))
        assert chk5.rows(adv[0], inst[0]) == {name: [lay5.lt_row] for name in must}
        inst_col = [0] * lay5.n
        inst_col[:4] = _ints(inst[0])
        failures = mock_prover.verify(cs, lay5.fixed_columns(), _columns(adv[0]), [inst_col], lay5.copies(), lay5.n, lay5.n - sy.BLINDING_ROWS)
        assert failures and all(f[0] == "gate" and f[3] == lay5.lt_row for f in failures)
        assert set(mock_prover.gate_names(failures)) == must
        cpu = mock_prover.verify(cs, lay5.fixed_columns(), exp, [inst_col], lay5.copies(), lay5.n, lay5.n - sy.BLINDING_ROWS)
        assert cpu == failures
    # the batch from the tree with assets below the total: every user fails at the less-than row only
    adv, inst = batch["tree"].witness(batch["idx"][:8], 1 << 30, batch["k"])
    for u in range(8):
        assert batch["check"].rows(adv[u], inst[u]) == {"check == is_lt": [batch["lay"].lt_row]}


def _sparse_columns_to_words(cols):
    """sy.columns_to_words, converting the non-zero cells only (zero is four zero words): most of a witness is unassigned"""
    out = np.zeros((len(cols), len(cols[0]), 4), dtype=np.uint64)
    for c, col in enumerate(cols):
        rows = [r for r, v in enumerate(col) if v]
        if rows:
            out[c, rows] = ps.ints_to_words([col[r] for r in rows])
    return out


@pytest.mark.parametrize("depth,m,k,with_tree", [(1, 1, 9, True), (1, 257, 9, True), (1, 257, 9, False), (2, 129, 9, True),
                                                 (2, 129, 9, False), (3, 86, 9, False)])
def test_smallest_shapes(spec, depth, m, k, with_tree):
    """depth 1: the lane of level 0 is also the lane of the last level and the chain has nothing to do; depth 2 without a tree is the
    shortest chain; m * depth = 257 and 258 cross one workgroup of 256 lanes.  Every word of every user's columns and instance."""
    lay = sy.MerkleSumTreeLayout(depth, k, spec)
    rng = random.Random(100 * depth + m)
    assets = 1 << 60
    if with_tree:
        n = 1 << depth
        tree_leaves = [(rng.randrange(R), rng.randrange(1 << 40)) for _ in range(n)]
        tree = ps.MerkleSumTree.build(_gpu(ps.ints_to_words([v for leaf in tree_leaves for v in leaf]).reshape(n, 2, 4)), spec)
        index = [rng.randrange(n) for _ in range(m)]
        paths = [(tree_leaves[i], list(zip(hashes, balances)), bits) for i, (hashes, balances, bits) in zip(index, tree.paths(index))]
        nodes = tree.nodes
    else:
        paths = [((rng.randrange(R), rng.randrange(1 << 40)), [(rng.randrange(R), rng.randrange(1 << 40)) for _ in range(depth)],
                  [rng.randrange(2) for _ in range(depth)]) for _ in range(m)]
        paths[0] = (paths[0][0], paths[0][1], [1] * depth)
        nodes = None
    leaves = _gpu(ps.ints_to_words([v for leaf, _, _ in paths for v in leaf]).reshape(m, 2, 4))
    sibs = _gpu(ps.ints_to_words([v for _, sib, _ in paths for e in sib for v in e]).reshape(m, depth, 2, 4))
    idx = torch.tensor([sum(b << l for l, b in enumerate(bits)) for _, _, bits in paths], dtype=torch.int64, device="cuda")
    out = torch.full((m, sy.N_ADVICE, 1 << k, 4), FILL, dtype=torch.int64, device="cuda")
    adv, inst = sy.merkle_sum_witness(spec, leaves, sibs, idx, assets, k, nodes=nodes, out=out)
    got, got_inst = adv.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64)
    for u, (leaf, sib, bits) in enumerate(paths):
        assert np.array_equal(got[u], _sparse_columns_to_words(lay.assign_ints(leaf, sib, bits, assets))), u
        root = ps.MerkleSumTree.verify_path(leaf, ([h for h, _ in sib], [b for _, b in sib], bits), spec)
        assert np.array_equal(got_inst[u], ps.ints_to_words(lay.instance(leaf, root[0], assets)[0][:4])), u
    if with_tree:
        assert set(_ints(inst[:, 2])) == {tree.root[0]}


def test_permutation_columns_on_the_device(spec):
    lay = sy.MerkleSumTreeLayout(5, 9, spec)
    cs = circuits.merkle_sum_tree(spec)
    dom = EvaluationDomain(4, 9)
    delta = pow(7, 1 << 28, R)
    got = sy.permutation_columns(cs, lay, dom.omega, delta)
    torch.cuda.synchronize()
    assert _columns(got) == sy.permutation_columns_ints(cs, lay, dom.omega, delta)


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def test_rejected_arguments_leave_the_output_untouched(spec):
    lib = _lib.load()
    leaf, sib, bits = golden()
    leaves, sibs, idx = _path_tensors(leaf, sib, bits)
    adv = torch.full((1, sy.N_ADVICE, 512, 4), FILL, dtype=torch.int64, device="cuda")
    inst = torch.full((1, 4, 4), FILL, dtype=torch.int64, device="cuda")
    assets = np.ascontiguousarray(ps.ints_to_words([500])[0])
    h5, h3 = spec.handle(), ps.default_spec(3).handle()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    I = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_uint64)) if t is not None else None

    class Shifted:                                                # a tensor's address moved by `off` bytes (never dereferenced)
        def __init__(self, t, off):
            self.data_ptr = lambda: t.data_ptr() + off

    def call(handle=h5, depth=5, log_n=9, lv=leaves, sb=sibs, ix=idx, a=assets, nodes=None, out=adv, ins=inst):
        return lib.hm_merkle_sum_witness_bn256_dev(handle, depth, log_n, 1, P(lv), P(sb), I(ix), _u64(a) if a is not None else None, P(nodes),
                                                   P(out), P(ins), None)

    assert call(handle=h3) == HM_ERR_BAD_ARG                      # a width-3 spec
    assert call(handle=987654321) == -4                           # HM_ERR_NOT_FOUND
    assert call(depth=0) == HM_ERR_BAD_ARG and call(depth=33, log_n=12) == HM_ERR_BAD_ARG
    assert call(log_n=7) == HM_ERR_BAD_ARG and call(log_n=8) == HM_ERR_BAD_ARG and call(log_n=25) == HM_ERR_BAD_ARG
    assert call(depth=20, log_n=9) == HM_ERR_BAD_ARG              # 963 rows do not fit 2^9 - 6
    assert b"963" in lib.hm_last_error()
    assert call(depth=31, log_n=11, nodes=adv) == HM_ERR_BAD_ARG  # a built tree has depth <= 30
    for kw in ("lv", "sb", "ix", "a", "out", "ins"):
        assert call(**{kw: None}) == HM_ERR_BAD_ARG, kw
    for kw, t, off in (("lv", leaves, 8), ("sb", sibs, 8), ("out", adv, 8), ("ins", inst, 8), ("nodes", adv, 8), ("ix", idx, 4)):
        assert call(**{kw: Shifted(t, off)}) == HM_ERR_BAD_ARG and b"aligned" in lib.hm_last_error(), kw     # the lanes move 16-byte vectors
    too_many = ((1 << 31) // 5) + 1                               # m * depth > 2^31: refused before any pointer is read
    assert lib.hm_merkle_sum_witness_bn256_dev(h5, 5, 9, too_many, P(leaves), P(sibs), I(idx), _u64(assets), None, P(adv), P(inst), None) == HM_ERR_BAD_ARG
    assert b"2^31" in lib.hm_last_error()
    torch.cuda.synchronize()
    assert bool((adv == FILL).all()) and bool((inst == FILL).all())
    tree8 = ps.MerkleSumTree.build(_gpu(ps.ints_to_words(list(range(32))).reshape(16, 2, 4)), spec)      # depth 4: too small for a depth-5 path
    with pytest.raises(ValueError, match="nodes"):
        sy.merkle_sum_witness(spec, leaves, sibs, idx, 500, 9, nodes=tree8.nodes)
    with pytest.raises(ValueError, match="nodes"):
        sy.merkle_sum_witness(spec, leaves, sibs, idx, 500, 9, nodes=tree8.nodes.cpu())
    h_adv = np.full((1, sy.N_ADVICE, 512, 4), FILL, dtype=np.uint64)
    h_inst = np.full((1, 4, 4), FILL, dtype=np.uint64)
    lv, sb, ix = (t.cpu().numpy().view(np.uint64) for t in (leaves, sibs, idx))
    host = lambda handle=h5, depth=5, log_n=9, m=1, lv=lv: lib.hm_merkle_sum_witness_bn256(
        handle, depth, log_n, m, _u64(lv) if lv is not None else None, _u64(sb), _u64(ix), _u64(assets), _u64(h_adv), _u64(h_inst))
    assert host(handle=h3) == HM_ERR_BAD_ARG and host(depth=0) == HM_ERR_BAD_ARG and host(log_n=8) == HM_ERR_BAD_ARG
    assert host(lv=None) == HM_ERR_BAD_ARG
    assert host(m=100000) == HM_ERR_BAD_ARG and b"256 MiB" in lib.hm_last_error()
    assert (h_adv == FILL).all() and (h_inst == FILL).all()
    rows, n_adv = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert lib.hm_merkle_sum_witness_layout(8, 56, 5, 9, None, ctypes.byref(n_adv), None) == HM_ERR_BAD_ARG
    assert lib.hm_merkle_sum_witness_layout(8, 55, 5, 9, ctypes.byref(rows), ctypes.byref(n_adv), None) == HM_ERR_BAD_ARG
    assert (rows.value, n_adv.value) == (7, 7)
    assert call() == HM_OK                                        # and the same arguments, valid, work
    torch.cuda.synchronize()
    assert not bool((adv == FILL).any())


def test_fault_points_of_the_host_form(spec):
    fi = _lib.load_fi()
    try:
        rc, mds, _ = spec.constants()
        h = ctypes.c_uint64(0)
        assert fi.hm_poseidon_create(5, 4, 8, 56, _u64(ps.ints_to_words([v for r in rc for v in r])),
                                     _u64(ps.ints_to_words([v for r in mds for v in r])), ctypes.byref(h)) == HM_OK
        leaf, sib, bits = golden()
        lay = sy.MerkleSumTreeLayout(5, 9, spec)
        exp = sy.columns_to_words(lay.assign_ints(leaf, sib, bits, 500))
        lv = ps.ints_to_words(list(leaf))
        sb = ps.ints_to_words([v for p in sib for v in p])
        ix = np.zeros(1, dtype=np.uint64)
        assets = np.ascontiguousarray(ps.ints_to_words([500])[0])
        for point in (b"witness_upload", b"witness_download"):
            adv = np.full((1, sy.N_ADVICE, 512, 4), FILL, dtype=np.uint64)
            inst = np.full((1, 4, 4), FILL, dtype=np.uint64)
            fi.hm_test_arm_fault(point, 0)
            assert fi.hm_merkle_sum_witness_bn256(h, 5, 9, 1, _u64(lv), _u64(sb), _u64(ix), _u64(assets), _u64(adv), _u64(inst)) == HM_ERR_INTERNAL
            assert b"injected fault at " + point in fi.hm_last_error()
            assert (adv == FILL).all() and (inst == FILL).all()
            assert fi.hm_merkle_sum_witness_bn256(h, 5, 9, 1, _u64(lv), _u64(sb), _u64(ix), _u64(assets), _u64(adv), _u64(inst)) == HM_OK
            assert np.array_equal(adv[0], exp)
        assert fi.hm_poseidon_destroy(h) == HM_OK
    finally:
        fi.hm_test_arm_fault(None, 0)


def _pcie_bytes():
    st = _lib.Stats()
    _lib.check(_lib.load().hm_get_stats(ctypes.byref(st)))
    return np.array([st.h2d_bytes, st.d2h_bytes], dtype=np.int64)


def _smallest_k(layout, *args):
    """the smallest log_n the layout call accepts"""
    rows, n_adv = ctypes.c_uint32(), ctypes.c_uint32()
    return next(k for k in range(1, 25) if layout(*args, k, ctypes.byref(rows), ctypes.byref(n_adv), None) == HM_OK)


def test_host_form_counts_the_bytes_it_moves(spec):
    """hm_get_stats' h2d_bytes / d2h_bytes of hm_merkle_sum_witness_bn256 at m = 3, depth 2 and the smallest 2^k the layout accepts:
    leaves, siblings and 24 bytes of indices up (padded to 64 in the staging buffer, not in the count), columns and instance down;
    the columns equal the device form's."""
    k = _smallest_k(_lib.load().hm_merkle_sum_witness_layout, 8, 56, 2)
    rng = random.Random(23)
    leaves = _gpu(ps.ints_to_words([rng.randrange(R) if e == 0 else rng.randrange(1 << 20) for _ in range(3) for e in range(2)]).reshape(3, 2, 4))
    sibs = _gpu(ps.ints_to_words([rng.randrange(R) if e == 0 else rng.randrange(1 << 20) for _ in range(6) for e in range(2)]).reshape(3, 2, 2, 4))
    idx = torch.tensor([2, 0, 3], dtype=torch.int64, device="cuda")
    adv, inst = sy.merkle_sum_witness(spec, leaves, sibs, idx, 1 << 40, k)
    host = lambda t: t.cpu().numpy().view(np.uint64)
    b0 = _pcie_bytes()
    h_adv, h_inst = sy.merkle_sum_witness_host(spec, host(leaves), host(sibs), host(idx), 1 << 40, k)
    assert (_pcie_bytes() - b0).tolist() == [3 * 64 + 6 * 64 + 24, 3 * sy.N_ADVICE * (32 << k) + 3 * 128]
    assert np.array_equal(h_adv, host(adv)) and np.array_equal(h_inst, host(inst))
