"""keygen on the GPU: the permutation assembly (``hm_permutation_assemble_dev``) cell for cell against ``synthesis.permutation_cells``, the
sigma columns word for word against ``synthesis.permutation_columns``, ``keygen_vk``'s commitments against [f(s)]G for a known s,
``keygen_pk``'s forms against the domain's transforms, and -- resting on no twin -- the permutation argument's grand products of a
GPU-built MerkleSumTree witness closing at 1 over the key's sigma columns.  Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
import keygen_cases as kc
from halo2_experiments_amd import _lib, circuits, evaluation as ev, keygen, poseidon as ps, synthesis as sy
from halo2_experiments_amd.arithmetic import _stream_ptr
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words
from halo2_experiments_amd.kzg import G1_GENERATOR, ParamsKZG

from conftest import g1_equal

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R
HM_ERR_BAD_ARG = -1
_u32p, _u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def cells_of(t):
    return t.cpu().numpy().tolist()


def dev_u32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32)).cuda()


def dev_pairs(pairs):
    return dev_u32(pairs).reshape(-1, 2)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the assembly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pairs", kc.small_sets(), ids=[n for n, _ in kc.small_sets()])
def test_cells_equal_the_twin_on_small_sets(name, pairs):
    got = keygen.permutation_cells_dev(pairs, 3, 4)
    assert got.dtype == torch.uint32 and got.is_cuda and got.shape == (48,)
    assert cells_of(got) == kc.twin_cells(pairs, 3, 4)


def test_cells_equal_the_twin_beyond_one_sort_tile_and_twice_the_same():
    """P = 12, n = 2^10, 5 000 random copies: 10 000 keys padded to 16 384 = 8 LDS tiles, so the global stages of the sort run; the
    cells are drawn from 3 000 so that classes of many sizes form"""
    P, k = 12, 10
    rng = random.Random(2024)
    pool = rng.sample(range(P << k), 3000)
    pairs = [(rng.choice(pool), rng.choice(pool)) for _ in range(5000)]
    first = keygen.permutation_cells_dev(pairs, P, k)
    second = keygen.permutation_cells_dev(pairs, P, k)
    exp = kc.twin_cells(pairs, P, k)
    assert cells_of(first) == exp
    assert same(first, second)
    assert sum(1 for c, s in enumerate(exp) if s != c) > 2000


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_one_class_of_4097_cells_given_as_a_chain(order):
    """every union but the first joins the one large class: the contended case of the compare-and-swap hooks"""
    P, k = 12, 10
    rng = random.Random(4097)
    members = sorted(rng.sample(range(P << k), 4097), reverse=True)
    pairs = list(zip(members, members[1:]))
    if order == "shuffled":
        rng.shuffle(pairs)
    got = cells_of(keygen.permutation_cells_dev(pairs, P, k))
    asc = members[::-1]
    exp = list(range(P << k))
    for c, nxt in zip(asc, asc[1:] + asc[:1]):
        exp[c] = nxt
    assert got == exp
    if order == "descending":
        assert got == kc.twin_cells(pairs, P, k)


def test_no_copies_give_the_identity():
    got, dropped = keygen.permutation_cells_dev([], 5, 6, return_dropped=True)
    assert cells_of(got) == list(range(5 << 6)) and cells_of(dropped) == [0]
    got = keygen.permutation_cells_dev(np.zeros((0, 2), dtype=np.uint32), 1, 0)
    assert cells_of(got) == [0]


def test_a_pair_out_of_range_is_dropped_and_counted_and_the_rest_is_unaffected():
    P, k = 3, 4
    cells = P << k
    valid = [(1, 2), (2, 40), (5, 5), (47, 0), (13, 12)]
    raw = valid[:2] + [(cells, 3)] + valid[2:4] + [(7, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)] + valid[4:]
    got, dropped = keygen.permutation_cells_dev(dev_pairs(raw), P, k, return_dropped=True)
    assert cells_of(dropped) == [3]
    assert cells_of(got) == kc.twin_cells(valid, P, k)
    assert cells_of(got)[3] == 3 and cells_of(got)[7] == 7          # the valid end of a dropped pair is not joined to anything
    got2, dropped2 = keygen.permutation_cells_dev(dev_pairs(valid), P, k, return_dropped=True)
    assert same(got, got2) and cells_of(dropped2) == [0]


# ---- 2. the columns -------------------------------------------------------------------------------------------------------------
def _layouts_for_columns():
    return kc.real_layouts() + [("merkle_sum_tree depth 20 k 10", circuits.merkle_sum_tree(), sy.MerkleSumTreeLayout(20, 10))]


@pytest.mark.parametrize("which", range(4), ids=["sum_tree_5_9", "v3_5_8", "poseidon_6", "sum_tree_20_10"])
def test_columns_equal_the_twin_word_for_word(which):
    name, cs, lay = _layouts_for_columns()[which]
    dom = keygen.EvaluationDomain(cs.degree(), lay.k)
    got = keygen.permutation_columns_dev(cs, lay, dom.omega, keygen.FR_DELTA)
    exp = sy.permutation_columns(cs, lay, dom.omega, keygen.FR_DELTA)
    assert got.shape == exp.shape == (len(cs.equality), lay.n, 4) and got.dtype == exp.dtype
    assert torch.equal(got, exp), name
    cells = keygen.permutation_cells_dev(keygen.copy_pairs(cs, lay), len(cs.equality), lay.k)
    assert cells_of(cells) == [j * lay.n + i for col in sy.permutation_cells(cs, lay) for (j, i) in col], name


def test_columns_of_a_cell_id_out_of_range_are_zero():
    cells = dev_u32([5, 0, 48, 0xFFFFFFFF] + list(range(4, 48)))
    omega, delta = keygen.EvaluationDomain(3, 4).omega, keygen.FR_DELTA
    out = keygen.permutation_columns_from_cells(cells, 3, 4, omega, delta)
    assert ints(out.reshape(48, 4)[:5]) == [pow(omega, 5, R), 1, 0, 0, pow(omega, 4, R)]
    assert ints(out[2, 15:16]) == [pow(delta, 2, R) * pow(omega, 15, R) % R]


# ---- 3 - 5. the keys of MerkleSumTree depth 5 at k = 9 --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def key9():
    spec = ps.default_spec(5)
    lay = sy.MerkleSumTreeLayout(5, 9, spec)
    cs = circuits.merkle_sum_tree(spec)
    params = ParamsKZG.setup(9, SRS_S)
    try:
        vk = keygen.keygen_vk(params, cs, lay)
        pk = keygen.keygen_pk(params, vk, cs, lay)
        dom = vk.domain
        twin_fixed = d([v for col in lay.fixed_columns() for v in col]).reshape(sy.N_FIXED, lay.n, 4)
        twin_sigma = sy.permutation_columns(cs, lay, dom.omega, keygen.FR_DELTA)
        torch.cuda.synchronize()
        yield dict(spec=spec, lay=lay, cs=cs, vk=vk, pk=pk, dom=dom, twin_fixed=twin_fixed, twin_sigma=twin_sigma)
    finally:
        params.release()


def test_keygen_vk_commits_to_the_fixed_and_sigma_columns(key9):
    """every commitment equals [f(s)]G, f(s) by Horner on the coefficients of the TWIN's columns (no kernel shared with the MSM)"""
    vk, dom = key9["vk"], key9["dom"]
    assert vk.cs is key9["cs"] and (dom.k, dom.extended_k) == (9, 12)
    assert vk.fixed_commitments.shape == (sy.N_FIXED, 12) and vk.permutation_commitments.shape == (12, 12)
    for com, values in ((vk.fixed_commitments, key9["twin_fixed"]), (vk.permutation_commitments, key9["twin_sigma"])):
        coeffs = dom.lagrange_to_coeff(values.clone())
        fs = h.eval_polynomial(coeffs, np.stack([fr_words(SRS_S)] * coeffs.shape[0]))
        expected = h.g1_fixed_base_mul(torch.from_numpy(fs.view(np.int64)).cuda(), G1_GENERATOR).cpu().numpy().view(np.uint64)
        for c in range(coeffs.shape[0]):
            assert g1_equal(com[c], expected[c]), c
    assert len({bytes(c) for c in vk.permutation_commitments}) == 12


def test_keygen_pk_holds_the_three_forms_of_every_column(key9):
    pk, dom, lay, cs = key9["pk"], key9["dom"], key9["lay"], key9["cs"]
    n, usable = lay.n, lay.n - cs.blinding_factors - 1
    assert pk.vk is key9["vk"]
    assert torch.equal(pk.fixed_values, key9["twin_fixed"]) and torch.equal(pk.permutation_values, key9["twin_sigma"])
    omega = fr_words(dom.omega)
    for values, polys, cosets in ((pk.fixed_values, pk.fixed_polys, pk.fixed_cosets),
                                  (pk.permutation_values, pk.permutation_polys, pk.permutation_cosets)):
        assert polys.shape == values.shape and cosets.shape == (values.shape[0], dom.extended_len(), 4)
        assert torch.equal(polys, dom.lagrange_to_coeff(values.clone()))
        back = polys.clone()
        for j in range(back.shape[0]):
            h.best_fft(back[j], omega, dom.k)                    # the forward transform of the coefficients gives the values back
        assert torch.equal(back, values)
        assert torch.equal(cosets, dom.coeff_to_extended(polys))
    assert torch.equal(pk.l0, d([1] + [0] * (n - 1)))
    assert torch.equal(pk.l_last, d([1 if i == usable else 0 for i in range(n)]))
    assert torch.equal(pk.l_active, d([1 if i < usable else 0 for i in range(n)]))


def test_keygen_pk_without_cosets_and_with_other_parameters(key9):
    params = ParamsKZG.setup(8, SRS_S)
    try:
        with pytest.raises(ValueError):
            keygen.keygen_vk(params, key9["cs"], key9["lay"])
    finally:
        params.release()
    params = ParamsKZG.setup(9, SRS_S)
    try:
        pk = keygen.keygen_pk(params, key9["vk"], key9["cs"], key9["lay"], cosets=False)
    finally:
        params.release()
    assert pk.fixed_cosets is None and pk.permutation_cosets is None
    assert torch.equal(pk.permutation_polys, key9["pk"].permutation_polys) and torch.equal(pk.fixed_polys, key9["pk"].fixed_polys)


def run(exprs, columns, n, **scalars):
    g = ev.GraphEvaluator()
    g.add_custom_gates(exprs)
    prog = g.compile(0, len(columns), 0)
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    prog.evaluate(list(columns), out, **scalars)
    prog.destroy()
    return out


@pytest.mark.parametrize("tamper", [None, "copied"])
def test_the_grand_products_of_a_real_witness_close_over_the_keys_sigma_columns(key9, tamper):
    """prod over the usable rows of (v + beta delta^j omega^i + gamma) / (v + beta sigma_j(omega^i) + gamma), chained over the three
    sets of 4 columns, is 1 exactly when the copies hold on the witness (up to a chance of about rows / r): the key's sigma columns
    are judged by what they are for, not by the twin.  One copied cell changed: the product does not close."""
    spec, lay, cs, pk, dom = key9["spec"], key9["lay"], key9["cs"], key9["pk"], key9["dom"]
    depth, k, n = 5, 9, lay.n
    usable = n - cs.blinding_factors - 1
    rng = random.Random(59)
    beta, gamma = rng.randrange(2, R), rng.randrange(2, R)
    leaf = (rng.randrange(R), rng.randrange(1 << 40))
    sib = [(rng.randrange(R), rng.randrange(1 << 40)) for _ in range(depth)]
    idx = torch.tensor([rng.randrange(1 << depth)], dtype=torch.int64, device="cuda")
    adv_all, inst4 = sy.merkle_sum_witness(spec, d(list(leaf)).reshape(1, 2, 4), d([v for p in sib for v in p]).reshape(1, depth, 2, 4), idx,
                                           1 << 50, k)
    adv = adv_all[0]
    if tamper:
        c, r = sy.STATE[4], lay.pad_row(0)
        adv[c, r] = d([(ints(adv[c, r:r + 1])[0] + 1) % R])[0]
    inst = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    inst[:4] = inst4[0]
    by_kind = {"advice": adv, "fixed": pk.fixed_values}
    perm_cols = [inst if kind == "instance" else by_kind[kind][c] for kind, c in cs.equality]
    P, chunk, delta = len(cs.equality), cs.permutation_chunk_len(), keygen.FR_DELTA
    assert (P, chunk, cs.permutation_sets()) == (12, 4, 3)
    x_col = d([pow(dom.omega, i, R) for i in range(n)])
    start = 1
    for s0 in range(0, P, chunk):
        cc, ss = perm_cols[s0:s0 + chunk], [pk.permutation_values[j] for j in range(s0, s0 + chunk)]
        den_e = num_e = None
        for j in range(chunk):
            de = ev.Advice(j) + ev.BETA * ev.Advice(chunk + j) + ev.GAMMA
            ne = ev.Advice(j) + ev.BETA * ev.Advice(2 * chunk) * pow(delta, s0 + j, R) + ev.GAMMA
            den_e = de if den_e is None else den_e * de
            num_e = ne if num_e is None else num_e * ne
        den = run([den_e], cc + ss + [x_col], n, beta=beta, gamma=gamma)
        num = run([num_e], cc + ss + [x_col], n, beta=beta, gamma=gamma)
        h.batch_invert(den)
        z = h.grand_product(run([ev.Advice(0) * ev.Advice(1)], [num, den], n), fr_words(start))
        start = ints(z[usable:usable + 1])[0]
    assert (start == 1) == (tamper is None)


# ---- 6. bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message_and_nothing_is_launched():
    lib = _lib.load()
    pairs = dev_pairs([(1, 2), (3, 4), (5, 6), (7, 8)])
    cells = dev_u32([0xABCD] * 49)
    dropped = dev_u32([0xABCD] * 2)
    out = torch.full((48, 4), -1, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(_stream_ptr(out))
    u32 = lambda t, off=0: ctypes.cast(ctypes.c_void_p(t.data_ptr() + off), _u32p)
    w = fr_words(5).ctypes.data_as(_u64p)
    ok = dict(copies=u32(pairs), m=4, columns=3, k=4, cells=u32(cells), dropped=u32(dropped))

    def assemble(**kw):
        a = dict(ok, **kw)
        return lib.hm_permutation_assemble_dev(a["copies"], a["m"], a["columns"], a["k"], a["cells"], a["dropped"], stream)
    for kw, word in ((dict(copies=None), b"null"), (dict(cells=None), b"null"), (dict(columns=0), b"columns"), (dict(k=31), b"2^32"),
                     (dict(m=(1 << 30) + 1), b"2^31"), (dict(copies=u32(pairs, 4)), b"aligned"), (dict(cells=u32(cells, 2)), b"aligned"),
                     (dict(dropped=u32(dropped, 2)), b"aligned"), (dict(copies=u32(cells, 8)), b"overlaps")):
        assert assemble(**kw) == HM_ERR_BAD_ARG and word in lib.hm_last_error(), kw
    okc = dict(cells=u32(cells), columns=3, k=4, omega=w, delta=w, out=ctypes.c_void_p(out.data_ptr()))

    def columns(**kw):
        a = dict(okc, **kw)
        return lib.hm_permutation_columns_bn256_fr_dev(a["cells"], a["columns"], a["k"], a["omega"], a["delta"], a["out"], stream)
    for kw, word in ((dict(cells=None), b"null"), (dict(omega=None), b"null"), (dict(delta=None), b"null"), (dict(out=None), b"null"),
                     (dict(columns=0), b"columns"), (dict(columns=1 << 20, k=13), b"2^32"),
                     (dict(out=ctypes.c_void_p(out.data_ptr() + 8)), b"aligned"), (dict(cells=u32(cells, 1)), b"aligned"),
                     (dict(cells=u32(out, 16)), b"overlaps")):
        assert columns(**kw) == HM_ERR_BAD_ARG and word in lib.hm_last_error(), kw
    torch.cuda.synchronize()
    assert cells_of(cells) == [0xABCD] * 49 and cells_of(dropped) == [0xABCD] * 2 and bool((out == -1).all())
    with pytest.raises(ValueError):
        keygen.permutation_cells_dev(pairs.view(torch.int32), 3, 4)
