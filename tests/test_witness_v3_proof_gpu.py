"""One real proof's polynomial side from the GPU-built MerkleTreeV3 witness: tests/test_witness_proof_gpu.py step for step, with
circuits.merkle_v3(spec) in place of the sum tree's circuit.  Depth 20 at min_k = 10 and the reference's depth 5 at its k = 10
(/root/reference/src/circuits/merkle_v3.rs:91-114).

From the device columns (advice of synthesis.merkle_witness with random blinding rows, the layout's fixed columns, the instance
column, the sigma columns of synthesis.permutation_columns) the device makes the 2 grand products of the permutation argument over
the 8 equality columns (the constraint system's degree is 6: chunks of 4), every polynomial in coefficient form and on the extended
coset, and h = evaluate_h_program(cs, ...) / (X^n - 1); the circuit has no lookups.  Checked: h has degree below (d - 1) n = 5 n; the
quotient from min_cosets() = 5 of the 8 cosets (quotient_by_cosets) equals the whole-array h word for word; the verifier's identity
sum_i y^.. expression_i(x) == h(x) (x^n - 1) holds at a random x; every advice commitment equals [f(s)]G.  With one witness cell
changed (a Pow5 state word, a prove-layer word, a copied cell) all three polynomial checks fail."""
import random

import numpy as np
import pytest
import torch

import halo2_experiments_amd as h
from halo2_experiments_amd import circuits, evaluation as ev, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import EvaluationDomain, FR_MODULUS as R, FR_ZETA, fr_words
from halo2_experiments_amd.kzg import G1_GENERATOR, ParamsKZG
from oracle import graph_ref

from conftest import g1_equal

pytestmark = pytest.mark.gpu
SRS_S = 0x5EED5EED5EED5EED_0123456789ABCDEF_0F1E2D3C4B5A6978 % R


def d(values):
    return torch.from_numpy(ps.ints_to_words(values).view(np.int64)).cuda()


def ints(t):
    return ps.words_to_ints(t.cpu().numpy().view(np.uint64))


def run(exprs, columns, n, **scalars):
    g = ev.GraphEvaluator()
    g.add_custom_gates(exprs)
    prog = g.compile(0, len(columns), 0)
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    prog.evaluate(list(columns), out, **scalars)
    prog.destroy()
    return out


V3 = sy.MerkleTreeV3Layout


def path_of(depth, rng):
    if depth == 5:
        return 99, [1, 5, 6, 9, 9], [0, 0, 0, 0, 0]              # the reference's own case
    return rng.randrange(R), [rng.randrange(R) for _ in range(depth)], [rng.randrange(2) for _ in range(depth)]


@pytest.mark.parametrize("tamper", [None, "pow5 state", "prove layer", "copied"])
@pytest.mark.parametrize("depth,k", [(5, 10), (20, 10)])
def test_quotient_of_the_real_witness(depth, k, tamper):
    spec = ps.default_spec(3)
    assert k >= V3.min_k(depth, spec) and V3.min_k(20, spec) == 10
    lay = V3(depth, k, spec)
    cs = circuits.merkle_v3(spec)
    lay.check_constraint_system(cs)
    blinding = cs.blinding_factors
    n, usable = 1 << k, (1 << k) - blinding - 1
    deg = cs.degree()
    dom = EvaluationDomain(deg, k)
    ek, rot_scale = dom.extended_k, 1 << (dom.extended_k - k)
    assert (deg, dom.num_cosets(), dom.min_cosets()) == (6, 8, 5)
    omega, delta = dom.omega, pow(7, 1 << 28, R)
    rng = random.Random(1000 * depth + k)
    beta, gamma, theta, y, x = (rng.randrange(2, R) for _ in range(5))
    rnd = lambda cnt: [rng.randrange(R) for _ in range(cnt)]

    # ---- the witness: GPU columns, blinding rows random ----------------------------------------------------------------------
    leaf, sib, bits = path_of(depth, rng)
    leaves = d([leaf]).reshape(1, 4)
    sibs = d(sib).reshape(1, depth, 4)
    idx = torch.tensor([sum(b << l for l, b in enumerate(bits))], dtype=torch.int64, device="cuda")
    adv_all, inst2 = sy.merkle_witness(spec, leaves, sibs, idx, k)
    adv = adv_all[0]
    assert ints(inst2[0]) == [leaf, ps.MerkleTree.verify_path(leaf, (sib, bits), spec)]
    adv[:, usable:] = d(rnd(V3.N_ADVICE * (n - usable))).reshape(V3.N_ADVICE, n - usable, 4)
    cell = {None: None, "pow5 state": (V3.STATE[2], lay.perm_row(depth - 1) + 20), "prove layer": (V3.B, lay.prove_row(depth // 2) + 1),
            "copied": (V3.STATE[2], lay.pad_row(0))}[tamper]
    if cell:
        adv[cell[0], cell[1]] = d([(ints(adv[cell[0], cell[1]])[0] + 1) % R])[0]
    inst = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    inst[:2] = inst2[0]
    fixed = d([v for col in lay.fixed_columns() for v in col]).reshape(V3.N_FIXED, n, 4)
    sigma = sy.permutation_columns(cs, lay, omega, delta)
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    assert (P, chunk, nsets, L) == (8, 4, 2, 0)
    l0 = [1] + [0] * (n - 1)
    l_last = [1 if i == usable else 0 for i in range(n)]
    l_active = [1 if i < usable else 0 for i in range(n)]
    x_col = d([pow(omega, i, R) for i in range(n)])

    lookups = []                                    # the circuit has none

    # ---- the permutation argument over cs.equality, chunks of 4 ---------------------------------------------------------------
    by_kind = {"advice": adv, "fixed": fixed}
    perm_cols = [inst if kind == "instance" else by_kind[kind][c] for kind, c in cs.equality]
    zs, start = [], 1
    for s0 in range(0, P, chunk):
        cc, ss = perm_cols[s0:s0 + chunk], [sigma[j] for j in range(s0, min(s0 + chunk, P))]
        w = len(cc)
        den_e = num_e = None
        for j in range(w):
            de = ev.Advice(j) + ev.BETA * ev.Advice(w + j) + ev.GAMMA
            ne = ev.Advice(j) + ev.BETA * ev.Advice(2 * w) * pow(delta, s0 + j, R) + ev.GAMMA
            den_e = de if den_e is None else den_e * de
            num_e = ne if num_e is None else num_e * ne
        den = run([den_e], cc + ss + [x_col], n, beta=beta, gamma=gamma)
        num = run([num_e], cc + ss + [x_col], n, beta=beta, gamma=gamma)
        h.batch_invert(den)
        z = h.grand_product(run([ev.Advice(0) * ev.Advice(1)], [num, den], n), fr_words(start))
        start = ints(z[usable:usable + 1])[0]
        z[usable + 1:] = d(rnd(n - usable - 1))
        zs.append(z)
    if tamper in (None, "pow5 state"):
        assert start == 1                           # the copies of the layout hold on the GPU columns: the product closes

    # ---- the column table of evaluate_h_program: every polynomial in coefficient form, then on the extended coset --------------
    g, tab = circuits.evaluate_h_program(cs, k, ek, delta)
    assert (tab.sigma0, tab.z0, tab.l0, tab.x_coset, tab.lookup0, tab.t_inv) == (11, 19, 21, 24, 25, 25)
    lagrange = [fixed[i] for i in range(V3.N_FIXED)] + [sigma[j] for j in range(P)] + zs + [d(l0), d(l_last), d(l_active)]
    n_before_x = len(lagrange)                      # the x_coset entry (the polynomial X) comes here, already in coefficient form
    lagrange += lookups + [adv[c] for c in range(V3.N_ADVICE)] + [inst]
    coeffs = dom.lagrange_to_coeff(torch.stack(lagrange))
    x_poly = d([0, 1] + [0] * (n - 2)).reshape(1, n, 4)
    coeffs = torch.cat([coeffs[:n_before_x], x_poly, coeffs[n_before_x:]])       # fixed entries 0 .. 24, advice 25 .. 31, instance 32
    n_fixed_polys = tab.t_inv
    assert coeffs.shape[0] == n_fixed_polys + V3.N_ADVICE + 1
    ext = dom.coeff_to_extended(coeffs)
    t_inv = d([pow((pow(FR_ZETA * pow(dom.extended_omega, i, R) % R, n, R) - 1) % R, -1, R) for i in range(rot_scale)])
    prog = g.compile(tab.num_fixed_entries, cs.num_advice, cs.num_instance, rot_scale=rot_scale, short_columns=tab.short_columns)
    h_ext = torch.zeros((dom.extended_len(), 4), dtype=torch.int64, device="cuda")
    prog.evaluate([ext[i] for i in range(n_fixed_polys)] + [t_inv] + [ext[i] for i in range(n_fixed_polys, coeffs.shape[0])], h_ext,
                  beta=beta, gamma=gamma, theta=theta, y=y)
    prog.destroy()
    h_coeff = dom.extended_to_coeff(h_ext)                                        # ((d - 1) n, 4): h(X); in place on h_ext
    torch.cuda.synchronize()
    assert h_coeff.shape[0] == (deg - 1) * n
    degree_ok = not bool(h_ext[(deg - 1) * n:].any())                             # deg h < 5 n iff X^n - 1 divides the numerator

    # ---- the same quotient from 5 of the 8 cosets, in one call from the coefficient arrays -------------------------------------
    g2, tab2 = circuits.evaluate_h_program(cs, k, ek, delta, per_coset=True, divide=False)
    prog2 = g2.compile(tab2.num_fixed_entries, cs.num_advice, cs.num_instance, rot_scale=1)
    use = [7, 0, 2, 5, 3]
    coeff_cols = [coeffs[i] for i in range(n_fixed_polys)] + [coeffs[tab.x_coset]] + [coeffs[i] for i in range(n_fixed_polys, coeffs.shape[0])]
    h_min = prog2.quotient_by_cosets(dom, coeff_cols, cosets=use, beta=beta, gamma=gamma, theta=theta, y=y)   # (the t_inv entry is unread)
    prog2.destroy()
    cosets_ok = h_min.shape == h_coeff.shape and bool((h_min == h_coeff).all())

    # ---- the verifier's check at x -----------------------------------------------------------------------------------------------
    kind = {"advice": ev.Advice, "fixed": ev.Fixed, "instance": ev.Instance}
    F = ev.Fixed
    exprs = list(cs.polynomials())
    exprs += ev.permutation_expressions([kind[kd](i) for kd, i in cs.equality], [F(tab.sigma0 + j) for j in range(P)],
                                        [lambda rot, i=i: F(tab.z0 + i, rot) for i in range(nsets)], F(tab.l0), F(tab.l_last), F(tab.l_active),
                                        F(tab.x_coset), chunk, delta, -(blinding + 1))
    for j, (ins, tabs) in enumerate(cs.lookups):
        b = tab.lookup0 + 3 * j
        exprs += ev.lookup_expressions(ins, tabs, lambda rot, b=b: F(b, rot), lambda rot, b=b: F(b + 1, rot), lambda rot, b=b: F(b + 2, rot),
                                       F(tab.l0), F(tab.l_last), F(tab.l_active))
    rots, M, npoly = [0, 1, -1, -(blinding + 1)], 16, coeffs.shape[0]
    pts = np.stack([fr_words(x * pow(omega, r, R) % R) for r in rots for _ in range(npoly)])
    which = np.array([p for _ in rots for p in range(npoly)], dtype=np.uint32)
    vals = ps.words_to_ints(h.eval_polynomial(coeffs, pts, poly_index=which))
    at = [[None] * M for _ in range(npoly)]
    for ri, r in enumerate(rots):
        for p in range(npoly):
            at[p][r % M] = vals[ri * npoly + p]
    at[tab.x_coset] = [x] + [None] * (M - 1)
    fixed_at, advice_at, inst_at = at[:n_fixed_polys] + [None], at[n_fixed_polys:n_fixed_polys + V3.N_ADVICE], at[n_fixed_polys + V3.N_ADVICE:]
    acc = 0
    for e in exprs:
        acc = (acc * y + graph_ref.evaluate_expression(e, fixed_at, advice_at, inst_at, {"beta": beta, "gamma": gamma, "theta": theta}, 0, 1, M)) % R
    hx = ps.words_to_ints(h.eval_polynomial(h_coeff.reshape(1, (deg - 1) * n, 4).contiguous(), np.stack([fr_words(x)])))[0]
    identity_ok = acc == hx * (pow(x, n, R) - 1) % R

    print(f"depth {depth} k {k} tamper {tamper}: degree_ok {degree_ok} cosets_ok {cosets_ok} identity_ok {identity_ok}")
    if tamper:
        assert not (degree_ok or cosets_ok or identity_ok)             # one changed cell fails all of them
        return
    assert degree_ok and cosets_ok and identity_ok

    # ---- the advice commitments against [f(s)]G, f(s) by Horner on the coefficients (no kernel shared with the MSM) ---------------
    params = ParamsKZG.setup(k, SRS_S)
    try:
        adv_coeffs = coeffs[n_fixed_polys:n_fixed_polys + V3.N_ADVICE].contiguous()
        fs = h.eval_polynomial(adv_coeffs, np.stack([fr_words(SRS_S)] * V3.N_ADVICE))
        expected = h.g1_fixed_base_mul(torch.from_numpy(fs.view(np.int64)).cuda(), G1_GENERATOR).cpu().numpy().view(np.uint64)
        for c in range(V3.N_ADVICE):
            assert g1_equal(params.commit_lagrange(adv[c].contiguous()), expected[c]), c
            assert g1_equal(params.commit(adv_coeffs[c]), expected[c]), c
    finally:
        params.release()
