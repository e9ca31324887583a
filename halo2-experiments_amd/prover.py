"""``create_proof`` of ``halo2_proofs::plonk`` for one circuit over KZG with the SHPLONK multiopen, every polynomial step on the
device entry points that existed before it plus the set-quotient kernel of ``shplonk``.

The order of the transcript is RECALLED from upstream tag v2023_02_02 (plonk/prover.rs) and not pinned against its bytes: the vk digest;
the instance values as scalars (the KZG path does not commit them); the advice commitments; theta; per lookup the permuted input and
table; beta, gamma; the permutation z columns, then the lookup z columns; the vanishing argument's random polynomial; y; the h
pieces; x; the evaluations -- advice, fixed, random polynomial, permutation common, permutation z, lookups --; SHPLONK.  The order
of the advice / fixed queries is this project's own (``ConstraintSystem.queries``: first use in the gates, then the lookups, then the
equality columns), since upstream's depends on the order of ``meta.query_*`` calls inside chips that are not in this tree.  The vk
digest is Blake2b-512 (``person = b"Halo2-Verify-Key"``) over k, the column counts, the equality list and the commitments, reduced
mod r: upstream hashes the ``Debug`` print of its own struct, which cannot be reproduced here.

Nothing but the blinding is random, and it comes from ``random_fr(seed + ...)``: a seed fixes the bytes."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from . import circuits, evaluation as ev
from ._marshal import _is_tensor
from .arithmetic import (batch_invert, best_multiexp_batch, eval_polynomial, grand_product_batch, linear_combination,
                         permute_expression_pairs, random_fr)
from .domain import FR_MODULUS, FR_ZETA, fr_words
from .keygen import FR_DELTA, ProvingKey, VerifyingKey
from .poseidon import ints_to_words, words_to_ints
from .shplonk import create_opening, g1_words_to_int
from .transcript import Blake2bWrite

R = FR_MODULUS


def vk_digest(vk: VerifyingKey) -> int:
    """the scalar both sides absorb first (see the module docstring)"""
    cs = vk.cs
    hsh = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    hsh.update(struct.pack("<5I", vk.domain.k, cs.num_fixed, cs.num_advice, cs.num_instance, len(cs.equality)))
    for kind, index in cs.equality:
        hsh.update(kind.encode() + struct.pack("<I", index))
    for com in list(vk.fixed_commitments) + list(vk.permutation_commitments):
        p = g1_words_to_int(com)
        hsh.update(bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"))
    return int.from_bytes(hsh.digest(), "little") % R


def instance_values(cs, instance):
    """``instance`` -> one list of integers per instance column.  A single (len, 4) word tensor / array or a flat list of integers
    stands for the only column of a one-column system."""
    def column(c):
        if _is_tensor(c):
            return words_to_ints(c.cpu().numpy().view(np.uint64).reshape(-1, 4))
        if isinstance(c, np.ndarray):
            return words_to_ints(c.view(np.uint64).reshape(-1, 4))
        return [int(v) % R for v in c]
    single = _is_tensor(instance) or isinstance(instance, np.ndarray) or (len(instance) > 0 and isinstance(instance[0], int))
    cols = [column(instance)] if single else [column(c) for c in instance]
    if len(cols) != cs.num_instance:
        raise ValueError(f"instance: {cs.num_instance} column(s) expected")
    return cols


def _dev(values, device):
    import torch
    return torch.from_numpy(ints_to_words(values).view(np.int64)).to(device)


def _run(exprs, columns, n, counts, **scalars):
    """the value of one expression list (folded in y; a single expression is itself) on the n rows of the domain"""
    import torch
    g = ev.GraphEvaluator()
    g.add_custom_gates(exprs)
    prog = g.compile(*counts)
    out = torch.zeros((n, 4), dtype=torch.int64, device=columns[0].device)
    try:
        prog.evaluate(list(columns), out, **scalars)
    finally:
        prog.destroy()
    return out


def _compress(exprs):
    acc = ev.Constant(0)
    for e in exprs:
        acc = acc * ev.THETA + e
    return acc


def create_proof(params, pk: ProvingKey, advice, instance, seed: int, _trace: dict = None) -> bytes:
    """The proof bytes for the witness ``advice`` -- the (num_advice, n, 4) device tensor a witness writer returns for one circuit --
    and its ``instance`` values.  One circuit per proof: a list of several witnesses, or a 4-dimensional tensor holding more than
    one, raises ValueError.  ``_trace``: a dict that receives the committed polynomials and their commitments (tests)."""
    import torch

    if isinstance(advice, (list, tuple)):
        if len(advice) != 1:
            raise ValueError("create_proof: one circuit per proof (multi-circuit proofs are out of scope)")
        advice = advice[0]
    if _is_tensor(advice) and advice.dim() == 4:
        if advice.shape[0] != 1:
            raise ValueError("create_proof: one circuit per proof (multi-circuit proofs are out of scope)")
        advice = advice[0]
    vk = pk.vk
    cs, dom = vk.cs, vk.domain
    k, n = dom.k, 1 << dom.k
    if params.k != k:
        raise ValueError("create_proof: the parameters and the key differ in k")
    if not _is_tensor(advice) or not advice.is_cuda or tuple(advice.shape) != (cs.num_advice, n, 4):
        raise ValueError(f"create_proof: advice must be a ({cs.num_advice}, {n}, 4) GPU tensor")
    device = advice.device
    blinding, deg = cs.blinding_factors, cs.degree()
    usable = n - blinding - 1
    omega, delta = dom.omega, FR_DELTA
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    counts = (cs.num_fixed, cs.num_advice, cs.num_instance)
    base = (int(seed) & 0xFFFFFFFFFFFF) << 10      # the seeds of the blinding: advice, permuted columns, z columns, random polynomial
    d = lambda values: _dev(values, device)
    commits = {}

    def commit_lagrange(key_cols):
        com = best_multiexp_batch([c for _, c in key_cols], params.g_lagrange_handle)
        for (key, _), c in zip(key_cols, com):
            commits[key] = g1_words_to_int(c)
            transcript.write_point(commits[key])

    def commit_coeff(key_cols):
        com = best_multiexp_batch([c for _, c in key_cols], params.g_handle)
        for (key, _), c in zip(key_cols, com):
            commits[key] = g1_words_to_int(c)
            transcript.write_point(commits[key])

    # ---- the columns -----------------------------------------------------------------------------------------------------------------------
    adv = advice.clone()
    adv[:, usable:] = random_fr(cs.num_advice * (n - usable), base, device, shape=(cs.num_advice, n - usable, 4))
    inst_cols = instance_values(cs, instance)
    inst = torch.zeros((cs.num_instance, n, 4), dtype=torch.int64, device=device)
    for c, values in enumerate(inst_cols):
        if len(values) > usable:
            raise ValueError("create_proof: too many instance values")
        if values:
            inst[c, :len(values)] = d(values)
    fixed = pk.fixed_values
    table = [fixed[i] for i in range(cs.num_fixed)] + [adv[i] for i in range(cs.num_advice)] + [inst[i] for i in range(cs.num_instance)]

    transcript = Blake2bWrite()
    transcript.common_scalar(vk_digest(vk))
    for values in inst_cols:
        for v in values:
            transcript.common_scalar(v)
    commit_lagrange([(("advice", c), adv[c]) for c in range(cs.num_advice)])
    theta = transcript.squeeze_challenge()

    # ---- the lookups: permuted columns -------------------------------------------------------------------------------------------------------
    lk_in = [_run([_compress(ins)], table, n, counts, theta=theta) for ins, _ in cs.lookups]
    lk_tab = [_run([_compress(tabs)], table, n, counts, theta=theta) for _, tabs in cs.lookups]
    permuted = permute_expression_pairs(lk_in, lk_tab, usable, blinding_seed=base + 0x40) if L else []
    commit_lagrange([pair for j, (a, s) in enumerate(permuted) for pair in ((("lookup_a", j), a), (("lookup_s", j), s))])
    beta = transcript.squeeze_challenge()
    gamma = transcript.squeeze_challenge()

    # ---- the permutation argument: one z per chunk of columns, chained at the last usable row ----------------------------------------------
    by_kind = {"advice": adv, "fixed": fixed, "instance": inst}
    perm_cols = [by_kind[kind][c] for kind, c in cs.equality]
    sigma = pk.permutation_values
    acc, xs = 1, []
    for _ in range(n):
        xs.append(acc)
        acc = acc * omega % R
    x_col = d(xs)
    mul2 = [ev.Advice(0) * ev.Advice(1)]
    factors = []
    for s0 in range(0, P, chunk):
        cc, ss = perm_cols[s0:s0 + chunk], [sigma[j] for j in range(s0, min(s0 + chunk, P))]
        w = len(cc)
        den_e = num_e = None
        for j in range(w):
            de = ev.Advice(j) + ev.BETA * ev.Advice(w + j) + ev.GAMMA
            ne = ev.Advice(j) + ev.BETA * ev.Advice(2 * w) * pow(delta, s0 + j, R) + ev.GAMMA
            den_e = de if den_e is None else den_e * de
            num_e = ne if num_e is None else num_e * ne
        cols = cc + ss + [x_col]
        den = _run([den_e], cols, n, (0, len(cols), 0), beta=beta, gamma=gamma)
        num = _run([num_e], cols, n, (0, len(cols), 0), beta=beta, gamma=gamma)
        batch_invert(den)
        factors.append(_run(mul2, [num, den], n, (0, 2, 0)))
    zs = grand_product_batch(factors, fr_words(1), chain_row=usable) if factors else []
    for i, z in enumerate(zs):
        z[usable + 1:] = random_fr(n - usable - 1, base + 0x80 + i, device)
    commit_lagrange([(("perm_z", i), z) for i, z in enumerate(zs)])

    # ---- the lookup arguments' z ----------------------------------------------------------------------------------------------------------------
    pair = [(ev.Advice(0) + ev.BETA) * (ev.Advice(1) + ev.GAMMA)]
    lk_factors = []
    for j, (a_perm, s_perm) in enumerate(permuted):
        num = _run(pair, [lk_in[j], lk_tab[j]], n, (0, 2, 0), beta=beta, gamma=gamma)
        den = _run(pair, [a_perm, s_perm], n, (0, 2, 0), beta=beta, gamma=gamma)
        batch_invert(den)
        lk_factors.append(_run(mul2, [num, den], n, (0, 2, 0)))
    lk_z = grand_product_batch(lk_factors, fr_words(1)) if lk_factors else []
    for j, z in enumerate(lk_z):
        z[usable + 1:] = random_fr(n - usable - 1, base + 0xC0 + j, device)
    commit_lagrange([(("lookup_z", j), z) for j, z in enumerate(lk_z)])

    # ---- the vanishing argument's random polynomial, then h -------------------------------------------------------------------------------------
    random_poly = random_fr(n, base + 0x100, device)
    commit_coeff([(("random",), random_poly)])
    y = transcript.squeeze_challenge()

    g, tab = circuits.evaluate_h_program(cs, k, dom.extended_k, delta)
    lookups3 = [c for j in range(L) for c in (lk_z[j], permuted[j][0], permuted[j][1])]
    lagrange = zs + lookups3 + [adv[c] for c in range(cs.num_advice)] + [inst[c] for c in range(cs.num_instance)]
    var_coeffs = dom.lagrange_to_coeff(torch.stack(lagrange))
    z_polys, lk_polys = var_coeffs[:nsets], var_coeffs[nsets:nsets + 3 * L]
    adv_polys, inst_polys = var_coeffs[nsets + 3 * L:nsets + 3 * L + cs.num_advice], var_coeffs[nsets + 3 * L + cs.num_advice:]
    sel = dom.lagrange_to_coeff(torch.stack([pk.l0, pk.l_last, pk.l_active]))
    x_poly = d([0, 1] + [0] * (n - 2)).reshape(1, n, 4)
    coeffs = torch.cat([pk.fixed_polys, pk.permutation_polys, z_polys, sel, x_poly, lk_polys, adv_polys, inst_polys])
    n_fixed_entries = tab.t_inv
    assert coeffs.shape[0] == n_fixed_entries + cs.num_advice + cs.num_instance
    ext = dom.coeff_to_extended(coeffs)
    rot_scale = 1 << (dom.extended_k - k)
    t_inv = d([pow((pow(FR_ZETA * pow(dom.extended_omega, i, R) % R, n, R) - 1) % R, -1, R) for i in range(rot_scale)])
    prog = g.compile(tab.num_fixed_entries, cs.num_advice, cs.num_instance, rot_scale=rot_scale, short_columns=tab.short_columns)
    h_ext = torch.zeros((dom.extended_len(), 4), dtype=torch.int64, device=device)
    try:
        prog.evaluate([ext[i] for i in range(n_fixed_entries)] + [t_inv] + [ext[i] for i in range(n_fixed_entries, coeffs.shape[0])], h_ext,
                      beta=beta, gamma=gamma, theta=theta, y=y)
    finally:
        prog.destroy()
    del ext
    h_coeff = dom.extended_to_coeff(h_ext)                      # ((deg - 1) n, 4): in place on h_ext
    pieces = [h_coeff[i * n:(i + 1) * n] for i in range(deg - 1)]
    commit_coeff([(("h_piece", i), p) for i, p in enumerate(pieces)])
    x = transcript.squeeze_challenge()

    # ---- the evaluations ----------------------------------------------------------------------------------------------------------------------
    adv_q, fix_q, _ = cs.queries()
    last = -(blinding + 1)
    rot = lambda r: x * pow(omega, r, R) % R
    polys = {("random",): random_poly}
    for c in range(cs.num_advice):
        polys[("advice", c)] = adv_polys[c]
    for c in range(cs.num_fixed):
        polys[("fixed", c)] = pk.fixed_polys[c]
    for j in range(P):
        polys[("sigma", j)] = pk.permutation_polys[j]
    for i in range(nsets):
        polys[("perm_z", i)] = z_polys[i]
    for j in range(L):
        polys[("lookup_z", j)], polys[("lookup_a", j)], polys[("lookup_s", j)] = lk_polys[3 * j], lk_polys[3 * j + 1], lk_polys[3 * j + 2]
    polys[("h",)] = linear_combination(pieces, np.stack([fr_words(pow(x, n * i, R)) for i in range(deg - 1)]))
    wanted = [(("advice", c), rot(r)) for c, r in adv_q] + [(("fixed", c), rot(r)) for c, r in fix_q] + [(("random",), x)]
    wanted += [(("sigma", j), x) for j in range(P)]
    for i in range(nsets):
        wanted += [(("perm_z", i), x), (("perm_z", i), rot(1))] + ([(("perm_z", i), rot(last))] if i + 1 < nsets else [])
    for j in range(L):
        wanted += [(("lookup_z", j), x), (("lookup_z", j), rot(1)), (("lookup_a", j), x), (("lookup_a", j), rot(-1)), (("lookup_s", j), x)]
    keys = list(polys)
    stack = torch.stack([polys[key] for key in keys])
    index = {key: i for i, key in enumerate(keys)}
    vals = words_to_ints(eval_polynomial(stack, np.stack([fr_words(pt) for _, pt in wanted]),
                                         poly_index=np.array([index[key] for key, _ in wanted], dtype=np.uint32)))
    evals = {}
    for (key, pt), v in zip(wanted, vals):
        evals[(key, pt)] = v
        transcript.write_scalar(v)
    hx = words_to_ints(eval_polynomial(polys[("h",)].reshape(1, n, 4), np.stack([fr_words(x)])))[0]

    # ---- the multiopen: upstream's order of queries ---------------------------------------------------------------------------------------------
    q = lambda key, pt: (key, pt, evals[(key, pt)])
    queries = [q(("advice", c), rot(r)) for c, r in adv_q]
    queries += [qq for i in range(nsets) for qq in (q(("perm_z", i), x), q(("perm_z", i), rot(1)))]
    queries += [q(("perm_z", i), rot(last)) for i in reversed(range(nsets - 1))]
    for j in range(L):
        queries += [q(("lookup_z", j), x), q(("lookup_a", j), x), q(("lookup_s", j), x), q(("lookup_a", j), rot(-1)), q(("lookup_z", j), rot(1))]
    queries += [q(("fixed", c), rot(r)) for c, r in fix_q] + [q(("sigma", j), x) for j in range(P)]
    queries += [(("h",), x, hx), q(("random",), x)]
    create_opening(params, transcript, queries, polys)
    if _trace is not None:
        _trace.update(polys=polys, commits=commits, lagrange={"advice": adv, "perm_z": zs, "lookup_z": lk_z, "permuted": permuted},
                      pieces=pieces, challenges=dict(theta=theta, beta=beta, gamma=gamma, y=y, x=x))
    return transcript.finalize()
