"""``create_proof`` of ``halo2_proofs::plonk`` over KZG with the SHPLONK multiopen, for one circuit (``create_proof``) or for m circuits of
one constraint system in a single transcript (``create_proof_multi``, upstream's ``&[circuit; m]``): ONE body of protocol code,
``_create_proof``, with every polynomial step on the device entry points (DESIGN.md sections 17 and 19).

The order of the transcript is RECALLED from upstream tag v2023_02_02 (plonk/prover.rs) and not pinned against its bytes.  All circuits
share theta, beta, gamma, y and x:

    1. the vk digest;  2. per circuit, its instance values as scalars (the KZG path does not commit them);  3. per circuit, its advice
    commitments;  4. theta;  5. per circuit, per lookup: the permuted input, then the permuted table;  6. beta, gamma;  7. per circuit,
    the permutation z columns;  8. per circuit, the lookup z columns;  9. ONE random polynomial of the vanishing argument;  10. y;
    11. the h pieces;  12. x;  13. the evaluations -- per circuit the advice; fixed; random polynomial; sigma; per circuit the
    permutation z; per circuit the lookups;  14. SHPLONK over the queries -- per circuit: advice, permutation z, lookups; once: fixed,
    sigma, h, random polynomial.

h folds in y through circuit 0's gates, permutation and lookup terms, then circuit 1's, and so on; the division by X^n - 1 happens
once.  The order of the advice / fixed queries is this project's own (``ConstraintSystem.queries``: first use in the gates, then the
lookups, then the equality columns), since upstream's depends on the order of ``meta.query_*`` calls inside chips that are not in this
tree.  The vk digest is Blake2b-512 (``person = b"Halo2-Verify-Key"``) over k, the column counts, the equality list and the
commitments, reduced mod r: upstream hashes the ``Debug`` print of its own struct, which cannot be reproduced here.

Per phase ONE batched call carries all circuits: ``best_multiexp_batch`` over m x columns, one stacked ``lagrange_to_coeff`` /
``coeff_to_extended``, one ``permute_expression_pairs``, one ``batch_invert`` per argument, one ``eval_polynomial``, the set quotients with
more polynomials per set; the helper graph programs are compiled once per proof and run with the circuits as segments; h comes from
``CompiledGraph.evaluate_circuits`` with the shared columns at stride 0, in chunks of circuits chained through PreviousValue when the
circuits' own extended columns pass ``H_COLUMN_BUDGET`` (2 GiB, the witness writers' convention).  The permutation products are one
``grand_product_batch`` per circuit: its chain runs from one column set to the next and must start at 1 in every circuit.

Nothing but the blinding is random, and it comes from ``random_fr(seed + ...)``: a seed fixes the bytes.  The advice columns named in
``cs.unblinded_advice`` keep zeros in their last rows (the draw for the other columns is what it is without them), so their commitments
are ``commit_lagrange`` of the witness columns themselves: what ``solvency`` opens.  ``base`` = the low 48 bits of
``seed`` shifted by 10 (58 bits; ``create_proof``'s derivation, kept so that its bytes stay) names the streams of circuit 0: + 0 advice,
+ 0x40 + 2 j / + 1 the permuted columns of lookup j, + 0x80 + i the permutation z, + 0xC0 + j the lookup z, + 0x100 the random
polynomial (drawn once per proof).  Circuit c uses ``base | c << 58``: the 6 bits above the base, hence at most 64 circuits; no two
circuits of a proof and no two seeds (mod 2^48) share a stream.

``create_proofs`` makes m INDEPENDENT proofs of one key -- one per user of a solvency tree -- in one batched pass: proof b is byte for
byte ``create_proof(params, pk, advice[b], instances[b], seeds[b])``, with its own transcript, challenges, random polynomial and h.  Its
body, ``_create_proofs``, follows the protocol order stated above step by step with m = 1 per transcript; what it adds is that every
device step carries all proofs (``_Programs.run_proofs`` and h through ``CompiledGraph.evaluate_proofs``, the per-proof constants in a
device table; ``linear_combination_batch``; ``create_openings``).

``multiopen="gwc"`` on the three entries ends the proof in the GWC multiopen instead (step 14: ``gwc.create_opening`` /
``gwc.create_openings``, one witness point per distinct query point); everything before step 14 is the same code and the same bytes."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from . import circuits, evaluation as ev
from ._marshal import _is_tensor
from . import _lib
from .arithmetic import (batch_invert, best_multiexp_batch, eval_polynomial, grand_product_batch, linear_combination,
                         linear_combination_batch, permute_expression_pairs, random_fr)
from .domain import FR_MODULUS, FR_ZETA, fr_words
from .keygen import FR_DELTA, ProvingKey, VerifyingKey
from .poseidon import ints_to_words, words_to_ints
from . import gwc
from .shplonk import create_opening, create_openings, g1_words_to_int
from .transcript import WRITERS, check_encoding, check_multiopen

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


class _Programs:
    """the helper graph programs of one proof -- compressed lookups, permutation numerators and denominators, products -- compiled once
    each, whatever the number of circuits, and destroyed together"""

    def __init__(self):
        self._progs, self._shared = {}, {}

    def run(self, name, exprs, counts, columns, m, n, **scalars):
        """the value of one expression (an expression list folded in y) on the n rows of each of the m circuits in ONE launch: a column
        is (m, n, 4) -- one per circuit -- or (n, 4), shared; the circuits are the segments of ``CompiledGraph.evaluate``, so a
        rotation wraps inside its circuit.  -> (m, n, 4)"""
        import torch
        if name not in self._progs:
            g = ev.GraphEvaluator()
            g.add_custom_gates(exprs)
            self._progs[name] = g.compile(*counts)
        def rows(c):
            if c.dim() == 3:
                return c.reshape(m * n, 4)
            if m == 1:
                return c
            key = (c.data_ptr(), m)                      # a shared column, once per circuit: copied once per proof
            if key not in self._shared:
                self._shared[key] = (c, c.expand(m, n, 4).reshape(m * n, 4))
            return self._shared[key][1]
        cols = [rows(c) for c in columns]
        out = torch.zeros((m * n, 4), dtype=torch.int64, device=cols[0].device)
        self._progs[name].evaluate(cols, out, segments=m, **scalars)
        return out.reshape(m, n, 4)

    def run_proofs(self, name, exprs, counts, columns, n, constants):
        """``run`` for independent proofs, proof b with its own ``constants[b]`` (a dict of theta / beta / gamma): a column is
        (proofs, n, 4) or (n, 4), shared -- at stride 0, not copied.  ONE launch (``CompiledGraph.evaluate_proofs``).  -> (proofs, n, 4)"""
        import torch
        if name not in self._progs:
            g = ev.GraphEvaluator()
            g.add_custom_gates(exprs)
            self._progs[name] = g.compile(*counts)
        ref = next(c for c in columns)
        out = torch.zeros((len(constants), n, 4), dtype=torch.int64, device=ref.device)
        self._progs[name].evaluate_proofs(list(columns), out, constants)
        return out

    def destroy(self):
        for prog in self._progs.values():
            prog.destroy()
        self._progs, self._shared = {}, {}


def _compress(exprs):
    acc = ev.Constant(0)
    for e in exprs:
        acc = acc * ev.THETA + e
    return acc


MAX_CIRCUITS = 64                   # the circuit's number sits in the 6 seed bits above the 58 of ``base``
H_COLUMN_BUDGET = 2 << 30           # bytes of per-circuit extended columns in flight in the h step (the witness writers' 2 GiB)


def create_proof(params, pk: ProvingKey, advice, instance, seed: int, _trace: dict = None, encoding: str = "halo2",
                 multiopen: str = "shplonk") -> bytes:
    """The proof bytes for the witness ``advice`` -- the (num_advice, n, 4) device tensor a witness writer returns for one circuit --
    and its ``instance`` values.  One circuit per proof: a list of several witnesses, or a 4-dimensional tensor holding more than
    one, raises ValueError (``create_proof_multi`` takes several).  ``_trace``: a dict that receives the committed polynomials and
    their commitments (tests).  ``encoding``: "halo2" -- Blake2b transcript, compressed points, little-endian scalars -- or "evm" --
    Keccak transcript, uncompressed big-endian points and scalars (``transcript`` states both); the protocol is the same.
    ``multiopen``: "shplonk", or "gwc" -- the proof then ends in one witness point per distinct query point (``gwc``) where SHPLONK
    writes two points; everything before the multiopen is byte for byte the same."""
    check_encoding(encoding, "create_proof")
    check_multiopen(multiopen, "create_proof")
    if isinstance(advice, (list, tuple)):
        if len(advice) != 1:
            raise ValueError("create_proof: one circuit per proof (create_proof_multi proves several)")
        advice = advice[0]
    if _is_tensor(advice) and advice.dim() == 4:
        if advice.shape[0] != 1:
            raise ValueError("create_proof: one circuit per proof (create_proof_multi proves several)")
        advice = advice[0]
    trace = None if _trace is None else {}
    proof = _create_proof("create_proof", params, pk, [advice], [instance], seed, trace, encoding, multiopen)
    if _trace is not None:                                 # one circuit: its keys without the circuit's number
        strip = lambda key: key[:2] if len(key) == 3 else key
        lag = trace["lagrange"]
        _trace.update(polys={strip(key): p for key, p in trace["polys"].items()}, commits={strip(key): p for key, p in trace["commits"].items()},
                      lagrange={"advice": lag["advice"][0], "perm_z": lag["perm_z"][0], "lookup_z": lag["lookup_z"][0], "permuted": lag["permuted"][0]},
                      pieces=trace["pieces"], challenges=trace["challenges"])
    return proof


def create_proof_multi(params, pk: ProvingKey, advice, instances, seed: int, _trace: dict = None, multiopen: str = "shplonk") -> bytes:
    """ONE proof for m circuits of ``pk``'s constraint system (upstream ``create_proof(params, pk, &[circuit; m], &[instances; m])``):
    ``advice`` is the (m, num_advice, n, 4) GPU tensor a witness writer returns, or a list of m (num_advice, n, 4) tensors;
    ``instances`` holds m entries, each in the form ``create_proof`` takes.  1 <= m <= 64.  All circuits share theta, beta, gamma, y
    and x; with m = 1 the bytes are ``create_proof``'s.  ``_trace``: as in ``create_proof``, the keys of what belongs to one circuit
    carrying its number as a third element (("advice", column, circuit) ...) and ``lagrange`` holding one entry per circuit.
    ``multiopen``: as in ``create_proof``."""
    check_multiopen(multiopen, "create_proof_multi")
    if _is_tensor(advice):
        if advice.dim() != 4:
            raise ValueError("create_proof_multi: advice must be a (m, num_advice, n, 4) GPU tensor or a list of m (num_advice, n, 4) tensors")
        advice = [advice[c] for c in range(advice.shape[0])]
    elif not isinstance(advice, (list, tuple)):
        raise ValueError("create_proof_multi: advice must be a (m, num_advice, n, 4) GPU tensor or a list of m (num_advice, n, 4) tensors")
    advice = list(advice)
    if not 1 <= len(advice) <= MAX_CIRCUITS:
        raise ValueError(f"create_proof_multi: between 1 and {MAX_CIRCUITS} circuits per proof")
    if _is_tensor(instances) or isinstance(instances, np.ndarray) or len(instances) != len(advice):
        raise ValueError(f"create_proof_multi: {len(advice)} circuit(s) need {len(advice)} instance entries")
    return _create_proof("create_proof_multi", params, pk, advice, list(instances), seed, _trace, multiopen=multiopen)


def _create_proof(who, params, pk, advice, instances, seed, _trace, encoding: str = "halo2", multiopen: str = "shplonk") -> bytes:
    import torch

    m = len(advice)
    vk = pk.vk
    cs, dom = vk.cs, vk.domain
    k, n = dom.k, 1 << dom.k
    if params.k != k:
        raise ValueError(f"{who}: the parameters and the key differ in k")
    for a in advice:
        if not _is_tensor(a) or not a.is_cuda or tuple(a.shape) != (cs.num_advice, n, 4):
            raise ValueError(f"{who}: advice must be a ({cs.num_advice}, {n}, 4) GPU tensor" + (" per circuit" if m > 1 else ""))
    device = advice[0].device
    A, I = cs.num_advice, cs.num_instance
    blinding, deg = cs.blinding_factors, cs.degree()
    usable = n - blinding - 1
    omega, delta = dom.omega, FR_DELTA
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    counts = (cs.num_fixed, A, I)
    # the seeds of the blinding: advice, permuted columns, z columns, random polynomial; the circuit's number above the 58 bits of the base
    base = (int(seed) & 0xFFFFFFFFFFFF) << 10
    bases = [base | (c << 58) for c in range(m)]
    d = lambda values: _dev(values, device)
    ck = lambda kind, index, c: (kind, index, c)            # the key of what belongs to circuit c
    commits = {}
    progs = _Programs()

    def commit(key_cols, handle):
        com = best_multiexp_batch([c for _, c in key_cols], handle)
        for (key, _), c in zip(key_cols, com):
            commits[key] = g1_words_to_int(c)
            transcript.write_point(commits[key])

    commit_lagrange = lambda key_cols: commit(key_cols, params.g_lagrange_handle)
    commit_coeff = lambda key_cols: commit(key_cols, params.g_handle)

    # ---- the columns -----------------------------------------------------------------------------------------------------------------------
    adv = torch.stack(list(advice), dim=1)                                   # (A, m, n, 4), a copy: adv[i] is column i of every circuit
    for c in range(m):
        adv[:, c, usable:] = random_fr(A * (n - usable), bases[c], device, shape=(A, n - usable, 4))
    for i in cs.unblinded_advice:                                            # the draw above is the same with or without them
        adv[i, :, usable:] = 0
    inst_cols = [instance_values(cs, instance) for instance in instances]
    inst = torch.zeros((I, m, n, 4), dtype=torch.int64, device=device)
    for c in range(m):
        for i, values in enumerate(inst_cols[c]):
            if len(values) > usable:
                raise ValueError(f"{who}: too many instance values")
            if values:
                inst[i, c, :len(values)] = d(values)
    fixed = pk.fixed_values
    table = [fixed[i] for i in range(cs.num_fixed)] + [adv[i] for i in range(A)] + [inst[i] for i in range(I)]

    transcript = WRITERS[encoding]()
    transcript.common_scalar(vk_digest(vk))
    for c in range(m):
        for values in inst_cols[c]:
            for v in values:
                transcript.common_scalar(v)
    commit_lagrange([(ck("advice", i, c), adv[i, c]) for c in range(m) for i in range(A)])
    theta = transcript.squeeze_challenge()

    try:
        # ---- the lookups: permuted columns (lookup j of circuit c at index c L + j) ------------------------------------------------------------
        lk_in = [progs.run(("in", j), [_compress(ins)], counts, table, m, n, theta=theta) for j, (ins, _) in enumerate(cs.lookups)]
        lk_tab = [progs.run(("tab", j), [_compress(tabs)], counts, table, m, n, theta=theta) for j, (_, tabs) in enumerate(cs.lookups)]
        order = [(c, j) for c in range(m) for j in range(L)]
        permuted = permute_expression_pairs([lk_in[j][c] for c, j in order], [lk_tab[j][c] for c, j in order], usable,
                                            blinding_seeds=[bases[c] + 0x40 + 2 * j for c, j in order]) if L else []
        commit_lagrange([pair for (c, j), (a, s) in zip(order, permuted) for pair in ((ck("lookup_a", j, c), a), (ck("lookup_s", j, c), s))])
        beta = transcript.squeeze_challenge()
        gamma = transcript.squeeze_challenge()

        # ---- the permutation argument: one z per chunk of columns, chained at the last usable row inside its circuit ---------------------------
        by_kind = {"advice": lambda i: adv[i], "fixed": lambda i: fixed[i], "instance": lambda i: inst[i]}
        perm_cols = [by_kind[kind](i) for kind, i in cs.equality]
        sigma = pk.permutation_values
        acc, xs = 1, []
        for _ in range(n):
            xs.append(acc)
            acc = acc * omega % R
        x_col = d(xs)
        mul2 = [ev.Advice(0) * ev.Advice(1)]
        factors = []                                                        # per set: (m, n, 4)
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
            den = progs.run(("den", s0), [den_e], (0, len(cols), 0), cols, m, n, beta=beta, gamma=gamma)
            num = progs.run(("num", s0), [num_e], (0, len(cols), 0), cols, m, n, beta=beta, gamma=gamma)
            batch_invert(den.reshape(m * n, 4))
            factors.append(progs.run("mul2", mul2, (0, 2, 0), [num, den], m, n))
        # the chain of grand_product_batch runs from one set to the next, so a circuit's sets are one call
        zs = [grand_product_batch([f[c] for f in factors], fr_words(1), chain_row=usable) if factors else [] for c in range(m)]
        for c in range(m):
            for i, z in enumerate(zs[c]):
                z[usable + 1:] = random_fr(n - usable - 1, bases[c] + 0x80 + i, device)
        commit_lagrange([(ck("perm_z", i, c), z) for c in range(m) for i, z in enumerate(zs[c])])

        # ---- the lookup arguments' z ----------------------------------------------------------------------------------------------------------------
        pair = [(ev.Advice(0) + ev.BETA) * (ev.Advice(1) + ev.GAMMA)]
        lk_z = [[] for _ in range(m)]
        if L:
            stacked = lambda ts: torch.stack(list(ts))                    # (m L, n, 4): the lookups of all circuits as the segments
            num = progs.run("pair", pair, (0, 2, 0), [stacked(lk_in[j][c] for c, j in order), stacked(lk_tab[j][c] for c, j in order)], m * L, n,
                            beta=beta, gamma=gamma)
            den = progs.run("pair", pair, (0, 2, 0), [stacked(a for a, _ in permuted), stacked(s for _, s in permuted)], m * L, n,
                            beta=beta, gamma=gamma)
            batch_invert(den.reshape(m * L * n, 4))
            lk_factors = progs.run("mul2", mul2, (0, 2, 0), [num, den], m * L, n)
            flat = grand_product_batch([lk_factors[i] for i in range(m * L)], fr_words(1))
            for (c, j), z in zip(order, flat):
                z[usable + 1:] = random_fr(n - usable - 1, bases[c] + 0xC0 + j, device)
                lk_z[c].append(z)
        commit_lagrange([(ck("lookup_z", j, c), z) for c in range(m) for j, z in enumerate(lk_z[c])])
    finally:
        progs.destroy()
    perm_of = [[permuted[c * L + j] for j in range(L)] for c in range(m)]

    # ---- the vanishing argument's random polynomial (one per proof), then h ------------------------------------------------------------------------
    random_poly = random_fr(n, base + 0x100, device)
    commit_coeff([(("random",), random_poly)])
    y = transcript.squeeze_challenge()

    g, tab = circuits.evaluate_h_program(cs, k, dom.extended_k, delta, divide=False)
    V = nsets + 3 * L + A + I                                               # the columns of its own that a circuit brings to h
    lagrange = [col for c in range(m)
                for col in zs[c] + [t for j in range(L) for t in (lk_z[c][j], perm_of[c][j][0], perm_of[c][j][1])] + [adv[i, c] for i in range(A)]
                + [inst[i, c] for i in range(I)]]
    var_coeffs = dom.lagrange_to_coeff(torch.stack(lagrange)).reshape(m, V, n, 4)
    z_polys, lk_polys = var_coeffs[:, :nsets], var_coeffs[:, nsets:nsets + 3 * L]
    adv_polys = var_coeffs[:, nsets + 3 * L:nsets + 3 * L + A]
    sel = dom.lagrange_to_coeff(torch.stack([pk.l0, pk.l_last, pk.l_active]))
    x_poly = d([0, 1] + [0] * (n - 2)).reshape(1, n, 4)
    shared = dom.coeff_to_extended(torch.cat([pk.fixed_polys, pk.permutation_polys, sel, x_poly]))
    n_shared = shared.shape[0]
    assert n_shared + nsets + 3 * L == tab.t_inv
    rot_scale = 1 << (dom.extended_k - k)
    en = dom.extended_len()
    unread = torch.zeros((max(rot_scale, 2), 4), dtype=torch.int64, device=device)[:rot_scale]     # the table's t_inv entry: divide=False never reads it
    prog = g.compile(tab.num_fixed_entries, A, I, rot_scale=rot_scale, short_columns=tab.short_columns)
    h_ext = torch.zeros((en, 4), dtype=torch.int64, device=device)
    # the program's table: fixed, sigma | z | l0, l_last, l_active, x | lookups | t_inv || advice | instance
    n_fs = cs.num_fixed + P
    step = max(1, H_COLUMN_BUDGET // max(V * en * 32, 1))                   # circuits whose extended columns are in flight together
    try:
        for c0 in range(0, m, step):
            mc = min(step, m - c0)
            ext = dom.coeff_to_extended(var_coeffs[c0:c0 + mc].reshape(mc * V, n, 4)).reshape(mc, V, en, 4)
            own = lambda v: ext[0, v]
            cols = ([shared[i] for i in range(n_fs)] + [own(i) for i in range(nsets)] + [shared[i] for i in range(n_fs, n_shared)]
                    + [own(nsets + i) for i in range(3 * L)] + [unread] + [own(nsets + 3 * L + i) for i in range(A + I)])
            strides = ([0] * n_fs + [V * en * 8] * nsets + [0] * (n_shared - n_fs) + [V * en * 8] * (3 * L) + [0] + [V * en * 8] * (A + I))
            prog.evaluate_circuits(cols, strides, h_ext, mc, beta=beta, gamma=gamma, theta=theta, y=y)     # chained through PreviousValue
            del ext
    finally:
        prog.destroy()
    dom.divide_by_vanishing_poly(h_ext)
    h_coeff = dom.extended_to_coeff(h_ext)                      # ((deg - 1) n, 4): in place on h_ext
    pieces = [h_coeff[i * n:(i + 1) * n] for i in range(deg - 1)]
    commit_coeff([(("h_piece", i), p) for i, p in enumerate(pieces)])
    x = transcript.squeeze_challenge()

    # ---- the evaluations ----------------------------------------------------------------------------------------------------------------------
    adv_q, fix_q, _ = cs.queries()
    last = -(blinding + 1)
    rot = lambda r: x * pow(omega, r, R) % R
    polys = {("random",): random_poly}
    for c in range(m):
        for i in range(A):
            polys[ck("advice", i, c)] = adv_polys[c, i]
    for i in range(cs.num_fixed):
        polys[("fixed", i)] = pk.fixed_polys[i]
    for j in range(P):
        polys[("sigma", j)] = pk.permutation_polys[j]
    for c in range(m):
        for i in range(nsets):
            polys[ck("perm_z", i, c)] = z_polys[c, i]
    for c in range(m):
        for j in range(L):
            polys[ck("lookup_z", j, c)], polys[ck("lookup_a", j, c)], polys[ck("lookup_s", j, c)] = (
                lk_polys[c, 3 * j], lk_polys[c, 3 * j + 1], lk_polys[c, 3 * j + 2])
    polys[("h",)] = linear_combination(pieces, np.stack([fr_words(pow(x, n * i, R)) for i in range(deg - 1)]))
    wanted = [(ck("advice", i, c), rot(r)) for c in range(m) for i, r in adv_q]
    wanted += [(("fixed", i), rot(r)) for i, r in fix_q] + [(("random",), x)]
    wanted += [(("sigma", j), x) for j in range(P)]
    for c in range(m):
        for i in range(nsets):
            wanted += [(ck("perm_z", i, c), x), (ck("perm_z", i, c), rot(1))] + ([(ck("perm_z", i, c), rot(last))] if i + 1 < nsets else [])
    for c in range(m):
        for j in range(L):
            wanted += [(ck("lookup_z", j, c), x), (ck("lookup_z", j, c), rot(1)), (ck("lookup_a", j, c), x), (ck("lookup_a", j, c), rot(-1)),
                       (ck("lookup_s", j, c), x)]
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
    queries = []
    for c in range(m):
        queries += [q(ck("advice", i, c), rot(r)) for i, r in adv_q]
        queries += [qq for i in range(nsets) for qq in (q(ck("perm_z", i, c), x), q(ck("perm_z", i, c), rot(1)))]
        queries += [q(ck("perm_z", i, c), rot(last)) for i in reversed(range(nsets - 1))]
        for j in range(L):
            queries += [q(ck("lookup_z", j, c), x), q(ck("lookup_a", j, c), x), q(ck("lookup_s", j, c), x), q(ck("lookup_a", j, c), rot(-1)),
                        q(ck("lookup_z", j, c), rot(1))]
    queries += [q(("fixed", i), rot(r)) for i, r in fix_q] + [q(("sigma", j), x) for j in range(P)]
    queries += [(("h",), x, hx), q(("random",), x)]
    (gwc.create_opening if multiopen == "gwc" else create_opening)(params, transcript, queries, polys)
    if _trace is not None:
        _trace.update(polys=polys, commits=commits,
                      lagrange={"advice": [adv[:, c] for c in range(m)], "perm_z": zs, "lookup_z": lk_z, "permuted": perm_of},
                      pieces=pieces, challenges=dict(theta=theta, beta=beta, gamma=gamma, y=y, x=x))
    return transcript.finalize()


def create_proofs(params, pk: ProvingKey, advice, instances, seeds, encoding: str = "halo2", multiopen: str = "shplonk") -> list:
    """m independent proofs of ``pk``'s constraint system in one batched pass: ``create_proofs(...)[b] == create_proof(params, pk,
    advice[b], instances[b], seeds[b])``, byte for byte.  ``advice``: the (m, num_advice, n, 4) GPU tensor a witness writer returns, or
    a list of m (num_advice, n, 4) tensors; ``instances``: m entries, each in the form ``create_proof`` takes; ``seeds``: m integers,
    pairwise distinct mod 2^48 (two proofs with one seed would share their blinding: ValueError), or ONE integer s standing for
    s, s + 1, ...  m >= 1, no upper limit.  ``encoding``, ``multiopen``: as in ``create_proof``."""
    who = "create_proofs"
    check_encoding(encoding, who)
    check_multiopen(multiopen, who)
    if _is_tensor(advice):
        if advice.dim() != 4:
            raise ValueError(f"{who}: advice must be a (m, num_advice, n, 4) GPU tensor or a list of m (num_advice, n, 4) tensors")
        advice = [advice[c] for c in range(advice.shape[0])]
    elif not isinstance(advice, (list, tuple)):
        raise ValueError(f"{who}: advice must be a (m, num_advice, n, 4) GPU tensor or a list of m (num_advice, n, 4) tensors")
    advice = list(advice)
    m = len(advice)
    if m < 1:
        raise ValueError(f"{who}: at least one proof")
    if _is_tensor(instances) or isinstance(instances, np.ndarray) or len(instances) != m:
        raise ValueError(f"{who}: {m} proof(s) need {m} instance entries")
    if isinstance(seeds, (int, np.integer)):
        seeds = [int(seeds) + b for b in range(m)]
    seeds = [int(s) for s in seeds]
    if len(seeds) != m:
        raise ValueError(f"{who}: {m} proof(s) need {m} seeds")
    if len({s & 0xFFFFFFFFFFFF for s in seeds}) != m:
        raise ValueError(f"{who}: the seeds must be pairwise distinct mod 2^48 (two proofs would share their blinding)")
    return _create_proofs(who, params, pk, advice, list(instances), seeds, encoding, multiopen)


def _create_proofs(who, params, pk, advice, instances, seeds, encoding: str = "halo2", multiopen: str = "shplonk") -> list:
    """The protocol of ``_create_proof`` (module docstring, steps 1 - 14) for m transcripts of one circuit each; the comments name the
    step.  What belongs to proof b carries b where ``_create_proof`` carries the circuit's number; the key inside a proof is circuit 0's."""
    import torch

    m = len(advice)
    vk = pk.vk
    cs, dom = vk.cs, vk.domain
    k, n = dom.k, 1 << dom.k
    if params.k != k:
        raise ValueError(f"{who}: the parameters and the key differ in k")
    for a in advice:
        if not _is_tensor(a) or not a.is_cuda or tuple(a.shape) != (cs.num_advice, n, 4):
            raise ValueError(f"{who}: advice must be a ({cs.num_advice}, {n}, 4) GPU tensor" + (" per proof" if m > 1 else ""))
    device = advice[0].device
    A, I = cs.num_advice, cs.num_instance
    blinding, deg = cs.blinding_factors, cs.degree()
    usable = n - blinding - 1
    omega, delta = dom.omega, FR_DELTA
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    counts = (cs.num_fixed, A, I)
    bases = [(s & 0xFFFFFFFFFFFF) << 10 for s in seeds]         # create_proof's streams of circuit 0, per proof
    d = lambda values: _dev(values, device)
    ck = lambda kind, index: (kind, index, 0)
    every = range(m)
    progs = _Programs()

    def commit(per_proof, handle):
        """one best_multiexp_batch over all proofs' columns; every transcript then absorbs its own points, in its own order"""
        flat = [c for cols in per_proof for c in cols]
        com = best_multiexp_batch(flat, handle) if flat else []
        at = 0
        for b, cols in enumerate(per_proof):
            for _ in cols:
                transcripts[b].write_point(g1_words_to_int(com[at]))
                at += 1

    commit_lagrange = lambda per_proof: commit(per_proof, params.g_lagrange_handle)
    commit_coeff = lambda per_proof: commit(per_proof, params.g_handle)

    # ---- the columns (steps 1 - 3) -------------------------------------------------------------------------------------------------------------
    adv = torch.stack(list(advice), dim=1)                                   # (A, m, n, 4), a copy: adv[i] is column i of every proof
    for b in every:
        adv[:, b, usable:] = random_fr(A * (n - usable), bases[b], device, shape=(A, n - usable, 4))
    for i in cs.unblinded_advice:
        adv[i, :, usable:] = 0
    inst_cols = [instance_values(cs, instance) for instance in instances]
    inst = torch.zeros((I, m, n, 4), dtype=torch.int64, device=device)
    for b in every:
        for i, values in enumerate(inst_cols[b]):
            if len(values) > usable:
                raise ValueError(f"{who}: too many instance values")
            if values:
                inst[i, b, :len(values)] = d(values)
    fixed = pk.fixed_values
    table = [fixed[i] for i in range(cs.num_fixed)] + [adv[i] for i in range(A)] + [inst[i] for i in range(I)]

    digest = vk_digest(vk)
    transcripts = [WRITERS[encoding]() for _ in every]
    for b, tr in enumerate(transcripts):
        tr.common_scalar(digest)
        for values in inst_cols[b]:
            for v in values:
                tr.common_scalar(v)
    commit_lagrange([[adv[i, b] for i in range(A)] for b in every])
    theta = [tr.squeeze_challenge() for tr in transcripts]                    # step 4

    try:
        # ---- the lookups: permuted columns (step 5; lookup j of proof b at index b L + j) ------------------------------------------------------
        thetas = [dict(theta=t) for t in theta]
        lk_in = [progs.run_proofs(("in", j), [_compress(ins)], counts, table, n, thetas) for j, (ins, _) in enumerate(cs.lookups)]
        lk_tab = [progs.run_proofs(("tab", j), [_compress(tabs)], counts, table, n, thetas) for j, (_, tabs) in enumerate(cs.lookups)]
        order = [(b, j) for b in every for j in range(L)]
        try:
            permuted = permute_expression_pairs([lk_in[j][b] for b, j in order], [lk_tab[j][b] for b, j in order], usable,
                                                blinding_seeds=[bases[b] + 0x40 + 2 * j for b, j in order]) if L else []
        except _lib.Halo2Mi355xError as e:                                    # what create_proof raises, naming the proof
            where = [order[i] for i in getattr(e, "missing", [])]
            err = _lib.Halo2Mi355xError(e.code, f"{e} -- " + ", ".join(f"proof {b} (lookup {j})" for b, j in where))
            err.missing, err.proofs = [j for _, j in where], sorted({b for b, _ in where})
            raise err from None
        commit_lagrange([[t for j in range(L) for t in permuted[b * L + j]] for b in every])
        beta = [tr.squeeze_challenge() for tr in transcripts]                 # step 6
        gamma = [tr.squeeze_challenge() for tr in transcripts]
        bg = [dict(beta=beta[b], gamma=gamma[b]) for b in every]

        # ---- the permutation argument (step 7): one z per chunk of columns, chained at the last usable row inside its proof ----------------
        by_kind = {"advice": lambda i: adv[i], "fixed": lambda i: fixed[i], "instance": lambda i: inst[i]}
        perm_cols = [by_kind[kind](i) for kind, i in cs.equality]
        sigma = pk.permutation_values
        acc, xs = 1, []
        for _ in range(n):
            xs.append(acc)
            acc = acc * omega % R
        x_col = d(xs)
        mul2 = [ev.Advice(0) * ev.Advice(1)]
        nothing = [{} for _ in every]
        factors = []                                                        # per set: (m, n, 4)
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
            den = progs.run_proofs(("den", s0), [den_e], (0, len(cols), 0), cols, n, bg)
            num = progs.run_proofs(("num", s0), [num_e], (0, len(cols), 0), cols, n, bg)
            batch_invert(den.reshape(m * n, 4))
            factors.append(progs.run_proofs("mul2", mul2, (0, 2, 0), [num, den], n, nothing))
        # grand_product_batch chains from one column to the next and must start at 1 in every proof: one call per proof, as per circuit
        zs = [grand_product_batch([f[b] for f in factors], fr_words(1), chain_row=usable) if factors else [] for b in every]
        for b in every:
            for i, z in enumerate(zs[b]):
                z[usable + 1:] = random_fr(n - usable - 1, bases[b] + 0x80 + i, device)
        commit_lagrange([list(zs[b]) for b in every])

        # ---- the lookup arguments' z (step 8): the lookups of all proofs as the proofs of one launch ------------------------------------------
        pair = [(ev.Advice(0) + ev.BETA) * (ev.Advice(1) + ev.GAMMA)]
        lk_z = [[] for _ in every]
        if L:
            stacked = lambda ts: torch.stack(list(ts))                    # (m L, n, 4)
            bg_l = [bg[b] for b, _ in order]
            num = progs.run_proofs("pair", pair, (0, 2, 0), [stacked(lk_in[j][b] for b, j in order), stacked(lk_tab[j][b] for b, j in order)], n, bg_l)
            den = progs.run_proofs("pair", pair, (0, 2, 0), [stacked(a for a, _ in permuted), stacked(s for _, s in permuted)], n, bg_l)
            batch_invert(den.reshape(m * L * n, 4))
            lk_factors = progs.run_proofs("mul2", mul2, (0, 2, 0), [num, den], n, [{} for _ in order])
            flat = grand_product_batch([lk_factors[i] for i in range(m * L)], fr_words(1))
            for (b, j), z in zip(order, flat):
                z[usable + 1:] = random_fr(n - usable - 1, bases[b] + 0xC0 + j, device)
                lk_z[b].append(z)
        commit_lagrange([list(lk_z[b]) for b in every])
    finally:
        progs.destroy()
    perm_of = [[permuted[b * L + j] for j in range(L)] for b in every]

    # ---- the vanishing argument's random polynomial (step 9: one per PROOF), y (step 10), then h ------------------------------------------------
    random_polys = [random_fr(n, bases[b] + 0x100, device) for b in every]
    commit_coeff([[random_polys[b]] for b in every])
    y = [tr.squeeze_challenge() for tr in transcripts]

    g, tab = circuits.evaluate_h_program(cs, k, dom.extended_k, delta, divide=False)
    V = nsets + 3 * L + A + I                                               # the columns of its own that a proof brings to h
    lagrange = [col for b in every
                for col in zs[b] + [t for j in range(L) for t in (lk_z[b][j], perm_of[b][j][0], perm_of[b][j][1])] + [adv[i, b] for i in range(A)]
                + [inst[i, b] for i in range(I)]]
    var_coeffs = dom.lagrange_to_coeff(torch.stack(lagrange)).reshape(m, V, n, 4)
    z_polys, lk_polys = var_coeffs[:, :nsets], var_coeffs[:, nsets:nsets + 3 * L]
    adv_polys = var_coeffs[:, nsets + 3 * L:nsets + 3 * L + A]
    sel = dom.lagrange_to_coeff(torch.stack([pk.l0, pk.l_last, pk.l_active]))
    x_poly = d([0, 1] + [0] * (n - 2)).reshape(1, n, 4)
    shared = dom.coeff_to_extended(torch.cat([pk.fixed_polys, pk.permutation_polys, sel, x_poly]))
    n_shared = shared.shape[0]
    assert n_shared + nsets + 3 * L == tab.t_inv
    rot_scale = 1 << (dom.extended_k - k)
    en = dom.extended_len()
    unread = torch.zeros((max(rot_scale, 2), 4), dtype=torch.int64, device=device)[:rot_scale]     # the table's t_inv entry: divide=False never reads it
    prog = g.compile(tab.num_fixed_entries, A, I, rot_scale=rot_scale, short_columns=tab.short_columns)
    h_ext = torch.zeros((m, en, 4), dtype=torch.int64, device=device)
    n_fs = cs.num_fixed + P
    step = max(1, H_COLUMN_BUDGET // max(V * en * 32, 1))                   # proofs whose extended columns are in flight together
    stride = V * en * 8
    try:
        for b0 in range(0, m, step):
            mb = min(step, m - b0)
            ext = dom.coeff_to_extended(var_coeffs[b0:b0 + mb].reshape(mb * V, n, 4)).reshape(mb, V, en, 4)
            own = lambda v: (ext[0, v], stride)
            cols = ([shared[i] for i in range(n_fs)] + [own(i) for i in range(nsets)] + [shared[i] for i in range(n_fs, n_shared)]
                    + [own(nsets + i) for i in range(3 * L)] + [unread] + [own(nsets + 3 * L + i) for i in range(A + I)])
            prog.evaluate_proofs(cols, h_ext[b0:b0 + mb],
                                 [dict(beta=beta[b], gamma=gamma[b], theta=theta[b], y=y[b]) for b in range(b0, b0 + mb)])
            del ext
    finally:
        prog.destroy()
    dom.divide_by_vanishing_poly(h_ext)
    h_coeff = dom.extended_to_coeff(h_ext)                      # (m, (deg - 1) n, 4): in place on h_ext
    pieces = [[h_coeff[b, i * n:(i + 1) * n] for i in range(deg - 1)] for b in every]
    commit_coeff(pieces)                                                      # step 11
    x = [tr.squeeze_challenge() for tr in transcripts]                        # step 12

    # ---- the evaluations (step 13): one eval_polynomial over all proofs ----------------------------------------------------------------------
    adv_q, fix_q, _ = cs.queries()
    last = -(blinding + 1)
    h_polys = linear_combination_batch(pieces, [[pow(x[b], n * i, R) for i in range(deg - 1)] for b in every])
    common = {}
    for i in range(cs.num_fixed):
        common[("fixed", i)] = pk.fixed_polys[i]
    for j in range(P):
        common[("sigma", j)] = pk.permutation_polys[j]
    polys_of, wanted_of = [], []
    for b in every:
        rot = lambda r, xb=x[b]: xb * pow(omega, r, R) % R
        polys = {("random",): random_polys[b]}
        for i in range(A):
            polys[ck("advice", i)] = adv_polys[b, i]
        polys.update(common)
        for i in range(nsets):
            polys[ck("perm_z", i)] = z_polys[b, i]
        for j in range(L):
            polys[ck("lookup_z", j)], polys[ck("lookup_a", j)], polys[ck("lookup_s", j)] = (
                lk_polys[b, 3 * j], lk_polys[b, 3 * j + 1], lk_polys[b, 3 * j + 2])
        polys[("h",)] = h_polys[b]
        wanted = [(ck("advice", i), rot(r)) for i, r in adv_q]
        wanted += [(("fixed", i), rot(r)) for i, r in fix_q] + [(("random",), x[b])]
        wanted += [(("sigma", j), x[b]) for j in range(P)]
        for i in range(nsets):
            wanted += [(ck("perm_z", i), x[b]), (ck("perm_z", i), rot(1))] + ([(ck("perm_z", i), rot(last))] if i + 1 < nsets else [])
        for j in range(L):
            wanted += [(ck("lookup_z", j), x[b]), (ck("lookup_z", j), rot(1)), (ck("lookup_a", j), x[b]), (ck("lookup_a", j), rot(-1)),
                       (ck("lookup_s", j), x[b])]
        polys_of.append(polys)
        wanted_of.append(wanted + [(("h",), x[b])])                           # h(x) is evaluated with the rest and not written
    slots, index = [], {}
    for b in every:
        for key, poly in polys_of[b].items():
            at = (key,) if key in common else (key, b)
            if at not in index:
                index[at] = len(slots)
                slots.append(poly)
    at_of = lambda b, key: index[(key,) if key in common else (key, b)]
    flat = [(b, key, pt) for b in every for key, pt in wanted_of[b]]
    vals = words_to_ints(eval_polynomial(torch.stack(slots), np.stack([fr_words(pt) for _, _, pt in flat]),
                                         poly_index=np.array([at_of(b, key) for b, key, _ in flat], dtype=np.uint32)))
    evals_of = [{} for _ in every]
    for (b, key, pt), v in zip(flat, vals):
        evals_of[b][(key, pt)] = v
        if key != ("h",):
            transcripts[b].write_scalar(v)

    # ---- the multiopen (step 14): upstream's order of queries, per proof -----------------------------------------------------------------------
    queries_of = []
    for b in every:
        rot = lambda r, xb=x[b]: xb * pow(omega, r, R) % R
        q = lambda key, pt, e=evals_of[b]: (key, pt, e[(key, pt)])
        queries = [q(ck("advice", i), rot(r)) for i, r in adv_q]
        queries += [qq for i in range(nsets) for qq in (q(ck("perm_z", i), x[b]), q(ck("perm_z", i), rot(1)))]
        queries += [q(ck("perm_z", i), rot(last)) for i in reversed(range(nsets - 1))]
        for j in range(L):
            queries += [q(ck("lookup_z", j), x[b]), q(ck("lookup_a", j), x[b]), q(ck("lookup_s", j), x[b]), q(ck("lookup_a", j), rot(-1)),
                        q(ck("lookup_z", j), rot(1))]
        queries += [q(("fixed", i), rot(r)) for i, r in fix_q] + [q(("sigma", j), x[b]) for j in range(P)]
        queries += [q(("h",), x[b]), q(("random",), x[b])]
        queries_of.append(queries)
    (gwc.create_openings if multiopen == "gwc" else create_openings)(params, transcripts, queries_of, polys_of)
    return [tr.finalize() for tr in transcripts]
