"""``create_proof`` of ``halo2_proofs::plonk`` over KZG with the SHPLONK multiopen, for one circuit (``create_proof``) or for m circuits of
one constraint system in a single transcript (``create_proof_multi``, upstream's ``&[circuit; m]``), or T independent proofs of one
circuit each in one batched pass (``create_proofs``): ONE body of protocol code, ``_prove``, for T transcripts of m circuits each, with
every polynomial step on the device entry points (DESIGN.md sections 17, 19 and 21).  ``create_proof`` is T = m = 1,
``create_proof_multi`` T = 1, ``create_proofs`` m = 1; no entry has both above 1.  What belongs to a circuit is indexed by its unit
u = t m + c, what belongs to a transcript by t.

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

Per phase ONE batched call carries all units: ``best_multiexp_batch`` over units x columns (every transcript then absorbs its own
points, in unit order), one stacked ``lagrange_to_coeff`` / ``coeff_to_extended``, one ``permute_expression_pairs``, one ``batch_invert``
per argument, one ``eval_polynomial`` over deduplicated polynomials (h(x) with the rest, not written), ``linear_combination_batch``; the
helper graph programs are compiled once per call and run through ``_Programs.run_proofs``, every unit carrying its transcript's
theta / beta / gamma.  The shape chooses the device call in two places, each stated once.  The helper programs: the circuits of ONE
transcript are the segments of ``CompiledGraph.evaluate``; the units of several go through ``evaluate_proofs``, the shared columns at
stride 0.  The h step: with m = 1 the transcripts are the proofs of ``evaluate_proofs``; otherwise a transcript's circuits go through
``evaluate_circuits``, chained through PreviousValue.  Either way in chunks when the units' own extended columns pass
``H_COLUMN_BUDGET`` (2 GiB, the witness writers' convention).  The permutation products are one ``grand_product_batch`` per unit: its
chain runs from one column set to the next and must start at 1 in every circuit.  The multiopen is ``create_opening`` for one
transcript and ``create_openings`` for several (the one-proof call of the batched form is slower, see HISTORY.md).

Nothing but the blinding is random, and it comes from ``random_fr(seed + ...)``: a seed fixes the bytes.  The advice columns named in
``cs.unblinded_advice`` keep zeros in their last rows (the draw for the other columns is what it is without them), so their commitments
are ``commit_lagrange`` of the witness columns themselves: what ``solvency`` opens.  ``base`` = the low 48 bits of
``seed`` shifted by 10 (58 bits; ``create_proof``'s derivation, kept so that its bytes stay) names the streams of circuit 0: + 0 advice,
+ 0x40 + 2 j / + 1 the permuted columns of lookup j, + 0x80 + i the permutation z, + 0xC0 + j the lookup z, + 0x100 the random
polynomial (drawn once per proof).  Circuit c uses ``base | c << 58``: the 6 bits above the base, hence at most 64 circuits; no two
circuits of a proof and no two seeds (mod 2^48) share a stream.

``create_proofs`` makes INDEPENDENT proofs of one key -- one per user of a solvency tree -- in one batched pass: proof b is byte for
byte ``create_proof(params, pk, advice[b], instances[b], seeds[b])``, with its own transcript, challenges, random polynomial and h.
The bytes of all three entries are pinned to recordings (tests/test_prover_bytes_gpu.py, tests/golden/prover_digests.json).

``multiopen="gwc"`` on the three entries ends the proof in the GWC multiopen instead (step 14: ``gwc.create_opening`` /
``gwc.create_openings``, one witness point per distinct query point); everything before step 14 is the same code and the same bytes.

``lookup="logup"`` on the three entries proves the lookups with the logarithmic-derivative argument instead (the
proof format of this mode is this project's own, after Haboeck's logUp paper, not the bytes of any fork).  The lookups are grouped
into the arguments of ``cs.logup_arguments()``; the order above stands with two substitutions: at step 5, per circuit and per
argument, the commitment of the multiplicity column m takes the place of the permuted pair (``logup_multiplicities``, nothing is
sorted for small tables), and at step 8 the commitment of the running sum phi takes the place of the lookup z (the denominators
f_j + beta and t + beta of all arguments and units from ONE helper program and ONE ``batch_invert``, the terms from one program per
number of inputs, ``grand_sum_batch``).  gamma is still drawn.  The evaluations per circuit and argument are phi(x), phi(wx), m(x),
the queries phi(x), m(x), phi(wx).  The blinding of m (rows from u on) comes from stream + 0x40 + 2 g, that of phi (rows from u + 1
on) from + 0xC0 + g.  The keys are the same: the grouping never raises the degree.  Without lookups the bytes are those of the default argument."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from . import circuits, evaluation as ev
from ._marshal import _is_tensor
from . import _lib
from .arithmetic import (batch_invert, best_multiexp_batch, eval_polynomial, grand_product_batch, grand_sum_batch, linear_combination_batch,
                         logup_multiplicities, permute_expression_pairs, random_fr)
from .domain import FR_MODULUS, FR_ZETA, fr_words
from .keygen import FR_DELTA, ProvingKey, VerifyingKey
from .poseidon import ints_to_words, words_to_ints
from . import gwc, shplonk
from .shplonk import g1_words_to_int
from .transcript import WRITERS, check_encoding, check_lookup, check_multiopen

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
    """the helper graph programs of one call -- compressed lookups, permutation numerators and denominators, products -- compiled once
    each, whatever the number of circuits and transcripts, and destroyed together"""

    def __init__(self, one_transcript: bool):
        self._progs, self._tiled, self._one = {}, {}, one_transcript

    def run_proofs(self, name, exprs, counts, columns, n, constants):
        """the value of one expression on the n rows of each of ``len(constants)`` units in ONE launch, unit u with its own
        ``constants[u]`` (a dict of theta / beta / gamma): a column is (units, n, 4) or (n, 4), shared; a rotation wraps inside its
        unit.  -> (units, n, 4).  The one place where the shape chooses the helpers' device call: the units of ONE transcript share
        their constants and are the segments of ``CompiledGraph.evaluate``, which takes the constants as arguments (the
        constants table of ``evaluate_proofs`` cost create_proof_multi 0.4 ms at four circuits); a shared column is then tiled,
        once per call of the prover.  Units of several transcripts go through ``evaluate_proofs``, shared columns at stride 0."""
        import torch
        if name not in self._progs:
            g = ev.GraphEvaluator()
            g.add_custom_gates(exprs)
            self._progs[name] = g.compile(*counts)
        units = len(constants)
        out = torch.zeros((units, n, 4), dtype=torch.int64, device=columns[0].device)
        if not self._one:
            self._progs[name].evaluate_proofs(list(columns), out, constants)
            return out
        def rows(c):
            if c.dim() == 3:
                return c.reshape(units * n, 4)
            if units == 1:
                return c
            key = (c.data_ptr(), units)
            if key not in self._tiled:
                self._tiled[key] = (c, c.expand(units, n, 4).reshape(units * n, 4))      # c is kept: its address is the key
            return self._tiled[key][1]
        self._progs[name].evaluate([rows(c) for c in columns], out.reshape(units * n, 4), segments=units, **constants[0])
        return out

    def destroy(self):
        for prog in self._progs.values():
            prog.destroy()
        self._progs, self._tiled = {}, {}


def _compress(exprs):
    acc = ev.Constant(0)
    for e in exprs:
        acc = acc * ev.THETA + e
    return acc


MAX_CIRCUITS = 64                   # the circuit's number sits in the 6 seed bits above the 58 of ``base``
H_COLUMN_BUDGET = 2 << 30           # bytes of per-circuit extended columns in flight in the h step (the witness writers' 2 GiB)


def create_proof(params, pk: ProvingKey, advice, instance, seed: int, _trace: dict = None, encoding: str = "halo2",
                 multiopen: str = "shplonk", lookup: str = "halo2") -> bytes:
    """The proof bytes for the witness ``advice`` -- the (num_advice, n, 4) device tensor a witness writer returns for one circuit --
    and its ``instance`` values.  One circuit per proof: a list of several witnesses, or a 4-dimensional tensor holding more than
    one, raises ValueError (``create_proof_multi`` takes several).  ``_trace``: a dict that receives the committed polynomials and
    their commitments (tests).  ``encoding``: "halo2" -- Blake2b transcript, compressed points, little-endian scalars -- or "evm" --
    Keccak transcript, uncompressed big-endian points and scalars (``transcript`` states both); the protocol is the same.
    ``multiopen``: "shplonk", or "gwc" -- the proof then ends in one witness point per distinct query point (``gwc``) where SHPLONK
    writes two points; everything before the multiopen is byte for byte the same.  ``lookup``: "halo2", the permutation-based lookup
    argument, or "logup", the logarithmic-derivative one (the module docstring's last paragraph); the same keys prove under either."""
    check_encoding(encoding, "create_proof")
    check_multiopen(multiopen, "create_proof")
    check_lookup(lookup, "create_proof")
    if isinstance(advice, (list, tuple)):
        if len(advice) != 1:
            raise ValueError("create_proof: one circuit per proof (create_proof_multi proves several)")
        advice = advice[0]
    if _is_tensor(advice) and advice.dim() == 4:
        if advice.shape[0] != 1:
            raise ValueError("create_proof: one circuit per proof (create_proof_multi proves several)")
        advice = advice[0]
    trace = None if _trace is None else {}
    proof = _prove("create_proof", params, pk, [advice], [instance], [seed], 1, encoding, multiopen, trace, lookup)[0]
    if _trace is not None:                                 # one circuit: its keys without the circuit's number
        strip = lambda key: key[:2] if len(key) == 3 else key
        lag = trace["lagrange"]
        _trace.update(polys={strip(key): p for key, p in trace["polys"].items()}, commits={strip(key): p for key, p in trace["commits"].items()},
                      lagrange={key: cols[0] for key, cols in lag.items()},
                      pieces=trace["pieces"], challenges=trace["challenges"])
    return proof


def create_proof_multi(params, pk: ProvingKey, advice, instances, seed: int, _trace: dict = None, multiopen: str = "shplonk",
                       lookup: str = "halo2") -> bytes:
    """ONE proof for m circuits of ``pk``'s constraint system (upstream ``create_proof(params, pk, &[circuit; m], &[instances; m])``):
    ``advice`` is the (m, num_advice, n, 4) GPU tensor a witness writer returns, or a list of m (num_advice, n, 4) tensors;
    ``instances`` holds m entries, each in the form ``create_proof`` takes.  1 <= m <= 64.  All circuits share theta, beta, gamma, y
    and x; with m = 1 the bytes are ``create_proof``'s.  ``_trace``: as in ``create_proof``, the keys of what belongs to one circuit
    carrying its number as a third element (("advice", column, circuit) ...) and ``lagrange`` holding one entry per circuit.
    ``multiopen``, ``lookup``: as in ``create_proof``."""
    check_multiopen(multiopen, "create_proof_multi")
    check_lookup(lookup, "create_proof_multi")
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
    return _prove("create_proof_multi", params, pk, advice, list(instances), [seed], len(advice), "halo2", multiopen, _trace, lookup)[0]


def create_proofs(params, pk: ProvingKey, advice, instances, seeds, encoding: str = "halo2", multiopen: str = "shplonk",
                  lookup: str = "halo2") -> list:
    """m independent proofs of ``pk``'s constraint system in one batched pass: ``create_proofs(...)[b] == create_proof(params, pk,
    advice[b], instances[b], seeds[b])``, byte for byte.  ``advice``: the (m, num_advice, n, 4) GPU tensor a witness writer returns, or
    a list of m (num_advice, n, 4) tensors; ``instances``: m entries, each in the form ``create_proof`` takes; ``seeds``: m integers,
    pairwise distinct mod 2^48 (two proofs with one seed would share their blinding: ValueError), or ONE integer s standing for
    s, s + 1, ...  m >= 1, no upper limit.  ``encoding``, ``multiopen``, ``lookup``: as in ``create_proof`` (the keyword arguments of
    both calls being the same)."""
    who = "create_proofs"
    check_encoding(encoding, who)
    check_multiopen(multiopen, who)
    check_lookup(lookup, who)
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
    return _prove(who, params, pk, advice, list(instances), seeds, 1, encoding, multiopen, lookup=lookup)


def _prove(who, params, pk, advice, instances, seeds, m, encoding, multiopen, _trace: dict = None, lookup: str = "halo2") -> list:
    """The protocol (module docstring, steps 1 - 14) for T = len(seeds) transcripts of m circuits each -> the T proofs.  ``advice`` and
    ``instances`` hold one entry per unit u = t m + c, circuit c of transcript t; what belongs to a circuit is indexed by its unit, what
    belongs to a transcript (challenges, random polynomial, h) by t.  ``_trace`` is filled for T = 1 only."""
    import torch

    U, T = len(advice), len(seeds)
    assert U == T * m and (T == 1 or _trace is None)
    vk = pk.vk
    cs, dom = vk.cs, vk.domain
    k, n = dom.k, 1 << dom.k
    if params.k != k:
        raise ValueError(f"{who}: the parameters and the key differ in k")
    for a in advice:
        if not _is_tensor(a) or not a.is_cuda or tuple(a.shape) != (cs.num_advice, n, 4):
            raise ValueError(f"{who}: advice must be a ({cs.num_advice}, {n}, 4) GPU tensor" + ("" if U == 1 else " per circuit" if T == 1 else " per proof"))
    device = advice[0].device
    A, I = cs.num_advice, cs.num_instance
    blinding, deg = cs.blinding_factors, cs.degree()
    usable = n - blinding - 1
    omega, delta = dom.omega, FR_DELTA
    P, chunk, nsets, L = len(cs.equality), cs.permutation_chunk_len(), cs.permutation_sets(), len(cs.lookups)
    logup = lookup == "logup"
    groups = cs.logup_arguments() if logup else []        # "logup": the lookups are proved as these arguments, none on its own
    G = len(groups)
    if logup:
        L = 0
        if max([len(ins_list) for _, ins_list in groups] or [0]) * usable >= 1 << 32:
            raise ValueError(f"{who}: a logUp argument needs inputs x usable rows below 2^32")
    counts = (cs.num_fixed, A, I)
    units, every = range(U), range(T)
    at = [(u // m, u % m) for u in units]                                    # unit -> (transcript, circuit inside it)
    # the seeds of the blinding: advice, permuted columns, z columns, random polynomial; the circuit's number above the 58 bits of the base
    bases = [((int(seeds[t]) & 0xFFFFFFFFFFFF) << 10) | (c << 58) for t, c in at]
    d = lambda values: _dev(values, device)
    commits = {}
    progs = _Programs(one_transcript=T == 1)

    def commit(items, handle):
        """``items``: (transcript, key, column) triples.  One best_multiexp_batch over all of them; every transcript then absorbs its own
        points, in the order listed"""
        com = best_multiexp_batch([col for _, _, col in items], handle) if items else []
        for (t, key, _), c in zip(items, com):
            point = g1_words_to_int(c)
            transcripts[t].write_point(point)
            if _trace is not None:
                commits[key] = point

    commit_lagrange = lambda items: commit(items, params.g_lagrange_handle)
    commit_coeff = lambda items: commit(items, params.g_handle)

    # ---- the columns (steps 1 - 3) -------------------------------------------------------------------------------------------------------------
    adv = torch.stack(list(advice), dim=1)                                   # (A, U, n, 4), a copy: adv[i] is column i of every unit
    for u in units:
        adv[:, u, usable:] = random_fr(A * (n - usable), bases[u], device, shape=(A, n - usable, 4))
    for i in cs.unblinded_advice:                                            # the draw above is the same with or without them
        adv[i, :, usable:] = 0
    inst_cols = [instance_values(cs, instance) for instance in instances]
    inst = torch.zeros((I, U, n, 4), dtype=torch.int64, device=device)
    for u in units:
        for i, values in enumerate(inst_cols[u]):
            if len(values) > usable:
                raise ValueError(f"{who}: too many instance values")
            if values:
                inst[i, u, :len(values)] = d(values)
    fixed = pk.fixed_values
    table = [fixed[i] for i in range(cs.num_fixed)] + [adv[i] for i in range(A)] + [inst[i] for i in range(I)]

    digest = vk_digest(vk)
    transcripts = [WRITERS[encoding]() for _ in every]
    squeeze = lambda: [tr.squeeze_challenge() for tr in transcripts]
    for t, tr in enumerate(transcripts):
        tr.common_scalar(digest)
        for u in range(t * m, (t + 1) * m):
            for values in inst_cols[u]:
                for v in values:
                    tr.common_scalar(v)
    commit_lagrange([(t, ("advice", i, c), adv[i, u]) for u, (t, c) in enumerate(at) for i in range(A)])
    theta = squeeze()                                                         # step 4

    try:
        # ---- the lookups: permuted columns (step 5; lookup j of unit u at index u L + j) -------------------------------------------------------
        thetas = [dict(theta=theta[t]) for t, _ in at]
        lookups = [] if logup else cs.lookups
        lk_in = [progs.run_proofs(("in", j), [_compress(ins)], counts, table, n, thetas) for j, (ins, _) in enumerate(lookups)]
        lk_tab = [progs.run_proofs(("tab", j), [_compress(tabs)], counts, table, n, thetas) for j, (_, tabs) in enumerate(lookups)]
        order = [(u, j) for u in units for j in range(L)]
        try:
            permuted = permute_expression_pairs([lk_in[j][u] for u, j in order], [lk_tab[j][u] for u, j in order], usable,
                                                blinding_seeds=[bases[u] + 0x40 + 2 * j for u, j in order]) if L else []
        except _lib.Halo2Mi355xError as e:
            if T == 1:
                raise
            where = [order[i] for i in getattr(e, "missing", [])]             # several proofs: the same error, naming the proof (u = t)
            err = _lib.Halo2Mi355xError(e.code, f"{e} -- " + ", ".join(f"proof {b} (lookup {j})" for b, j in where))
            err.missing, err.proofs = [j for _, j in where], sorted({b for b, _ in where})
            raise err from None
        commit_lagrange([item for (u, j), (a, s) in zip(order, permuted)
                         for item in ((at[u][0], ("lookup_a", j, at[u][1]), a), (at[u][0], ("lookup_s", j, at[u][1]), s))])
        # ---- "logup": the multiplicity columns in their place (argument g of unit u at index u G + g) -----------------------------------
        lu_tab = [progs.run_proofs(("lu_tab", g), [_compress(tabs)], counts, table, n, thetas) for g, (tabs, _) in enumerate(groups)]
        lu_in = [[progs.run_proofs(("lu_in", g, j), [_compress(ins)], counts, table, n, thetas) for j, ins in enumerate(ins_list)]
                 for g, (_, ins_list) in enumerate(groups)]
        lu_order = [(u, g) for u in units for g in range(G)]
        try:
            lu_m = logup_multiplicities([lu_tab[g][u] for u, g in lu_order], [[f[u] for f in lu_in[g]] for u, g in lu_order], usable) if G else []
        except _lib.Halo2Mi355xError as e:
            if T == 1:
                raise
            where = [lu_order[i] for i in getattr(e, "missing", [])]          # several proofs: the same error, naming the proof (u = t)
            err = _lib.Halo2Mi355xError(e.code, f"{e} -- " + ", ".join(f"proof {b} (argument {g})" for b, g in where))
            err.missing, err.proofs = [g for _, g in where], sorted({b for b, _ in where})
            raise err from None
        for (u, g), col in zip(lu_order, lu_m):
            col[usable:] = random_fr(n - usable, bases[u] + 0x40 + 2 * g, device)
        commit_lagrange([(at[u][0], ("logup_m", g, at[u][1]), col) for (u, g), col in zip(lu_order, lu_m)])
        beta, gamma = squeeze(), squeeze()                                    # step 6
        bg = [dict(beta=beta[t], gamma=gamma[t]) for t, _ in at]

        # ---- the permutation argument (step 7): one z per chunk of columns, chained at the last usable row inside its circuit ----------------
        by_kind = {"advice": lambda i: adv[i], "fixed": lambda i: fixed[i], "instance": lambda i: inst[i]}
        perm_cols = [by_kind[kind](i) for kind, i in cs.equality]
        sigma = pk.permutation_values
        acc, xs = 1, []
        for _ in range(n):
            xs.append(acc)
            acc = acc * omega % R
        x_col = d(xs)
        mul2 = [ev.Advice(0) * ev.Advice(1)]
        factors = []                                                        # per set: (U, n, 4)
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
            batch_invert(den.reshape(U * n, 4))
            factors.append(progs.run_proofs("mul2", mul2, (0, 2, 0), [num, den], n, [{} for _ in units]))
        # the chain of grand_product_batch runs from one set to the next and must start at 1 in every circuit: one call per unit
        zs = [grand_product_batch([f[u] for f in factors], fr_words(1), chain_row=usable) if factors else [] for u in units]
        for u in units:
            for i, z in enumerate(zs[u]):
                z[usable + 1:] = random_fr(n - usable - 1, bases[u] + 0x80 + i, device)
        commit_lagrange([(t, ("perm_z", i, c), z) for u, (t, c) in enumerate(at) for i, z in enumerate(zs[u])])

        # ---- the lookup arguments' z (step 8): the lookups of all units as the units of one launch ---------------------------------------------
        pair = [(ev.Advice(0) + ev.BETA) * (ev.Advice(1) + ev.GAMMA)]
        lk_z = [[] for _ in units]
        if L:
            stacked = lambda ts: torch.stack(list(ts))                    # (U L, n, 4)
            bg_l = [bg[u] for u, _ in order]
            num = progs.run_proofs("pair", pair, (0, 2, 0), [stacked(lk_in[j][u] for u, j in order), stacked(lk_tab[j][u] for u, j in order)], n, bg_l)
            den = progs.run_proofs("pair", pair, (0, 2, 0), [stacked(a for a, _ in permuted), stacked(s for _, s in permuted)], n, bg_l)
            batch_invert(den.reshape(U * L * n, 4))
            lk_factors = progs.run_proofs("mul2", mul2, (0, 2, 0), [num, den], n, [{} for _ in order])
            flat = grand_product_batch([lk_factors[i] for i in range(U * L)], fr_words(1))
            for (u, j), z in zip(order, flat):
                z[usable + 1:] = random_fr(n - usable - 1, bases[u] + 0xC0 + j, device)
                lk_z[u].append(z)
        commit_lagrange([(t, ("lookup_z", j, c), z) for u, (t, c) in enumerate(at) for j, z in enumerate(lk_z[u])])
        # ---- "logup": the running sums in their place.  The denominators t + beta, f_j + beta of all arguments and units are the units
        # of ONE launch and ONE batch_invert; the terms sum_j 1 / (f_j + beta) - m / (t + beta) one launch per number of inputs --------------
        lu_phi = [[] for _ in units]
        if G:
            dens, bg_d, slot = [], [], {}
            for u, g in lu_order:
                for key, col in [(("t", u, g), lu_tab[g][u])] + [(("f", u, g, j), f[u]) for j, f in enumerate(lu_in[g])]:
                    slot[key] = len(dens)
                    dens.append(col)
                    bg_d.append(bg[u])
            inv = progs.run_proofs("lu_den", [ev.Advice(0) + ev.BETA], (0, 1, 0), [torch.stack(dens)], n, bg_d)
            batch_invert(inv.reshape(len(dens) * n, 4))
            terms = {}
            for c in sorted({len(f) for f in lu_in}):
                mine = [(u, g) for u, g in lu_order if len(lu_in[g]) == c]
                e = ev.Advice(0)
                for j in range(1, c):
                    e = e + ev.Advice(j)
                cols = [torch.stack([inv[slot[("f", u, g, j)]] for u, g in mine]) for j in range(c)]
                cols += [torch.stack([lu_m[u * G + g] for u, g in mine]), torch.stack([inv[slot[("t", u, g)]] for u, g in mine])]
                out = progs.run_proofs(("lu_term", c), [e - ev.Advice(c) * ev.Advice(c + 1)], (0, c + 2, 0), cols, n, [{} for _ in mine])
                terms.update({ug: out[i] for i, ug in enumerate(mine)})
            for (u, g), phi in zip(lu_order, grand_sum_batch([terms[ug] for ug in lu_order])):
                phi[usable + 1:] = random_fr(n - usable - 1, bases[u] + 0xC0 + g, device)
                lu_phi[u].append(phi)
        commit_lagrange([(t, ("logup_phi", g, c), phi) for u, (t, c) in enumerate(at) for g, phi in enumerate(lu_phi[u])])
    finally:
        progs.destroy()
    perm_of = [[permuted[u * L + j] for j in range(L)] for u in units]
    lu_m_of = [[lu_m[u * G + g] for g in range(G)] for u in units]
    NL = 2 * G if logup else 3 * L                                           # the lookup columns of its own that a circuit brings to h

    # ---- the vanishing argument's random polynomial (step 9: one per transcript), y (step 10), then h ------------------------------------------
    random_polys = [random_fr(n, bases[t * m] + 0x100, device) for t in every]
    commit_coeff([(t, ("random",), random_polys[t]) for t in every])
    y = squeeze()

    g, tab = circuits.evaluate_h_program(cs, k, dom.extended_k, delta, divide=False, lookup=lookup)
    V = nsets + NL + A + I                                               # the columns of its own that a circuit brings to h
    lagrange = [col for u in units
                for col in zs[u] + [t for j in range(L) for t in (lk_z[u][j], perm_of[u][j][0], perm_of[u][j][1])]
                + [t for g_ in range(G) for t in (lu_phi[u][g_], lu_m_of[u][g_])] + [adv[i, u] for i in range(A)]
                + [inst[i, u] for i in range(I)]]
    var_coeffs = dom.lagrange_to_coeff(torch.stack(lagrange)).reshape(U, V, n, 4)
    z_polys, lk_polys = var_coeffs[:, :nsets], var_coeffs[:, nsets:nsets + NL]
    adv_polys = var_coeffs[:, nsets + NL:nsets + NL + A]
    sel = dom.lagrange_to_coeff(torch.stack([pk.l0, pk.l_last, pk.l_active]))
    x_poly = d([0, 1] + [0] * (n - 2)).reshape(1, n, 4)
    shared = dom.coeff_to_extended(torch.cat([pk.fixed_polys, pk.permutation_polys, sel, x_poly]))
    n_shared = shared.shape[0]
    assert n_shared + nsets + NL == tab.t_inv
    rot_scale = 1 << (dom.extended_k - k)
    en = dom.extended_len()
    unread = torch.zeros((max(rot_scale, 2), 4), dtype=torch.int64, device=device)[:rot_scale]     # the table's t_inv entry: divide=False never reads it
    prog = g.compile(tab.num_fixed_entries, A, I, rot_scale=rot_scale, short_columns=tab.short_columns)
    h_ext = torch.zeros((T, en, 4), dtype=torch.int64, device=device)
    n_fs = cs.num_fixed + P
    step = max(1, H_COLUMN_BUDGET // max(V * en * 32, 1))                   # units whose extended columns are in flight together
    stride = V * en * 8
    # the one place where the shape chooses the device call: transcripts of one circuit are the proofs of evaluate_proofs, a chunk of
    # them per call; the circuits of a transcript go through evaluate_circuits, chunk after chunk chained through PreviousValue
    chunks = [(u0, min(step, U - u0)) for u0 in range(0, U, step)] if m == 1 else \
             [(t * m + c0, min(step, m - c0)) for t in every for c0 in range(0, m, step)]
    try:
        for u0, nu in chunks:
            ext = dom.coeff_to_extended(var_coeffs[u0:u0 + nu].reshape(nu * V, n, 4)).reshape(nu, V, en, 4)
            own = lambda v: (ext[0, v], stride)
            share = lambda i: (shared[i], 0)
            # the program's table: fixed, sigma | z | l0, l_last, l_active, x | lookups | t_inv || advice | instance
            cols = ([share(i) for i in range(n_fs)] + [own(i) for i in range(nsets)] + [share(i) for i in range(n_fs, n_shared)]
                    + [own(nsets + i) for i in range(NL)] + [(unread, 0)] + [own(nsets + NL + i) for i in range(A + I)])
            if m == 1:
                prog.evaluate_proofs(cols, h_ext[u0:u0 + nu], [dict(beta=beta[t], gamma=gamma[t], theta=theta[t], y=y[t]) for t in range(u0, u0 + nu)])
            else:
                t = u0 // m
                prog.evaluate_circuits([c for c, _ in cols], [s for _, s in cols], h_ext[t], nu, beta=beta[t], gamma=gamma[t], theta=theta[t], y=y[t])
            del ext
    finally:
        prog.destroy()
    dom.divide_by_vanishing_poly(h_ext)
    h_coeff = dom.extended_to_coeff(h_ext)                      # (T, (deg - 1) n, 4): in place on h_ext
    pieces = [[h_coeff[t, i * n:(i + 1) * n] for i in range(deg - 1)] for t in every]
    commit_coeff([(t, ("h_piece", i), p) for t in every for i, p in enumerate(pieces[t])])      # step 11
    x = squeeze()                                                             # step 12

    # ---- the evaluations (step 13): one eval_polynomial over all transcripts ------------------------------------------------------------------
    adv_q, fix_q, _ = cs.queries()
    last = -(blinding + 1)
    circuits_ = range(m)
    h_polys = linear_combination_batch(pieces, [[pow(x[t], n * i, R) for i in range(deg - 1)] for t in every])
    # what is evaluated and what is opened, as (key, rotation): the same in every transcript, each list written once
    wanted = [(("advice", i, c), r) for c in circuits_ for i, r in adv_q]
    wanted += [(("fixed", i), r) for i, r in fix_q] + [(("random",), 0)]
    wanted += [(("sigma", j), 0) for j in range(P)]
    for c in circuits_:
        for i in range(nsets):
            wanted += [(("perm_z", i, c), 0), (("perm_z", i, c), 1)] + ([(("perm_z", i, c), last)] if i + 1 < nsets else [])
    for c in circuits_:
        for j in range(L):
            wanted += [(("lookup_z", j, c), 0), (("lookup_z", j, c), 1), (("lookup_a", j, c), 0), (("lookup_a", j, c), -1), (("lookup_s", j, c), 0)]
        for g_ in range(G):
            wanted += [(("logup_phi", g_, c), 0), (("logup_phi", g_, c), 1), (("logup_m", g_, c), 0)]
    wanted.append((("h",), 0))                                                # h(x): evaluated with the rest and not written
    queries = []                                                              # the multiopen's (step 14), upstream's order
    for c in circuits_:
        queries += [(("advice", i, c), r) for i, r in adv_q]
        queries += [qq for i in range(nsets) for qq in ((("perm_z", i, c), 0), (("perm_z", i, c), 1))]
        queries += [(("perm_z", i, c), last) for i in reversed(range(nsets - 1))]
        for j in range(L):
            queries += [(("lookup_z", j, c), 0), (("lookup_a", j, c), 0), (("lookup_s", j, c), 0), (("lookup_a", j, c), -1), (("lookup_z", j, c), 1)]
        for g_ in range(G):
            queries += [(("logup_phi", g_, c), 0), (("logup_m", g_, c), 0), (("logup_phi", g_, c), 1)]
    queries += [(("fixed", i), r) for i, r in fix_q] + [(("sigma", j), 0) for j in range(P)]
    queries += [(("h",), 0), (("random",), 0)]
    omega_to = {r: pow(omega, r, R) for r in {r for _, r in wanted}}
    points_of = [{r: x[t] * w % R for r, w in omega_to.items()} for t in every]      # transcript t's x omega^r
    common = {}
    for i in range(cs.num_fixed):
        common[("fixed", i)] = pk.fixed_polys[i]
    for j in range(P):
        common[("sigma", j)] = pk.permutation_polys[j]
    polys_of, slots, index = [], [], {}
    for t in every:
        polys = {("random",): random_polys[t]}
        for c in circuits_:
            for i in range(A):
                polys[("advice", i, c)] = adv_polys[t * m + c, i]
        polys.update(common)
        for c in circuits_:
            for i in range(nsets):
                polys[("perm_z", i, c)] = z_polys[t * m + c, i]
        for c in circuits_:
            for j in range(L):
                polys[("lookup_z", j, c)], polys[("lookup_a", j, c)], polys[("lookup_s", j, c)] = lk_polys[t * m + c, 3 * j:3 * j + 3]
            for g_ in range(G):
                polys[("logup_phi", g_, c)], polys[("logup_m", g_, c)] = lk_polys[t * m + c, 2 * g_:2 * g_ + 2]
        polys[("h",)] = h_polys[t]
        polys_of.append(polys)
        for key, poly in polys.items():                                       # a slot per polynomial, the shared ones once
            slot = key if key in common else (key, t)
            if slot not in index:
                index[slot] = len(slots)
                slots.append(poly)
    vals = words_to_ints(eval_polynomial(torch.stack(slots), np.stack([fr_words(points_of[t][r]) for t in every for _, r in wanted]),
                                         poly_index=np.array([index[key if key in common else (key, t)] for t in every for key, _ in wanted],
                                                             dtype=np.uint32)))
    queries_of = []
    for t in every:
        mine = vals[t * len(wanted):(t + 1) * len(wanted)]
        for v in mine[:-1]:
            transcripts[t].write_scalar(v)
        evals = dict(zip(wanted, mine))
        queries_of.append([(key, points_of[t][r], evals[(key, r)]) for key, r in queries])

    # ---- the multiopen (step 14) -----------------------------------------------------------------------------------------------------------
    scheme = gwc if multiopen == "gwc" else shplonk
    if T == 1:
        scheme.create_opening(params, transcripts[0], queries_of[0], polys_of[0])
    else:
        scheme.create_openings(params, transcripts, queries_of, polys_of)
    if _trace is not None:
        _trace.update(polys=polys_of[0], commits=commits,
                      lagrange={"advice": [adv[:, u] for u in units], "perm_z": zs, "lookup_z": lk_z, "permuted": perm_of, "logup_m": lu_m_of,
                                "logup_phi": lu_phi},
                      pieces=pieces[0], challenges=dict(theta=theta[0], beta=beta[0], gamma=gamma[0], y=y[0], x=x[0]))
    return [tr.finalize() for tr in transcripts]
