#!/usr/bin/env python3
"""create_proof / verify_proof end to end and the SHPLONK multiopen alone, on one MI355X.

(a) MerkleSumTree depth 5 / k = 9 (the reference's test_full_prover) and depth 20 / k = 10: ParamsKZG.setup, keygen, a GPU witness,
    then create_proof and verify_proof (pairing route) wall-clock, with the time inside shplonk.create_opening split out.
(b) the multiopen of the k = 18 MerkleSumTree shape (the rotation sets of that constraint system, random polynomials): the route of
    hm_shplonk_set_quotient_bn256_fr_dev -- one call per rotation set into h, one for the final quotient -- against the same two
    polynomials composed from the kernels that existed before it: linear_combination, eval_polynomial, host interpolation, one
    kate_division per point.  The results are compared word for word; the commitments are left out of both.
(c) ``--circuits m``: instead of (a) and (b), m users' MerkleSumTree witnesses at depth 20 / k = 10 and depth 5 / k = 9 (DESIGN.md section
    19): create_proof_multi against m separate create_proof calls in the same run, and the h step alone -- the undivided numerator over
    the extended domain through CompiledGraph.evaluate_circuits against the loop of m evaluate calls on the same columns (equal word for
    word).
(d) ``--proofs m[,m...]``: instead, m users' witnesses at depth 20 / k = 10 and depth 5 / k = 9: create_proofs -- m
    independent proofs in one batched pass -- against the loop of m create_proof calls in the same run (the bytes are compared), and two
    of its steps alone, each against its loop: the h numerator through CompiledGraph.evaluate_proofs against m evaluate calls with
    per-proof constants on the same columns, and the multiopen (shplonk.create_openings inside create_proofs against the m
    create_opening calls inside the loop, both timed in a second pass of their own; at m = 1 create_proofs too ends in create_opening).
(e) ``--multiopen shplonk|gwc|both`` (with ``--proofs m[,m...]``, default 1,16,64): instead, the two multiopen schemes side by side
     at depth 5 / k = 9 and depth 20 / k = 10: create_proof (m = 1) or create_proofs (m > 1) wall-clock with
    ``multiopen=`` each scheme, the routes alternating inside every repeat of one session, and in a second pass the multiopen alone
    (``create_opening`` / ``create_openings`` of ``shplonk`` and of ``gwc``, commitments included); and the polynomial side at the
    k = 18 shape: the q one-point quotients of GWC beside SHPLONK's set quotients, commitments left out of both.
(f) ``--lookup halo2|logup|both`` (with ``--proofs m[,m...]``, default 1,16,64): instead, the two lookup arguments side by side
     at depth 5 / k = 9 and depth 20 / k = 10: create_proof (m = 1) or create_proofs (m > 1) wall-clock with
    ``lookup=`` each argument on the same witnesses and seeds, the arguments alternating inside every repeat of one session; the
    commitments, evaluations and bytes of a proof under each, counted from the constraint system; and the two new kernels alone
    (events around the call) at the k = 10 and k = 17 shapes -- eight byte columns into a 256-entry table --, the multiplicities of
    the three arguments beside ``hm_lookup_permute_batch_bn256_fr_dev`` on the same eight columns, the running sums beside
    ``grand_product_batch`` on as many columns: these are what they replace.
Five repeats each: median and min .. max.  Prints one JSON object."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import halo2_experiments_amd as h                                         # noqa: E402
from halo2_experiments_amd import circuits, gwc, poseidon as ps, shplonk as sh   # noqa: E402
from halo2_experiments_amd.domain import FR_MODULUS as R, EvaluationDomain, fr_words   # noqa: E402
from halo2_experiments_amd.kzg import ParamsKZG                            # noqa: E402
import prover_cases as pc                                                  # noqa: E402
import prover_multi_cases as pmc                                           # noqa: E402

REPEATS = 5


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def end_to_end(name):
    cs, lay, advice, instance, _ = pc.build(name)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    inner = []
    real = sh.create_opening

    def timed(*a, **kw):
        _, ms = wall(lambda: real(*a, **kw))
        inner.append(ms)
    sh.create_opening = timed
    try:
        h.create_proof(params, pk, advice, instance, 1)                    # warm-up: program compiles, allocator pools
        inner.clear()
        prove, verify = [], []
        for rep in range(REPEATS):
            proof, ms = wall(lambda: h.create_proof(params, pk, advice, instance, 2 + rep))
            prove.append(ms)
            ok, ms = wall(lambda: h.verify_proof(params, vk, instance, proof))
            assert ok
            verify.append(ms)
    finally:
        sh.create_opening = real
        params.release()
    return {"k": lay.k, "proof_bytes": len(proof), "create_proof": spread(prove), "of_which_shplonk": spread(inner), "verify_proof": spread(verify)}


def h_step(cs, dom, m):
    """the numerator of h for m circuits on random extended columns, laid out as create_proof_multi lays them out: what a circuit owns
    stacked per circuit, the rest shared"""
    from halo2_experiments_amd.keygen import FR_DELTA
    g, lay = circuits.evaluate_h_program(cs, dom.k, dom.extended_k, FR_DELTA, divide=False)
    en, scale = dom.extended_len(), 1 << (dom.extended_k - dom.k)
    n_cols = lay.num_fixed_entries + cs.num_advice + cs.num_instance
    nsets, L = cs.permutation_sets(), len(cs.lookups)
    own = set(range(lay.z0, lay.z0 + nsets)) | set(range(lay.lookup0, lay.lookup0 + 3 * L)) | set(range(lay.num_fixed_entries, n_cols))
    cols = [h.random_fr(m * en, 50 + i, shape=(m, en, 4)) if i in own else h.random_fr(scale if i == lay.t_inv else en, 50 + i) for i in range(n_cols)]
    prev = h.random_fr(en, 49)
    scalars = dict(beta=3, gamma=5, theta=7, y=11)
    prog = g.compile(lay.num_fixed_entries, cs.num_advice, cs.num_instance, rot_scale=scale, short_columns=lay.short_columns)
    per_circuit = [[col[c] if i in own else col for i, col in enumerate(cols)] for c in range(m)]

    def loop():
        values = prev.clone()
        for c in range(m):
            prog.evaluate(per_circuit[c], values, **scalars)
        return values

    def entry():
        values = prev.clone()
        prog.evaluate_circuits(cols, None, values, m, **scalars)
        return values
    try:
        assert torch.equal(loop(), entry()), "the entry and the loop differ"
        one, many = [], []
        for _ in range(REPEATS):
            many.append(wall(loop)[1])
            one.append(wall(entry)[1])
    finally:
        prog.destroy()
    return {"rows": en, "lanes": m * en, "program_calculations": int(prog.calcs.shape[0]), "evaluate_circuits": spread(one),
            "loop_of_evaluate": spread(many)}


def multi(name, m):
    cs, lay, advice, instances = pmc.build_multi(name, m)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    try:
        h.create_proof_multi(params, pk, advice, instances, 1)                 # warm-up
        h.create_proof(params, pk, advice[0], instances[0], 1)
        one, separate, verify = [], [], []
        for rep in range(REPEATS):
            proof, ms = wall(lambda: h.create_proof_multi(params, pk, advice, instances, 2 + rep))
            one.append(ms)
            _, ms = wall(lambda: [h.create_proof(params, pk, advice[c], instances[c], 2 + rep) for c in range(m)])
            separate.append(ms)
        for rep in range(2):
            ok, ms = wall(lambda: h.verify_proof_multi(params, vk, instances, proof))
            assert ok
            verify.append(ms)
        out = {"k": lay.k, "circuits": m, "proof_bytes": len(proof), "create_proof_multi": spread(one),
               "separate_create_proof_calls": spread(separate), "verify_proof_multi": spread(verify), "h_step": h_step(cs, vk.domain, m)}
    finally:
        params.release()
    return out


def h_step_proofs(cs, dom, m):
    """the numerator of h for m independent proofs on random extended columns, laid out as create_proofs lays them out (what a proof
    owns stacked per proof, the rest shared at stride 0), every proof with its own beta, gamma, theta, y"""
    from halo2_experiments_amd.keygen import FR_DELTA
    g, lay = circuits.evaluate_h_program(cs, dom.k, dom.extended_k, FR_DELTA, divide=False)
    en, scale = dom.extended_len(), 1 << (dom.extended_k - dom.k)
    n_cols = lay.num_fixed_entries + cs.num_advice + cs.num_instance
    nsets, L = cs.permutation_sets(), len(cs.lookups)
    own = set(range(lay.z0, lay.z0 + nsets)) | set(range(lay.lookup0, lay.lookup0 + 3 * L)) | set(range(lay.num_fixed_entries, n_cols))
    cols = [h.random_fr(m * en, 50 + i, shape=(m, en, 4)) if i in own else h.random_fr(scale if i == lay.t_inv else en, 50 + i) for i in range(n_cols)]
    rng = random.Random(m)
    scalars = [dict(beta=rng.randrange(R), gamma=rng.randrange(R), theta=rng.randrange(R), y=rng.randrange(R)) for _ in range(m)]
    prog = g.compile(lay.num_fixed_entries, cs.num_advice, cs.num_instance, rot_scale=scale, short_columns=lay.short_columns)
    per_proof = [[col[b] if i in own else col for i, col in enumerate(cols)] for b in range(m)]
    zeros = lambda: torch.zeros((m, en, 4), dtype=torch.int64, device="cuda")

    def loop():
        values = zeros()
        for b in range(m):
            prog.evaluate(per_proof[b], values[b], **scalars[b])
        return values

    def entry():
        values = zeros()
        prog.evaluate_proofs(cols, values, scalars)
        return values
    try:
        assert torch.equal(loop(), entry()), "the entry and the loop differ"
        one, many = [], []
        for _ in range(REPEATS):
            many.append(wall(loop)[1])
            one.append(wall(entry)[1])
    finally:
        prog.destroy()
    return {"rows": en, "lanes": m * en, "program_calculations": int(prog.calcs.shape[0]), "evaluate_proofs": spread(one),
            "loop_of_evaluate": spread(many)}


def proofs(name, m):
    cs, lay, advice, instances = pmc.build_multi(name, m)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    seeds = lambda rep: [1000 * rep + b for b in range(m)]
    batched = lambda rep: h.create_proofs(params, pk, advice, instances, seeds(rep))
    looped = lambda rep: [h.create_proof(params, pk, advice[b], instances[b], seeds(rep)[b]) for b in range(m)]
    inner = []
    real_one, real_many = sh.create_opening, sh.create_openings

    def timed(real):
        def run(*a, **kw):
            inner.append(wall(lambda: real(*a, **kw))[1])
        return run
    try:
        assert batched(1) == looped(1), "create_proofs and the loop of create_proof differ"      # and the warm-up of both
        one, separate = [], []
        for rep in range(REPEATS):
            out, ms = wall(lambda: batched(2 + rep))
            one.append(ms)
            _, ms = wall(lambda: looped(2 + rep))
            separate.append(ms)
        ok, verify_ms = wall(lambda: h.verify_proofs(params, vk, instances, out))
        assert ok
        # the multiopen alone, in a pass of its own: the synchronisation around it would count against the totals above
        sh.create_opening, sh.create_openings = timed(real_one), timed(real_many)
        open_batched, open_looped = [], []
        for rep in range(REPEATS):
            inner.clear()
            batched(2 + rep)
            open_batched.append(sum(inner))
            inner.clear()
            looped(2 + rep)
            open_looped.append(sum(inner))
        res = {"k": lay.k, "proofs": m, "proof_bytes": len(out[0]), "create_proofs": spread(one), "loop_of_create_proof": spread(separate),
               "per_proof_ms": {"create_proofs": round(statistics.median(one) / m, 3), "loop": round(statistics.median(separate) / m, 3)},
               "verify_proofs_once_ms": round(verify_ms, 3),
               "multiopen": {"create_openings": spread(open_batched), "loop_of_create_opening": spread(open_looped)},
               "h_step": h_step_proofs(cs, vk.domain, m)}
    finally:
        sh.create_opening, sh.create_openings = real_one, real_many
        params.release()
    return res


def k18_queries():
    """the queries of the MerkleSumTree constraint system at k = 18 in the prover's order, every evaluation 0"""
    cs = circuits.merkle_sum_tree(ps.default_spec(5))
    dom = EvaluationDomain(cs.degree(), 18)
    x = 0x123456789ABCDEF % R
    rot = lambda r: x * pow(dom.omega, r, R) % R
    adv_q, fix_q, _ = cs.queries()
    nsets, L, P, last = cs.permutation_sets(), len(cs.lookups), len(cs.equality), -(cs.blinding_factors + 1)
    q = [(("advice", c), rot(r), 0) for c, r in adv_q]
    q += [qq for i in range(nsets) for qq in ((("perm_z", i), x, 0), (("perm_z", i), rot(1), 0))]
    q += [(("perm_z", i), rot(last), 0) for i in reversed(range(nsets - 1))]
    for j in range(L):
        q += [(("lookup_z", j), x, 0), (("lookup_a", j), x, 0), (("lookup_s", j), x, 0), (("lookup_a", j), rot(-1), 0), (("lookup_z", j), rot(1), 0)]
    q += [(("fixed", c), rot(r), 0) for c, r in fix_q] + [(("sigma", j), x, 0) for j in range(P)] + [(("h",), x, 0), (("random",), x, 0)]
    return q


def k18_sets():
    """the rotation sets of the MerkleSumTree constraint system as (points, keys), with the prover's order of queries"""
    sets, super_points = sh.construct_intermediate_sets(k18_queries())
    return [(pts, [key for key, _ in members]) for pts, members in sets], super_points


def multiopen_k18():
    n = 1 << 18
    sets, super_points = k18_sets()
    keys = [key for _, members in sets for key in members]
    polys = {key: h.random_fr(n, 100 + i) for i, key in enumerate(keys)}
    rng = random.Random(18)
    y, v, u = (rng.randrange(2, R) for _ in range(3))
    zt = sh.vanishing_eval(super_points, u)
    z = [sh.vanishing_eval([p for p in super_points if p not in pts], u) for pts, _ in sets]
    w = lambda values: np.stack([fr_words(c % R) for c in values])
    zeros = lambda rows: torch.zeros((rows, 4), dtype=torch.int64, device="cuda")

    def final_terms(hx):
        cols, weights = [], []
        for i, (pts, members) in enumerate(sets):
            for j, key in enumerate(members):
                cols.append(polys[key])
                weights.append(pow(v, i, R) * z[i] % R * pow(y, j, R) % R)
        return cols + [hx], weights + [-zt % R]

    def new_route():
        hx = None
        for i, (pts, members) in enumerate(sets):
            hx = sh.set_quotient([polys[k] for k in members], [pow(y, j, R) for j in range(len(members))], pts, pow(v, i, R), out=hx, accumulate=i > 0)
        cols, weights = final_terms(hx)
        return hx, sh.set_quotient(cols, weights, [u], pow(z[0], -1, R))

    def composed_route():
        hx = zeros(n)
        for i, (pts, members) in enumerate(sets):
            t = len(pts)
            num = h.linear_combination([polys[k] for k in members], w([pow(y, j, R) for j in range(len(members))]))
            evals = ps.words_to_ints(h.eval_polynomial(num.reshape(1, n, 4), w(pts), poly_index=np.zeros(t, dtype=np.uint32)))
            r = zeros(n)
            r[:t] = torch.from_numpy(ps.ints_to_words(sh.lagrange_interpolate_ints(pts, evals)).view(np.int64)).cuda()
            qx = h.linear_combination([num, r], w([1, R - 1]))
            for p in pts:
                qx = h.kate_division(qx, fr_words(p))
            h.linear_combination([hx, torch.cat([qx, zeros(t)])], w([1, pow(v, i, R)]), out=hx)
        cols, weights = final_terms(hx)
        lx = h.linear_combination(cols, w(weights))
        fin = h.linear_combination([h.kate_division(lx, fr_words(u))], w([pow(z[0], -1, R)]))
        return hx, torch.cat([fin, zeros(1)])

    a, b = new_route(), composed_route()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two routes differ"
    new, old = [], []
    for _ in range(REPEATS):
        new.append(wall(new_route)[1])
        old.append(wall(composed_route)[1])
    return {"n": n, "sets": [{"points": len(pts), "polynomials": len(members)} for pts, members in sets],
            "set_quotient_entry": spread(new), "composed_from_existing_kernels": spread(old)}


def schemes(name, m, multiopens):
    """(e): m proofs of one shape under every scheme of ``multiopens`` -- totals with the routes alternating, then the multiopen alone"""
    cs, lay, advice, instances = pmc.build_multi(name, m)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)
    entry = "create_opening" if m == 1 else "create_openings"
    where = {"shplonk": sh, "gwc": gwc}                       # the module whose attribute the prover calls for the scheme
    real = {mo: getattr(where[mo], entry) for mo in multiopens}
    inner = []

    def run(mo, rep):
        if m == 1:
            return [h.create_proof(params, pk, advice[0], instances[0], 1000 * rep, multiopen=mo)]
        return h.create_proofs(params, pk, advice, instances, [1000 * rep + b for b in range(m)], multiopen=mo)

    def timed(fn):
        def call(*a, **kw):
            inner.append(wall(lambda: fn(*a, **kw))[1])
        return call
    try:
        sizes = {}
        for mo in multiopens:                                     # warm-up, and the proofs verify
            made = run(mo, 1)
            assert h.verify_proofs(params, vk, instances[:m], made, transcript="device", pairing="device", multiopen=mo)
            sizes[mo] = len(made[0])
        totals, opens = {mo: [] for mo in multiopens}, {mo: [] for mo in multiopens}
        for rep in range(REPEATS):
            for mo in multiopens:
                totals[mo].append(wall(lambda: run(mo, 2 + rep))[1])
        for mo in multiopens:
            setattr(where[mo], entry, timed(real[mo]))
        for rep in range(REPEATS):
            for mo in multiopens:
                inner.clear()
                run(mo, 2 + rep)
                opens[mo].append(sum(inner))
    finally:
        for mo in multiopens:
            setattr(where[mo], entry, real[mo])
        params.release()
    return {"k": lay.k, "proofs": m, "entry": "create_proof" if m == 1 else "create_proofs",
            **{mo: {"proof_bytes": sizes[mo], "total": spread(totals[mo]), "multiopen": spread(opens[mo]),
                    "per_proof_ms": round(statistics.median(totals[mo]) / m, 3)} for mo in multiopens}}


def multiopen_k18_schemes(multiopens):
    """the polynomial side at k = 18, commitments left out: SHPLONK's set quotients (h, then the final quotient) beside GWC's q one-point
    quotients on the same polynomials; one GWC quotient is checked against linear_combination + kate_division"""
    n = 1 << 18
    queries = k18_queries()
    sets, super_points = k18_sets()
    groups = gwc.construct_point_groups(queries)
    keys = [key for _, members in sets for key in members]
    polys = {key: h.random_fr(n, 100 + i) for i, key in enumerate(keys)}
    rng = random.Random(18)
    y, v, u = (rng.randrange(2, R) for _ in range(3))
    zt = sh.vanishing_eval(super_points, u)
    z = [sh.vanishing_eval([p for p in super_points if p not in pts], u) for pts, _ in sets]

    def shplonk_route():
        hx = None
        for i, (pts, members) in enumerate(sets):
            hx = sh.set_quotient([polys[k] for k in members], [pow(y, j, R) for j in range(len(members))], pts, pow(v, i, R), out=hx, accumulate=i > 0)
        cols, weights = [], []
        for i, (pts, members) in enumerate(sets):
            for j, key in enumerate(members):
                cols.append(polys[key])
                weights.append(pow(v, i, R) * z[i] % R * pow(y, j, R) % R)
        return hx, sh.set_quotient(cols + [hx], weights + [-zt % R], [u], pow(z[0], -1, R))

    def gwc_route():
        return [sh.set_quotient([polys[key] for key, _ in members], [pow(v, j, R) for j in range(len(members))], [pt]) for pt, members in groups]

    pt, members = groups[-1]
    lc = h.linear_combination([polys[key] for key, _ in members], np.stack([fr_words(pow(v, j, R)) for j in range(len(members))]))
    want = torch.cat([h.kate_division(lc, fr_words(pt)), torch.zeros((1, 4), dtype=torch.int64, device="cuda")])
    assert torch.equal(gwc_route()[-1], want), "a GWC quotient differs from linear_combination + kate_division"
    routes = {"shplonk": shplonk_route, "gwc": gwc_route}
    times = {mo: [] for mo in multiopens}
    for mo in multiopens:
        routes[mo]()
    for _ in range(REPEATS):
        for mo in multiopens:
            times[mo].append(wall(routes[mo])[1])
    return {"n": n, "sets": [{"points": len(pts), "polynomials": len(members)} for pts, members in sets],
            "groups": [{"polynomials": len(members)} for _, members in groups], **{mo: spread(times[mo]) for mo in multiopens}}


def lookup_counts(cs, k):
    """commitments and evaluations of one proof under each lookup argument, and its bytes: counted, not measured"""
    from halo2_experiments_amd.verifier import proof_length
    adv_q, fix_q, _ = cs.queries()
    nsets, L, G, P = cs.permutation_sets(), len(cs.lookups), len(cs.logup_arguments()), len(cs.equality)
    base_c, base_e = cs.num_advice + nsets + 1 + (cs.degree() - 1), len(adv_q) + len(fix_q) + 1 + P + (3 * nsets - 1 if nsets else 0)
    return {"lookups": L, "logup_arguments": [len(ins) for _, ins in cs.logup_arguments()], "sorts_removed": 2 * L,
            "halo2": {"commitments": base_c + 3 * L, "evaluations": base_e + 5 * L, "proof_bytes": proof_length(cs, k=k)},
            "logup": {"commitments": base_c + 2 * G, "evaluations": base_e + 3 * G, "proof_bytes": proof_length(cs, k=k, lookup="logup")}}


def arguments(name, m, lookups):
    """(f): m proofs of one shape under every lookup argument of ``lookups``, the arguments alternating inside every repeat"""
    cs, lay, advice, instances = pmc.build_multi(name, m)
    params = ParamsKZG.setup(lay.k, pc.SRS_S)
    vk = h.keygen_vk(params, cs, lay)
    pk = h.keygen_pk(params, vk, cs, lay, cosets=False)

    def run(lk, rep):
        if m == 1:
            return [h.create_proof(params, pk, advice[0], instances[0], 1000 * rep, lookup=lk)]
        return h.create_proofs(params, pk, advice, instances, [1000 * rep + b for b in range(m)], lookup=lk)
    try:
        sizes = {}
        for lk in lookups:                                        # warm-up, and the first and last proof verify
            made = run(lk, 1)
            assert all(h.verify_proof(params, vk, instances[b], made[b], lookup=lk) for b in {0, m - 1})
            sizes[lk] = len(made[0])
        totals = {lk: [] for lk in lookups}
        for rep in range(REPEATS):
            for lk in lookups:
                totals[lk].append(wall(lambda: run(lk, 2 + rep))[1])
    finally:
        params.release()
    return {"k": lay.k, "proofs": m, "entry": "create_proof" if m == 1 else "create_proofs", "counts": lookup_counts(cs, lay.k),
            **{lk: {"proof_bytes": sizes[lk], "total": spread(totals[lk]), "per_proof_ms": round(statistics.median(totals[lk]) / m, 3)}
               for lk in lookups}}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def logup_kernels(k):
    """the two new kernels alone beside what they replace, on the sum tree's lookup shape: eight byte columns, one 256-entry table"""
    n = 1 << k
    u = n - 6
    rng = np.random.default_rng(k)
    col = lambda values: torch.from_numpy(ps.ints_to_words([int(v) for v in values]).view(np.int64)).cuda()
    table = col(np.arange(n) % 256)
    inputs = [col(rng.integers(0, 256, n)) for _ in range(8)]
    groups = [inputs[0:3], inputs[3:6], inputs[6:8]]
    factors = [h.random_fr(n, 70 + i) for i in range(8)]
    routes = {"logup_multiplicities_3_arguments": lambda: h.logup_multiplicities([table] * 3, groups, u),
              "lookup_permute_8_pairs": lambda: h.permute_expression_pairs(inputs, [table] * 8, u),
              "grand_sum_3_columns": lambda: h.grand_sum_batch(factors[:3]),
              "grand_product_8_columns": lambda: h.grand_product_batch(factors, fr_words(1))}
    times = {name: [] for name in routes}
    for fn in routes.values():
        fn()
    for _ in range(REPEATS):
        for name, fn in routes.items():
            times[name].append(events(fn))
    return {"rows": u, **{name: spread(ms) for name, ms in times.items()}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--circuits", type=int, default=0, help="m: time create_proof_multi and the h step for m circuits (1 .. 64) instead")
    ap.add_argument("--proofs", default="", help="m[,m...]: time create_proofs against the loop of m create_proof calls, with the h step and the "
                    "multiopen split out, for every listed m instead")
    ap.add_argument("--multiopen", choices=("shplonk", "gwc", "both"), default="",
                    help="time the multiopen schemes side by side (create_proof / create_proofs for every m of --proofs, default 1,16,64) instead")
    ap.add_argument("--lookup", choices=("halo2", "logup", "both"), default="",
                    help="time the lookup arguments side by side (create_proof / create_proofs for every m of --proofs, default 1,16,64) instead")
    args = ap.parse_args()
    torch.cuda.init()
    if args.lookup:
        lookups = ("halo2", "logup") if args.lookup == "both" else (args.lookup,)
        out = {"tool": "tools/prove_time.py --lookup", "repeats": REPEATS, "lookups_measured": list(lookups)}
        for name in ("merkle_sum_d5_k9", "merkle_sum_d20_k10"):
            out[name] = {f"proofs_{m}": arguments(name, int(m), lookups) for m in (args.proofs or "1,16,64").split(",")}
        out["kernels_alone"] = {f"k{k}": logup_kernels(k) for k in (10, 17)}
        print(json.dumps(out))
        sys.exit(0)
    if args.multiopen:
        multiopens = ("shplonk", "gwc") if args.multiopen == "both" else (args.multiopen,)
        out = {"tool": "tools/prove_time.py --multiopen", "repeats": REPEATS, "multiopens_measured": list(multiopens)}
        for name in ("merkle_sum_d5_k9", "merkle_sum_d20_k10"):
            out[name] = {f"proofs_{m}": schemes(name, int(m), multiopens) for m in (args.proofs or "1,16,64").split(",")}
        out["multiopen_k18"] = multiopen_k18_schemes(multiopens)
        print(json.dumps(out))
        sys.exit(0)
    if args.proofs:
        print(json.dumps({f"proofs_{m}": {name: proofs(name, int(m)) for name in ("merkle_sum_d20_k10", "merkle_sum_d5_k9")}
                          for m in args.proofs.split(",")}))
        sys.exit(0)
    if args.circuits:
        print(json.dumps({name: multi(name, args.circuits) for name in ("merkle_sum_d20_k10", "merkle_sum_d5_k9")}))
        sys.exit(0)
    out = {"merkle_sum_d5_k9": end_to_end("merkle_sum_d5_k9"), "merkle_sum_d20_k10": end_to_end("merkle_sum_d20_k10"),
           "multiopen_k18": multiopen_k18()}
    print(json.dumps(out))
