"""The integer half of the batch verifier (``batch_verifier`` holds the device half and says where the work is done): what a
constraint system fixes about a proof, the integer twins of the device's per-proof work, and the plans the terms kernels walk.
Nothing here needs a device.

  - ``ProofLayout``: the slots of a proof, its queries, its rotation sets -- taken symbolically on ROTATIONS -- and its transcript's
    schedule, for both wire formats and for proofs of m circuits;
  - the twins: ``read_proof_ints`` of the read kernel, ``transcript_challenges`` of the transcript (Blake2b, or Keccak for an "evm"
    layout), ``terms_from_challenges`` of the terms kernels, ``proof_terms_ints`` of the whole per-proof part and ``proof_sums_ints``
    of the per-proof sums.  With a layout of m circuits they take a list of m instances;
  - ``TermsPlan`` and ``MultiTermsPlan``: the words ``hm_verify_terms_dev`` / ``hm_verify_terms_multi_dev`` are driven by
    (csrc/verify_terms.inc states their layout), and the numerator's program lowered from the constraint system alone;
  - ``shared_points``, ``derive_randomizer`` and the constants the kernels' tables and plans share with the C side;
  - with ``multiopen="gwc"`` the layout of a proof that ends in the GWC multiopen (``gwc``), its twins -- ``terms_from_challenges``
    and ``proof_terms_ints`` then also return the scalars u^i of the witness points in L -- and ``GwcTermsPlan``, the words
    ``hm_verify_terms_gwc_dev`` is driven by.

Two places where the symbolic form answers differently from ``verify_proof``, each of probability about 2^-254 for an honest or a
dishonest prover alike (x is a hash output): x = 0, where all rotations of x coincide, is reported as a failing proof; and h pieces whose
combination sum_i x^(n i) [h_i] is the identity are summed as they are, where ``verify_proof`` refuses to open the identity."""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import evaluation as ev
from .bn256 import FR_MODULUS
from .keygen import FR_DELTA, VerifyingKey
from .pairing import G1_GEN, g1_msm, g1_mul
from .shplonk import g1_words_to_int
from .transcript import (PERSONAL, PREFIX_CHALLENGE, PREFIX_POINT, PREFIX_SCALAR, TranscriptError, check_encoding, check_lookup, check_multiopen,
                         g1_decompress_int, g1_uncompressed_int, keccak256)
from .verifier import _instance_columns, _vk_digest, evaluate_expression, proof_length

R = FR_MODULUS
VR_POINT, VR_TAIL = 1 << 31, 1 << 30          # csrc/verify_read.inc: the slot table's bits
EVM_POINT, EVM_TAIL, EVM_SKIP = 1 << 31, 1 << 30, 1 << 29   # csrc/keccak.inc: the bits of an "evm" layout's table (x slot, tail, y slot)
MAX_CIRCUITS = 64                                            # prover.MAX_CIRCUITS, stated again: the lanes of one gfx950 wavefront


class MalformedProof(ValueError):
    """What ``verify_proof`` answers False to on structural grounds: a wrong length, a scalar >= r, an x >= p or off the curve, an
    all-zero point, x^n = 1 (and x = 0, see the module's note)."""


# ---- what a constraint system fixes: the slots of a proof, its queries and its rotation sets ---------------------------------------------
class ProofLayout:
    """Everything about a proof that the constraint system, n = 2^k and the number of circuits in the proof fix, built once per
    ``vk`` (``circuits=1``, a ``create_proof`` proof, unless said otherwise; ``circuits=m``: the last paragraph):

      ``point_keys``   the commitments in the order the proof holds them: advice, lookup a' / s', permutation z, lookup z, random, the
                       h pieces, then -- behind the evaluations -- [h] and [h'].  All but the last are the proof's OWN points.
      ``eval_keys``    (commitment key, rotation mod n) of the evaluations, in the proof's order.
      ``slot_table``   one u32 per 32-byte slot as ``hm_verify_read_proofs_dev`` takes it.
      ``sets``         the rotation sets of the multiopen, [(rotations, [commitment keys])], and ``super_rotations``: grouping and order
                       of first appearance as ``shplonk.construct_intermediate_sets`` finds them on the real points x * omega^rotation.
                       Two rotations give one point exactly when they agree mod n (x != 0), so the sets need no challenge; inside a set
                       the points stand in ascending ROTATION here and in ascending integer order there, which changes no scalar.
      ``shared_keys``  the points all proofs share: the fixed commitments, the sigma commitments, the generator.

    ``encoding="evm"``: a point takes two 32-byte slots, x then y, so ``slots`` = 2 points + scalars, and ``slot_table`` is of the kind
    ``hm_verify_read_proofs_evm_dev`` takes: EVM_POINT | index on the x slot of an own point, EVM_POINT | EVM_TAIL on that of [h'],
    EVM_SKIP on every y slot, the index on a scalar slot.  ``point_slots`` are then the x slots.  Everything else is the same.

    ``circuits=m`` > 1, a ``create_proof_multi`` proof, every list in the order of ``verifier._verify`` with m instances: the points
    are the advice of circuit 0 .. m - 1, then lookup a' / s' per circuit, permutation z per circuit, lookup z per circuit, then
    random, the h pieces, [h], [h']; the evaluations the advice evaluations per circuit, then fixed, random, sigma, then the
    permutation and the lookup evaluations per circuit.  A per-circuit key is (kind, index, circuit); shared keys stay as they are.
    The rotation sets are the single-circuit ones in the same order (circuit 0's queries come first), the members of a set circuit
    0's keys, circuit 1's, ..., then the shared ones.  ``lane`` is the single-circuit layout of the same system (the layout itself
    when m = 1).  ``encoding="evm"`` with m > 1 raises ValueError.

    ``multiopen="gwc"`` (``gwc``; single-circuit only, ``circuits`` > 1 raises ValueError): behind the evaluations the proof holds one
    witness point per distinct query point, so ``point_keys`` ends in ("w", 0) .. ("w", q - 1).  ALL points are own points: there is no
    tail point and no slot has a tail bit.  ``groups`` = [(rotation, [member keys])] stands in place of ``sets``: the distinct
    rotations in order of first appearance in ``queries``, every group's members in list order -- what
    ``gwc.construct_point_groups`` finds on the real points, by the argument above.  The transcript has seven challenges
    (``GWC_RECORD``): the schedule ends ... | evaluations | v | q points | u.

    ``lookup="logup"``: the lookups stand as the G arguments of ``cs.logup_arguments()``.  Per circuit the
    points ("logup_m", g) take the place of the lookup a' / s' pairs and ("logup_phi", g) that of the lookup z; the evaluations per
    circuit and argument are phi at 0 and 1 and m at 0, the queries phi(0), m(0), phi(1); ``exprs`` holds
    ``evaluation.logup_expressions`` over the table entries (phi, m) from ``lookup0`` on.  ``L`` is then 0 and ``G`` the number of
    arguments; ``step5_points`` / ``step8_points`` are the per-circuit point counts between theta and beta and between gamma and the
    random polynomial under either argument.  The integer twins below read such a layout; the terms plans and the batch verifier
    do not (ValueError)."""

    def __init__(self, cs, k: int, encoding: str = "halo2", circuits: int = 1, multiopen: str = "shplonk", lookup: str = "halo2"):
        self.encoding = check_encoding(encoding, "ProofLayout")
        self.multiopen = check_multiopen(multiopen, "ProofLayout")
        self.lookup = check_lookup(lookup, "ProofLayout")
        m = int(circuits)
        if not 1 <= m <= MAX_CIRCUITS:
            raise ValueError(f"ProofLayout: need 1 <= circuits <= {MAX_CIRCUITS}, got {circuits!r}")
        if m > 1 and encoding == "evm":
            raise ValueError("ProofLayout: a multi-circuit proof has no \"evm\" encoding (create_proof_multi writes none)")
        if m > 1 and multiopen == "gwc":
            raise ValueError("ProofLayout: multi-circuit proofs with the \"gwc\" multiopen are not laid out (circuits > 1)")
        self.circuits = m
        self.lane = self if m == 1 else ProofLayout(cs, k, encoding, lookup=lookup)       # what ONE circuit of the proof looks like
        self.cs, self.k, self.n = cs, k, 1 << k
        n = self.n
        adv_q, fix_q, _ = cs.queries()
        arguments = cs.logup_arguments() if lookup == "logup" else []
        self.P, self.nsets, self.L, self.G = len(cs.equality), cs.permutation_sets(), 0 if lookup == "logup" else len(cs.lookups), len(arguments)
        P_, nsets, L, G = self.P, self.nsets, self.L, self.G
        self.step5_points, self.step8_points = 2 * L + G, nsets + L + G
        self.pieces = cs.degree() - 1
        self.last = -(cs.blinding_factors + 1)
        last = self.last
        M = range(m)
        per = self.circuit_key
        pts = [per(("advice", i), c) for c in M for i in range(cs.num_advice)]
        for c in M:
            for j in range(L):
                pts += [per(("lookup_a", j), c), per(("lookup_s", j), c)]
            pts += [per(("logup_m", g), c) for g in range(G)]
        pts += [per(("perm_z", i), c) for c in M for i in range(nsets)]
        pts += [per((kd, j), c) for c in M for kd, count in (("lookup_z", L), ("logup_phi", G)) for j in range(count)] + [("random",)]
        pts += [("h_piece", i) for i in range(self.pieces)]
        self.points_before_evals = len(pts)
        evs = [(per(("advice", i), c), r % n) for c in M for i, r in adv_q] + [(("fixed", i), r % n) for i, r in fix_q] + [(("random",), 0)]
        evs += [(("sigma", j), 0) for j in range(P_)]
        for c in M:
            for i in range(nsets):
                evs += [(per(("perm_z", i), c), r % n) for r in (0, 1) + ((last,) if i + 1 < nsets else ())]
        for c in M:
            for j in range(L):
                evs += [(per((kd, j), c), r % n) for kd, r in (("lookup_z", 0), ("lookup_z", 1), ("lookup_a", 0), ("lookup_a", -1), ("lookup_s", 0))]
            for g in range(G):
                evs += [(per((kd, g), c), r) for kd, r in (("logup_phi", 0), ("logup_phi", 1), ("logup_m", 0))]
        # the queries in the order verifier._verify lists them; ("h",) stands for sum_i x^(n i) [h_i]
        q = []
        for c in M:
            q += [(per(("advice", i), c), r % n) for i, r in adv_q]
            q += [qq for i in range(nsets) for qq in ((per(("perm_z", i), c), 0), (per(("perm_z", i), c), 1))]
            q += [(per(("perm_z", i), c), last % n) for i in reversed(range(nsets - 1))]
            for j in range(L):
                q += [(per(("lookup_z", j), c), 0), (per(("lookup_a", j), c), 0), (per(("lookup_s", j), c), 0),
                      (per(("lookup_a", j), c), (-1) % n), (per(("lookup_z", j), c), 1)]
            for g in range(G):
                q += [(per(("logup_phi", g), c), 0), (per(("logup_m", g), c), 0), (per(("logup_phi", g), c), 1 % n)]
        q += [(("fixed", i), r % n) for i, r in fix_q] + [(("sigma", j), 0) for j in range(P_)]
        q += [(("h",), 0), (("random",), 0)]
        self.queries = q
        gwc = multiopen == "gwc"
        if gwc:
            if len(set(q)) != len(q):
                raise AssertionError("ProofLayout: the query list names a (key, rotation) pair twice")
            groups: List[Tuple[int, list]] = []
            for key, rot in q:
                for have, keys in groups:
                    if have == rot:
                        keys.append(key)
                        break
                else:
                    groups.append((rot, [key]))
            self.groups = groups
        self.point_keys = pts + ([("w", i) for i in range(len(self.groups))] if gwc else [("h1",), ("h2",)])
        self.eval_keys = evs
        self.eval_index = {}
        for at, key in enumerate(evs):
            self.eval_index.setdefault(key, at)
        self.n_points, self.own_points, self.n_scalars = len(self.point_keys), len(self.point_keys) - (0 if gwc else 1), len(evs)
        self.slots = (2 if encoding == "evm" else 1) * self.n_points + self.n_scalars
        if 32 * self.slots != proof_length(cs, m, encoding, multiopen, k, lookup):
            raise AssertionError("ProofLayout: the slots do not add up to proof_length")
        behind = range(self.points_before_evals, self.n_points)          # the multiopen's points, behind the evaluations
        if encoding == "evm":
            table = [e for i in range(self.points_before_evals) for e in (EVM_POINT | i, EVM_SKIP)] + list(range(self.n_scalars))
            if gwc:
                table += [e for i in behind for e in (EVM_POINT | i, EVM_SKIP)]
            else:
                table += [EVM_POINT | (self.n_points - 2), EVM_SKIP, EVM_POINT | EVM_TAIL | (self.n_points - 1), EVM_SKIP]
        else:
            table = [VR_POINT | i for i in range(self.points_before_evals)] + list(range(self.n_scalars))
            if gwc:
                table += [VR_POINT | i for i in behind]
            else:
                table += [VR_POINT | (self.n_points - 2), VR_POINT | VR_TAIL | (self.n_points - 1)]
        self.slot_table = np.array(table, dtype=np.uint32)
        self.point_slots = [s for s, e in enumerate(table) if e & VR_POINT]
        self.scalar_slots = [s for s, e in enumerate(table) if not e & (VR_POINT | (EVM_SKIP if encoding == "evm" else 0))]

        by_key: dict = {}
        for key, rot in q:
            by_key.setdefault(key, [])
            if rot not in by_key[key]:
                by_key[key].append(rot)
        sets: List[Tuple[tuple, list]] = []
        for key, rots in by_key.items():
            rots_t = tuple(sorted(rots))
            for have, keys in sets:
                if have == rots_t:
                    keys.append(key)
                    break
            else:
                sets.append((rots_t, [key]))
        if not gwc:
            self.sets = [(list(rots), keys) for rots, keys in sets]
        self.super_rotations = sorted({rot for _, rot in q})
        self.shared_keys = [("fixed", c) for c in range(cs.num_fixed)] + [("sigma", j) for j in range(P_)] + [("g",)]
        self.shared_index = {key: i for i, key in enumerate(self.shared_keys)}
        self.own_index = {key: i for i, key in enumerate(self.point_keys)}

        # the expressions of the identity, in the prover's order (verifier._verify builds the same list)
        nf = cs.num_fixed
        self.sigma0, self.z0 = nf, nf + P_
        z0 = self.z0
        self.i_l0, self.i_last, self.i_active, self.i_x, self.lookup0 = z0 + nsets, z0 + nsets + 1, z0 + nsets + 2, z0 + nsets + 3, z0 + nsets + 4
        F = ev.Fixed
        kind = {"advice": ev.Advice, "fixed": ev.Fixed, "instance": ev.Instance}
        exprs = list(cs.polynomials())
        exprs += ev.permutation_expressions([kind[kd](i) for kd, i in cs.equality], [F(self.sigma0 + j) for j in range(P_)],
                                            [lambda r, i=i: F(z0 + i, r) for i in range(nsets)], F(self.i_l0), F(self.i_last),
                                            F(self.i_active), F(self.i_x), cs.permutation_chunk_len(), FR_DELTA, last)
        for g, (tabs, ins_list) in enumerate(arguments):
            b = self.lookup0 + 2 * g
            exprs += ev.logup_expressions(ins_list, tabs, lambda r, b=b: F(b, r), lambda r, b=b: F(b + 1, r), F(self.i_l0), F(self.i_last),
                                          F(self.i_active))
        for j, (ins, tabs) in enumerate(cs.lookups if lookup == "halo2" else []):
            b = self.lookup0 + 3 * j
            exprs += ev.lookup_expressions(ins, tabs, lambda r, b=b: F(b, r), lambda r, b=b: F(b + 1, r), lambda r, b=b: F(b + 2, r),
                                           F(self.i_l0), F(self.i_last), F(self.i_active))
        self.exprs = exprs

    def circuit_key(self, key: tuple, c: int) -> tuple:
        """circuit c's copy of a per-circuit key: (kind, index, circuit) in a layout of several circuits, the key itself in one of one"""
        return key if self.circuits == 1 else key + (c,)

    def transcript_schedule(self) -> List[Tuple[int, int]]:
        """The (absorb a slots, squeeze s challenges) pairs of a proof's transcript over its slots in order, from the
        counts ``transcript_challenges`` uses: advice | theta | 2L | beta, gamma | sets + L + 1 | y | pieces | x | evaluations | y', v
        | [h] | u, and a last pair that absorbs [h'] behind the last challenge, as ``Blake2bRead`` does.  The counts are SLOTS: in an
        "evm" layout a point counts twice, and with ``circuits = m`` the per-circuit counts (advice, 2L, sets + L) are taken m times.
        A "gwc" layout ends ... | evaluations | v | the q witness points | u: seven challenges, nothing absorbed behind the last."""
        w, m = 2 if self.encoding == "evm" else 1, self.circuits
        pairs = [(w * m * self.cs.num_advice, 1), (w * m * self.step5_points, 2), (w * (m * self.step8_points + 1), 1), (w * self.pieces, 1)]
        pairs += [(self.n_scalars, 1), (w * len(self.groups), 1)] if self.multiopen == "gwc" else [(self.n_scalars, 2), (w, 1), (w, 0)]
        if sum(a for a, _ in pairs) != self.slots or sum(s for _, s in pairs) != len(self.record):
            raise AssertionError("ProofLayout: the transcript's schedule does not cover the proof's slots and its challenges")
        return pairs

    @property
    def record(self) -> tuple:
        """the names of the transcript's challenges in order: ``RECORD``, or ``GWC_RECORD`` for a "gwc" layout"""
        return GWC_RECORD if self.multiopen == "gwc" else RECORD


def read_proof_ints(layout: ProofLayout, proof: bytes):
    """The integer twin of the read kernel: (points, scalars) of ``proof`` in the layout's order -- points as (x, y) -- or
    ``MalformedProof`` for a wrong length, a scalar >= r, an x >= p or off the curve, the all-zero point.  An "evm" layout reads the
    other encoding: a coordinate >= p, a point off the curve (the 64 zero bytes among them), a scalar >= r."""
    if len(proof) != 32 * layout.slots:
        raise MalformedProof("the proof has the wrong length")
    points, scalars = [], []
    if layout.encoding == "evm":
        for s in range(layout.slots):
            entry = int(layout.slot_table[s])
            if entry & EVM_POINT:
                try:
                    points.append(g1_uncompressed_int(proof[32 * s:32 * s + 64]))
                except TranscriptError as e:
                    raise MalformedProof(str(e)) from None
            elif not entry & EVM_SKIP:
                v = int.from_bytes(proof[32 * s:32 * s + 32], "big")
                if v >= R:
                    raise MalformedProof("scalar: not below r")
                scalars.append(v)
        return points, scalars
    for s in range(layout.slots):
        data = proof[32 * s:32 * s + 32]
        if layout.slot_table[s] & VR_POINT:
            try:
                p = g1_decompress_int(data)
            except TranscriptError as e:
                raise MalformedProof(str(e)) from None
            if p is None:
                raise MalformedProof("point: the identity cannot be absorbed")
            points.append(p)
        else:
            v = int.from_bytes(data, "little")
            if v >= R:
                raise MalformedProof("scalar: not below r")
            scalars.append(v)
    return points, scalars


def _per_circuit(layout: ProofLayout, inst_cols) -> list:
    """the instance columns circuit by circuit: a single-circuit layout takes one circuit's columns, a multi-circuit one a list of m"""
    if layout.circuits == 1:
        return [inst_cols]
    per = list(inst_cols)
    if len(per) != layout.circuits:
        raise ValueError(f"a layout of {layout.circuits} circuits takes {layout.circuits} instances, got {len(per)}")
    return per


def _layout_instances(layout: ProofLayout, instance):
    """what ``add_proof`` and the twins are given, as instance columns: one circuit's, or with a multi-circuit layout a list of m"""
    if layout.circuits == 1:
        return _instance_columns(layout.cs, instance)
    per = [_instance_columns(layout.cs, one) for one in instance]
    if len(per) != layout.circuits:
        raise ValueError(f"a proof of {layout.circuits} circuits takes {layout.circuits} instances, got {len(per)}")
    return per


def _keccak_challenges(layout: ProofLayout, vk_digest: int, inst_cols, proof: bytes) -> dict:
    """``transcript_challenges`` of an "evm" layout: the preamble big-endian, then the proof's slots verbatim by the layout's schedule;
    the buffer rules are ``transcript``'s"""
    buf = bytearray(vk_digest.to_bytes(32, "big") + b"".join(int(v).to_bytes(32, "big") for values in inst_cols for v in values))
    out, at = [], 0
    for absorb, squeeze in layout.transcript_schedule():
        buf += proof[at:at + 32 * absorb]
        at += 32 * absorb
        for _ in range(squeeze):
            h = keccak256(bytes(buf) + (b"\x01" if len(buf) == 32 else b""))
            buf = bytearray(h)
            out.append(int.from_bytes(h, "big") % R)
    return dict(zip(layout.record, out))


def transcript_challenges(layout: ProofLayout, vk_digest: int, inst_cols, proof: bytes, y_bytes: Optional[Sequence[bytes]] = None) -> dict:
    """The Blake2b transcript of one proof, absorbed in the order of ``verifier._verify`` and ``shplonk.verify_opening``:
    ``y_bytes[j]`` the 32 canonical bytes of y of the proof's point j (x stands in the proof).  -> theta, beta, gamma, y, x and the
    multiopen's y' (``y2``), v, u.  With an "evm" layout the Keccak transcript, which absorbs the proof verbatim and takes no
    ``y_bytes``."""
    if layout.encoding == "evm":
        return _keccak_challenges(layout, vk_digest, inst_cols, proof)
    st = hashlib.blake2b(digest_size=64, person=PERSONAL)
    slot = [0]
    point = [0]

    def scalar(v: int) -> None:
        st.update(PREFIX_SCALAR + v.to_bytes(32, "little"))

    def points(count: int) -> None:
        for _ in range(count):
            at = 32 * slot[0]
            st.update(PREFIX_POINT + proof[at:at + 31] + bytes([proof[at + 31] & 0x7F]) + y_bytes[point[0]])
            slot[0] += 1
            point[0] += 1

    def squeeze() -> int:
        st.update(PREFIX_CHALLENGE)
        return int.from_bytes(st.copy().digest(), "little") % R

    cs, m = layout.cs, layout.circuits
    scalar(vk_digest)
    for columns in _per_circuit(layout, inst_cols):
        for values in columns:
            for v in values:
                scalar(v)
    ch = {}
    points(m * cs.num_advice)
    ch["theta"] = squeeze()
    points(m * layout.step5_points)
    ch["beta"] = squeeze()
    ch["gamma"] = squeeze()
    points(m * layout.step8_points + 1)
    ch["y"] = squeeze()
    points(layout.pieces)
    ch["x"] = squeeze()
    for _ in range(layout.n_scalars):
        at = 32 * slot[0]
        st.update(PREFIX_SCALAR + proof[at:at + 32])
        slot[0] += 1
    if layout.multiopen == "gwc":
        ch["v"] = squeeze()
        points(len(layout.groups))
        ch["u"] = squeeze()
        return ch
    ch["y2"] = squeeze()
    ch["v"] = squeeze()
    points(1)
    ch["u"] = squeeze()
    return ch


def terms_from_challenges(layout: ProofLayout, omega: int, inst_cols, evals: Sequence[int], ch: dict, details: Optional[dict] = None):
    """The scalars of one proof's R = sum own[j] * (point j of the proof) + sum shared[i] * (shared point i), from its evaluations (in
    the proof's order) and its challenges: ``own`` has one entry per point of ``layout.point_keys`` ([h'] last, with u), ``shared`` one
    per ``layout.shared_keys``.  ``MalformedProof`` when x^n = 1 (or x = 0).  ``details``, when given, receives what the device keeps in
    its value row: l0, l_last, l_active, the instance evaluations by (column, rotation), the numerator and h(x)."""
    cs, n, m = layout.cs, layout.n, layout.circuits
    insts, per = _per_circuit(layout, inst_cols), layout.circuit_key
    x, y = ch["x"], ch["y"]
    xn = pow(x, n, R)
    if xn == 1 or x == 0:
        raise MalformedProof("x^n = 1: the quotient cannot be taken" if x else "x = 0")
    wpow = lambda r: pow(omega, r % n, R)
    n_inv = pow(n, -1, R)
    zh = (xn - 1) * n_inv % R                                    # (point^n - 1) / n, the same for every rotation of x

    def lagrange_at(i: int, rot: int) -> int:                     # l_i(x omega^rot): never a zero denominator, since x^n != 1
        w = wpow(i)
        return w * zh % R * pow(x * wpow(rot) - w, -1, R) % R

    blinding = cs.blinding_factors
    l0, l_last = lagrange_at(0, 0), lagrange_at(n - blinding - 1, 0)
    l_blind = sum(lagrange_at(i, 0) for i in range(n - blinding, n)) % R
    l_active = (1 - l_last - l_blind) % R
    special = {layout.i_l0: l0, layout.i_last: l_last, layout.i_active: l_active, layout.i_x: x}
    ev_at = lambda key, r: evals[layout.eval_index[(key, r % n)]]
    nf = cs.num_fixed

    def leaf_of(c: int):
        def leaf(kind: str, column: int, r: int) -> int:
            if kind == "instance":
                value = sum(v * lagrange_at(i, r) for i, v in enumerate(insts[c][column]) if v) % R
                if details is not None:
                    details.setdefault("instance", {})[per((column, r % n), c)] = value
                return value
            if kind == "advice":
                return ev_at(per(("advice", column), c), r)
            if column < nf:
                return ev_at(("fixed", column), r)
            if column in special:
                return special[column]
            if column < layout.z0:
                return ev_at(("sigma", column - layout.sigma0), r)
            if column < layout.i_l0:
                return ev_at(per(("perm_z", column - layout.z0), c), r)
            if layout.lookup == "logup":
                g, part = divmod(column - layout.lookup0, 2)
                return ev_at(per((("logup_phi", "logup_m")[part], g), c), r)
            j, part = divmod(column - layout.lookup0, 3)
            return ev_at(per((("lookup_z", "lookup_a", "lookup_s")[part], j), c), r)
        return leaf

    scalars = {"Beta": ch["beta"], "Gamma": ch["gamma"], "Theta": ch["theta"]}
    acc, numerators = 0, []
    for c in range(m):                                            # ONE running value: circuit 0's expressions, then circuit 1's, ...
        leaf, own_fold = leaf_of(c), 0
        for e in layout.exprs:
            value = evaluate_expression(e, leaf, scalars)
            acc, own_fold = (acc * y + value) % R, (own_fold * y + value) % R
        numerators.append(own_fold)                               # N_c: what lane c of the device computes; acc = sum_c y^(E (m-1-c)) N_c
    hx = acc * pow(xn - 1, -1, R) % R
    if details is not None:
        details.update(l0=l0, l_last=l_last, l_active=l_active, numerator=acc, hx=hx)
        if m > 1:
            details["numerators"] = numerators

    if layout.multiopen == "gwc":
        return _gwc_terms(layout, wpow, ev_at, hx, xn, ch)

    # ---- the multiopen's scalars, per rotation set ---------------------------------------------------------------------------------
    y2, v, u = ch["y2"], ch["v"], ch["u"]
    pt = {rot: x * wpow(rot) % R for rot in layout.super_rotations}
    diff = {rot: (u - p) % R for rot, p in pt.items()}            # u - point; zero only when u hits a point
    zt = 1
    for d in diff.values():
        zt = zt * d % R
    own, shared = [0] * layout.n_points, [0] * len(layout.shared_keys)
    r_outer, z0_inv, v_i = 0, None, 1
    for i, (rots, keys) in enumerate(layout.sets):
        z_i = 1
        for rot in layout.super_rotations:
            if rot not in rots:
                z_i = z_i * diff[rot] % R
        if i == 0:
            if z_i == 0:
                raise MalformedProof("u is a point of the opening")
            z0_inv, z_i = pow(z_i, -1, R), 1
        else:
            z_i = z_i * z0_inv % R
        outer = v_i * z_i % R
        v_i = v_i * v % R
        basis = []                                                # the Lagrange basis of the set's points at u
        for l, rl in enumerate(rots):
            num = den = 1
            for m, rm in enumerate(rots):
                if m != l:
                    num = num * diff[rm] % R
                    den = den * (pt[rl] - pt[rm]) % R
            basis.append(num * pow(den, -1, R) % R)
        yj = 1
        for key in keys:
            coeff = outer * yj % R
            yj = yj * y2 % R
            values = [hx] if key == ("h",) else [ev_at(key, rot) for rot in rots]
            r_outer = (r_outer + coeff * sum(b * e for b, e in zip(basis, values))) % R
            if key == ("h",):
                xp = 1
                for piece in range(layout.pieces):
                    own[layout.own_index[("h_piece", piece)]] = coeff * xp % R
                    xp = xp * xn % R
            elif key in layout.shared_index:
                shared[layout.shared_index[key]] = coeff
            else:
                own[layout.own_index[key]] = coeff
    shared[layout.shared_index[("g",)]] = -r_outer % R
    own[layout.own_index[("h1",)]] = -z0_inv * zt % R
    own[layout.own_index[("h2",)]] = u
    return own, shared


def _gwc_terms(layout: ProofLayout, wpow, ev_at, hx: int, xn: int, ch: dict):
    """the GWC half of ``terms_from_challenges``: per group i and member j the scalar u^i v^j ADDED to the member's row (a commitment
    opened at several points is a member of several groups), the generator's -sum u^i v^j e_ij, and u^i z_i on W_i's own row.
    -> (own, shared, left): ``left[i]`` = u^i, the scalar of W_i in L."""
    x, v, u = ch["x"], ch["v"], ch["u"]
    own, shared, left = [0] * layout.n_points, [0] * len(layout.shared_keys), []
    e_sum, u_i = 0, 1
    for i, (rot, keys) in enumerate(layout.groups):
        coeff = u_i
        for key in keys:
            e_sum = (e_sum + coeff * (hx if key == ("h",) else ev_at(key, rot))) % R
            if key == ("h",):
                xp = 1
                for piece in range(layout.pieces):
                    at = layout.own_index[("h_piece", piece)]
                    own[at] = (own[at] + coeff * xp) % R
                    xp = xp * xn % R
            elif key in layout.shared_index:
                shared[layout.shared_index[key]] = (shared[layout.shared_index[key]] + coeff) % R
            else:
                own[layout.own_index[key]] = (own[layout.own_index[key]] + coeff) % R
            coeff = coeff * v % R
        own[layout.own_index[("w", i)]] = u_i * x % R * wpow(rot) % R
        left.append(u_i)
        u_i = u_i * u % R
    shared[layout.shared_index[("g",)]] = -e_sum % R
    return own, shared, left


# ---- the plan of the terms kernel (csrc/verify_terms.inc) ---------------------------------------------------------------------------------
VT_NO_SLOT, VT_T_SHARED, VT_T_H = 0xFFFFFFFF, 1 << 31, 1 << 30
VT_MAX_VALS, VT_MAX_INST_ROWS, VT_MAX_SUPER, VT_MAX_T = 256, 64, 32, 8
RECORD = ("theta", "beta", "gamma", "y", "x", "y2", "v", "u")          # then r_b: the per-proof record of hm_verify_terms_dev
GWC_RECORD = ("theta", "beta", "gamma", "y", "x", "v", "u")            # then r_b: the record of hm_verify_terms_gwc_dev


def _internal_words(v: int) -> List[int]:
    """the 9 limbs of 29 bits of v * 2^261 mod r: a constant as the kernels hold it"""
    m = v % R * (1 << 261) % R
    return [(m >> (29 * i)) & 0x1FFFFFFF for i in range(9)]


class TermsPlan:
    """What ``hm_verify_terms_dev`` needs beside the proofs, built once per constraint system and instance shape: the program of the
    gate, permutation and lookup expressions folded in y -- ``layout.exprs`` through ``GraphEvaluator.add_custom_gates``, lowered from
    the constraint system alone, undivided, with beta, gamma, theta, y as per-call constants (``lowered``: the arguments of
    ``hm_graph_create``) -- and the plan words (``words``; csrc/verify_terms.inc states the layout): where a (column, rotation) of the
    program stands in a proof's value row, the instance queries, the rotation sets on rotations, the constants in internal form.
    ``inst_rows[c]``: the rows given of instance column c (at most 64).  Needs no device."""

    def __init__(self, layout: ProofLayout, omega: int, inst_rows: Sequence[int]):
        if layout.lookup != "halo2":
            raise ValueError(f"{type(self).__name__}: the terms plans walk lookup=\"halo2\" layouts only (a logUp proof is verified by verify_proof)")
        cs, n = layout.cs, layout.n
        inst_rows = [int(r) for r in inst_rows]
        if len(inst_rows) != cs.num_instance:
            raise ValueError(f"TermsPlan: {cs.num_instance} instance column(s) expected")
        if any(r > VT_MAX_INST_ROWS for r in inst_rows):
            raise ValueError(f"TermsPlan: an instance column longer than {VT_MAX_INST_ROWS} rows")
        g = ev.GraphEvaluator()
        g.add_custom_gates(layout.exprs)
        num_fixed = layout.lookup0 + 3 * layout.L
        self.lowered = g.lower(num_fixed, cs.num_advice, cs.num_instance)
        rotations, n_cols = list(g.rotations), self.lowered["n_columns"]
        n_rot = max(len(rotations), 1)
        used = set()                                              # the (column, rotation index) pairs the program reads
        for op, a, b, c, _ in self.lowered["calcs"].tolist():
            for s in (a, b, c)[:3 if op == 7 else 2 if op <= 2 else 1]:
                if s >> 30 == 2:
                    used.add((s & 0x3FFF, (s >> 20) & 1023))
        s_l0 = layout.n_scalars
        s_inst = s_l0 + 4
        inst_first = num_fixed + cs.num_advice
        inst_queries = sorted((col - inst_first, rotations[ri] % n) for col, ri in used if col >= inst_first)
        inst_queries = sorted(set(inst_queries))
        s_hx = s_inst + len(inst_queries)
        n_vals = s_hx + 1
        if n_vals > VT_MAX_VALS:
            raise ValueError(f"TermsPlan: more than {VT_MAX_VALS} value slots")
        point_rotations = self._point_rotations(layout)           # the rotations whose omega^rot stand at c_super, in the walk's order

        def slot_of(col: int, rot: int) -> int:
            if col >= inst_first:
                return s_inst + inst_queries.index((col - inst_first, rot))
            if col >= num_fixed:
                return layout.eval_index[(("advice", col - num_fixed), rot)]
            if col < cs.num_fixed:
                return layout.eval_index[(("fixed", col), rot)]
            if layout.i_l0 <= col <= layout.i_x:
                return s_l0 + col - layout.i_l0
            if col < layout.z0:
                return layout.eval_index[(("sigma", col - layout.sigma0), rot)]
            if col < layout.i_l0:
                return layout.eval_index[(("perm_z", col - layout.z0), rot)]
            j, part = divmod(col - layout.lookup0, 3)
            return layout.eval_index[((("lookup_z", "lookup_a", "lookup_s")[part], j), rot)]

        colmap = [VT_NO_SLOT] * (n_cols * n_rot)
        for col, ri in used:
            colmap[col * n_rot + ri] = slot_of(col, rotations[ri] % n)

        consts: List[int] = [pow(n, -1, R)]

        def const(v: int) -> int:
            consts.append(v % R)
            return len(consts) - 1

        w = lambda e: pow(omega, e % n, R)
        blinding = cs.blinding_factors
        lagrange_rows = [0, n - blinding - 1] + list(range(n - blinding, n))
        c_lagrange = len(consts)
        for i in lagrange_rows:
            const(w(i))
        c_rows = len(consts)
        for i in range(max(inst_rows, default=0)):
            const(w(i))
        c_super = len(consts)
        for rot in point_rotations:
            const(w(rot))
        inst_off = [sum(inst_rows[:c]) for c in range(cs.num_instance)]
        inst_words: List[int] = []
        for col, rot in inst_queries:
            inst_words += [inst_off[col], inst_rows[col], const(w(rot))]
        set_words, n_sets = self._opening_words(layout, const, w, c_super, s_hx)
        header = 24
        off_colmap = header
        off_inst = off_colmap + len(colmap)
        off_sets = off_inst + len(inst_words)
        off_consts = off_sets + len(set_words)
        head = [layout.k, layout.n_scalars, n_vals, len(lagrange_rows), len(inst_queries), len(point_rotations), n_sets,
                layout.pieces, layout.own_points, len(layout.shared_keys), n_rot, n_cols, off_colmap, off_inst, off_sets, sum(inst_rows),
                c_lagrange, c_rows, c_super, s_l0, s_inst, s_hx, len(consts), off_consts]
        assert len(head) == header
        body = head + colmap + inst_words + set_words + [limb for v in consts for limb in _internal_words(v)]
        self.words = np.array(body, dtype=np.uint32)
        self.inst_rows, self.inst_queries, self.n_vals, self.n_columns = inst_rows, inst_queries, n_vals, n_cols
        self.s_l0, self.s_inst, self.s_hx = s_l0, s_inst, s_hx
        self.inst_elems = max(sum(inst_rows), 1)                  # the instance array is never empty: one zero element at least

    def _point_rotations(self, layout: ProofLayout) -> List[int]:
        if layout.multiopen != "shplonk":
            raise ValueError("TermsPlan: the layout's multiopen is not \"shplonk\" (GwcTermsPlan walks a \"gwc\" layout)")
        if len(layout.super_rotations) > VT_MAX_SUPER or any(len(rots) > VT_MAX_T for rots, _ in layout.sets):
            raise ValueError("TermsPlan: more rotations than the kernel's workspace holds")
        return layout.super_rotations

    def _opening_words(self, layout: ProofLayout, const, w, c_super: int, s_hx: int):
        """the words of the multiopen's walk and the number of its sets: here the rotation sets of SHPLONK"""
        set_words: List[int] = []
        for rots, keys in layout.sets:
            sup = [layout.super_rotations.index(r) for r in rots]
            dinv = []
            for rl in rots:                                       # 1 / prod_{m != l} (omega^r_l - omega^r_m); the x^(t-1) is the lane's
                den = 1
                for rm in rots:
                    if rm != rl:
                        den = den * (w(rl) - w(rm)) % R
                dinv.append(const(pow(den, -1, R)))
            set_words += [len(rots), sum(1 << s for s in sup), len(keys)] + sup + dinv
            for key in keys:
                if key == ("h",):
                    if len(rots) != 1:
                        raise AssertionError("TermsPlan: h is opened at x alone")
                    set_words += [VT_T_H | layout.own_index[("h_piece", 0)], s_hx]
                elif key in layout.shared_index:
                    set_words += [VT_T_SHARED | layout.shared_index[key]] + [layout.eval_index[(key, r)] for r in rots]
                else:
                    set_words += [layout.own_index[key]] + [layout.eval_index[(key, r)] for r in rots]
        return set_words, len(layout.sets)

    def instance_row(self, inst_cols) -> List[int]:
        """one proof's instance values as the kernel reads them: column after column, every column padded to the plan's rows"""
        row: List[int] = []
        for values, rows in zip(inst_cols, self.inst_rows):
            if len(values) > rows:
                raise ValueError("TermsPlan: an instance column longer than the plan's")
            row += list(values) + [0] * (rows - len(values))
        return row or [0]


class GwcTermsPlan(TermsPlan):
    """What ``hm_verify_terms_gwc_dev`` needs beside the proofs of a "gwc" layout, a sibling of ``TermsPlan``: the header, the column
    map, the instance queries and the constants are the same words (VT_N_SUPER = VT_N_SETS = q, the constants at VT_C_SUPER the
    omega^rot of the groups in their order); at VT_OFF_SETS stand the point groups in place of the rotation sets -- per group
    (constant index of omega^rot, the own row of W_i, members), then per member (target, evaluation slot), the targets as in
    ``TermsPlan`` (csrc/verify_terms.inc, at vg_plan_problem, states the layout).  ``lowered`` is the same program."""

    def _point_rotations(self, layout: ProofLayout) -> List[int]:
        if layout.multiopen != "gwc":
            raise ValueError("GwcTermsPlan: the layout's multiopen is not \"gwc\"")
        if len(layout.groups) > VT_MAX_SUPER:
            raise ValueError(f"GwcTermsPlan: more than {VT_MAX_SUPER} point groups")
        return [rot for rot, _ in layout.groups]

    def _opening_words(self, layout: ProofLayout, const, w, c_super: int, s_hx: int):
        words: List[int] = []
        for i, (rot, keys) in enumerate(layout.groups):
            words += [c_super + i, layout.own_index[("w", i)], len(keys)]
            for key in keys:
                if key == ("h",):
                    if rot != 0:
                        raise AssertionError("GwcTermsPlan: h is opened at x alone")
                    words += [VT_T_H | layout.own_index[("h_piece", 0)], s_hx]
                elif key in layout.shared_index:
                    words += [VT_T_SHARED | layout.shared_index[key], layout.eval_index[(key, rot)]]
                else:
                    words += [layout.own_index[key], layout.eval_index[(key, rot)]]
        return words, len(layout.groups)


VM_HDR = 12                                                       # csrc/verify_terms.inc: the words of a multi plan's header


class MultiTermsPlan:
    """What ``hm_verify_terms_multi_dev`` needs beside the proofs of a multi-circuit layout: the ``TermsPlan`` of ONE circuit
    (``lane``: every lane of the wavefront walks it on its own value row) wrapped in the words that say where circuit c stands in
    the proof -- the segments of its evaluations among the proof's scalars, the groups of own rows it answers for, and per
    rotation set how many members belong to a circuit and every member's (target, stride) in the proof's point order
    (csrc/verify_terms.inc, at the VM_* words, states the layout).  ``lowered`` is the lane's: the same program as the single-circuit
    kernel runs.  ``inst_rows[c]``: the rows given of instance column c, the same for every circuit.  Needs no device."""

    def __init__(self, layout: ProofLayout, omega: int, inst_rows: Sequence[int]):
        if layout.lookup != "halo2":
            raise ValueError(f"{type(self).__name__}: the terms plans walk lookup=\"halo2\" layouts only (a logUp proof is verified by verify_proof)")
        m, one, cs = layout.circuits, layout.lane, layout.cs
        self.lane = TermsPlan(one, omega, inst_rows)
        per = layout.circuit_key
        own_kinds = ("advice", "lookup_a", "lookup_s", "perm_z", "lookup_z")
        adv_q, fix_q, _ = cs.queries()
        n_adv, n_mid = len(adv_q), len(fix_q) + 1 + layout.P
        n_perm, n_look = (3 * layout.nsets - 1 if layout.nsets else 0), 5 * layout.L
        segments = [(n_adv, 0, n_adv), (n_mid, m * n_adv, 0), (n_perm, m * n_adv + n_mid, n_perm),
                    (n_look, m * n_adv + n_mid + m * n_perm, n_look)]
        slot = 0
        for count, base, stride in segments:                      # the formula against the layout's own lists, circuit by circuit
            for i in range(count):
                key, rot = one.eval_keys[slot]
                for c in range(m):
                    want = (per(key, c) if key[0] in own_kinds else key, rot)
                    if layout.eval_keys[base + c * stride + i] != want:
                        raise AssertionError("MultiTermsPlan: the segments and the layout's evaluations disagree")
                slot += 1
        if slot != one.n_scalars:
            raise AssertionError("MultiTermsPlan: the segments do not fill a lane's evaluations")
        segments = [s for s in segments if s[0]]
        rows_of = {"advice": cs.num_advice, "lookup_a": 2 * layout.L, "lookup_s": 2 * layout.L, "perm_z": layout.nsets, "lookup_z": layout.L}
        groups, at = [], 0
        for count in (cs.num_advice, 2 * layout.L, layout.nsets, layout.L):
            if count:
                groups.append((at, count))
            at += m * count
        own_tail = at
        if layout.point_keys[own_tail] != ("random",):
            raise AssertionError("MultiTermsPlan: the proof's own rows do not begin where the circuits' end")
        member_words: List[int] = []
        for (rots, keys), (rots_m, keys_m) in zip(one.sets, layout.sets):
            mine = [key for key in keys if key[0] in own_kinds]
            if keys[:len(mine)] != mine or rots != rots_m or keys_m != [per(key, c) for c in range(m) for key in mine] + keys[len(mine):]:
                raise AssertionError("MultiTermsPlan: a rotation set is not circuit 0's members, circuit 1's, ..., then the proof's")
            member_words.append(len(mine))
            for key in keys:
                if key == ("h",):
                    member_words += [VT_T_H | layout.own_index[("h_piece", 0)], 0]
                elif key in layout.shared_index:
                    member_words += [VT_T_SHARED | layout.shared_index[key], 0]
                elif key[0] in own_kinds:
                    member_words += [layout.own_index[per(key, 0)], rows_of[key[0]]]
                else:
                    member_words += [layout.own_index[key], 0]
        if len(one.sets) != len(layout.sets):
            raise AssertionError("MultiTermsPlan: the later circuits open a rotation set of their own")
        off_seg = VM_HDR
        off_groups = off_seg + 3 * len(segments)
        off_members = off_groups + 2 * len(groups)
        off_lane = off_members + len(member_words)
        head = [m, len(layout.exprs), layout.n_scalars, layout.own_points, own_tail, len(segments), off_seg, len(groups), off_groups,
                off_members, off_lane, len(self.lane.words)]
        assert len(head) == VM_HDR
        body = head + [w for s in segments for w in s] + [w for g in groups for w in g] + member_words
        self.words = np.concatenate([np.array(body, dtype=np.uint32), self.lane.words])
        self.circuits, self.off_lane = m, off_lane
        self.lowered, self.n_columns, self.n_vals = self.lane.lowered, self.lane.n_columns, self.lane.n_vals
        self.inst_rows, self.inst_elems = self.lane.inst_rows, self.lane.inst_elems

    def instance_row(self, inst_cols) -> List[int]:
        """one CIRCUIT's instance values as its lane reads them (``TermsPlan.instance_row``)"""
        return self.lane.instance_row(inst_cols)


def proof_terms_ints(vk: VerifyingKey, instance, proof: bytes, layout: Optional[ProofLayout] = None):
    """The integer twin of the per-proof part, without r_b: (challenges, own scalars, shared scalars, points) of one proof in the device
    layout -- sum own[j] * points[j] + sum shared[i] * (shared point i) is the R of ``verify_opening`` and points[-1] its L.  Raises
    ``MalformedProof`` where ``verify_proof`` is False on structural grounds."""
    layout = layout or ProofLayout(vk.cs, vk.domain.k)
    inst_cols = _layout_instances(layout, instance)
    points, evals = read_proof_ints(layout, proof)
    ch = transcript_challenges(layout, _vk_digest(vk), inst_cols, proof, [p[1].to_bytes(32, "little") for p in points])   # y_bytes: "halo2" only
    own, shared, *left = terms_from_challenges(layout, vk.domain.omega, inst_cols, evals, ch)
    return (ch, own, shared, points, *left)


def proof_sums_ints(vk: VerifyingKey, instance, proof: bytes, layout: Optional[ProofLayout] = None, weight: int = 1):
    """The integer twin of the per-proof sums: (L, R) of one proof as (x, y) integers (None = the identity), L = weight * [h'] and
    R = weight * (sum own[j] * points[j] + sum shared[i] * (shared point i)), from ``proof_terms_ints`` and ``g1_msm``; the proof
    verifies exactly when s * L == R, whatever the weight in [1, r).  Needs no device.  ``MalformedProof`` as ``proof_terms_ints``."""
    layout = layout or ProofLayout(vk.cs, vk.domain.k)
    _, own, shared, points, *left = proof_terms_ints(vk, instance, proof, layout)
    w = weight % R
    scalars = [w * v % R for v in list(own) + list(shared)]
    right = g1_msm(scalars, list(points) + shared_points(vk, layout))
    if left:                                                      # a "gwc" layout: L = sum_i u^i W_i over the proof's last q points
        return g1_msm([w * v % R for v in left[0]], list(points[len(points) - len(left[0]):])), right
    return g1_mul(w, points[-1]), right


def shared_points(vk: VerifyingKey, layout: ProofLayout):
    """the (x, y) points of ``layout.shared_keys``; None for a commitment that is the identity"""
    return [g1_words_to_int(c) for c in vk.fixed_commitments] + [g1_words_to_int(c) for c in vk.permutation_commitments] + [G1_GEN]


def derive_randomizer(seed, index: int) -> int:
    """r_b in [1, r) from (seed, index) by Blake2b: the same seed gives the same weights"""
    raw = seed if isinstance(seed, (bytes, bytearray)) else str(seed).encode()
    d = hashlib.blake2b(bytes(raw) + index.to_bytes(8, "little"), digest_size=64, person=b"Halo2-BatchRand").digest()
    return int.from_bytes(d, "little") % (R - 1) + 1

