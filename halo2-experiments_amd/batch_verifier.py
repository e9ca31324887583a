"""``halo2_proofs::plonk::BatchVerifier`` (``plonk/verifier/batch.rs``; RECALLED from upstream, not pinned against its source: the idea is
mirrored, not the bytes): many proofs of ONE verifying key are checked with ONE pairing.  Proof b leaves two G1 points (h2_b, R_b) with
e(h2_b, [s]G2) = e(R_b, G2) -- what ``shplonk.verify_opening`` returns; with a random weight r_b per proof the batch checks

    e(sum_b r_b h2_b, [s]G2) = e(sum_b r_b R_b, G2)

which a batch holding a proof that fails passes with probability 1 / r.  Scope: proofs of one ``vk``, single-circuit
(``create_proof``) or, with ``circuits=m``, multi-circuit (``create_proof_multi``, every proof of the batch holding m circuits).

Where the work is done:

  - the device reads the proofs (``hm_verify_read_proofs_dev``, csrc/verify_read.inc): one lane per (proof, 32-byte slot) decompresses a
    point -- one square root -- or checks a scalar < r.  Every point position is known from the constraint system (``ProofLayout``),
    so all points are decompressed before any challenge exists;
  - the host runs the Blake2b transcript of every proof with ``hashlib``, in the order of ``verifier._verify`` / ``verify_opening``, on
    the proof's own x bytes and the y bytes the device returned: theta, beta, gamma, y, x, the multiopen's y', v, u -- one record per
    proof, uploaded with its weight r_b.  With ``transcript="device"`` one lane per proof runs it between the two kernels instead
    (``hm_verify_transcript_dev``, csrc/transcript.inc, walking ``ProofLayout.transcript_schedule``) and nothing travels;
  - the device computes, one lane per proof (``hm_verify_terms_dev``, csrc/verify_terms.inc, driven by a ``TermsPlan``), x^n, l0, l_last,
    l_active and the instance columns' evaluations at x, the numerator by the ``GraphEvaluator`` interpreter on the proof's value row,
    h(x), and per rotation set the multiopen's scalars: r_b x the scalar of every point (``terms_from_challenges`` is the integer twin;
    the rotation sets are taken symbolically on ROTATIONS, see ``ProofLayout``).  An instance column may have 64 rows at most;
  - the device sums: every proof's own points (advice, lookup, permutation, random, h pieces, [h]) lie in one array, behind them the
    points all proofs share (fixed and sigma commitments, the generator; their scalars are the column sums of a (B, shared) array,
    ``hm_verify_column_sum_dev``), behind them the [h'] of every proof; the array is registered once as a plain base set and the sums are
    MSMs over offsets into it, folded with ``hm_g1_sum``;
  - one ``pairing.pairing_check`` (or, with the trapdoor, s * L == R in G1).

``encoding="evm"`` (``ProofLayout``, ``BatchVerifier``, ``verify_proofs``) takes proofs in the second wire format, a Keccak transcript
over uncompressed big-endian points and scalars (``transcript`` states it): the read is ``hm_verify_read_proofs_evm_dev`` -- a curve
check in place of the square root, no y bytes --, the transcript absorbs the proof verbatim (``keccak256`` on the host,
``hm_verify_transcript_evm_dev`` on the device; csrc/keccak.inc), and everything behind the challenges is the same code.

``proof_terms_ints`` is the integer twin of the whole per-proof part, ``read_proof_ints`` of the read kernel; neither needs a device.

``circuits=m`` (``ProofLayout``, ``BatchVerifier``, ``verify_proofs``, ``verify_each``; 2 <= m <= 64) takes ``create_proof_multi``
proofs: the layout lists the points and evaluations in the order ``verifier._verify`` reads m circuits -- per-circuit keys are
(kind, index, circuit) --, read, transcript, column sums, MSMs, per-proof sums and pairing are the same calls on the longer lists,
and the terms are ``hm_verify_terms_multi_dev``: ONE WAVEFRONT per proof, lane c = circuit c, driven by a ``MultiTermsPlan``.  A
lane runs the single-circuit phases and the same numerator program on its own circuit's value row; the proof's numerator
sum_c y^(E (m - 1 - c)) N_c and the sum of coeff x r_eval meet by cross-lane moves inside the wave.  The twins take a list of m
instances.  With ``circuits=1`` everything is as before, and the old terms entry is the one called.  The one combination left out
is multi-circuit proofs in the "evm" encoding, which ``create_proof_multi`` does not write: ValueError.

A verdict PER PROOF (``verdicts``, ``failing(method="each")``, ``verify_each``) takes the other road behind the same preparation: one
workgroup per proof sums the proof's own pair (L_b, R_b) (``hm_verify_proof_sums_dev``, csrc/verify_sums.inc; ``proof_sums_ints`` is
the integer twin), and one pairing call checks e(L_b, [s]G2) = e(R_b, G2) for every proof at once.  The weights r_b stay in the scalar
arrays, so the per-proof sums equal ``_sums(handle, b, b + 1)`` as group elements; a verdict does not depend on r_b, which multiplies
both sides of the proof's own equation.

Two places where the symbolic form answers differently from ``verify_proof``, each of probability about 2^-254 for an honest or a
dishonest prover alike (x is a hash output): x = 0, where all rotations of x coincide, is reported as a failing proof; and h pieces whose
combination sum_i x^(n i) [h_i] is the identity are summed as they are, where ``verify_proof`` refuses to open the identity."""
from __future__ import annotations

import ctypes
import hashlib
import secrets
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, device_pairing, device_transcript, evaluation as ev
from .bn256 import FQ_MODULUS, FR_MODULUS, fr_array, g1_words
from .keygen import FR_DELTA, VerifyingKey
from .kzg import g2_from_bytes
from .pairing import G1_GEN, g1_msm, g1_mul, g1_neg, g1_on_curve
from .shplonk import g1_words_to_int
from .transcript import (PERSONAL, PREFIX_CHALLENGE, PREFIX_POINT, PREFIX_SCALAR, TranscriptError, check_encoding, g1_decompress_int,
                         g1_uncompressed_int, keccak256)
from .verifier import _instance_columns, _vk_digest, evaluate_expression, proof_length

R, P = FR_MODULUS, FQ_MODULUS
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
    when m = 1).  ``encoding="evm"`` with m > 1 raises ValueError."""

    def __init__(self, cs, k: int, encoding: str = "halo2", circuits: int = 1):
        self.encoding = check_encoding(encoding, "ProofLayout")
        m = int(circuits)
        if not 1 <= m <= MAX_CIRCUITS:
            raise ValueError(f"ProofLayout: need 1 <= circuits <= {MAX_CIRCUITS}, got {circuits!r}")
        if m > 1 and encoding == "evm":
            raise ValueError("ProofLayout: a multi-circuit proof has no \"evm\" encoding (create_proof_multi writes none)")
        self.circuits = m
        self.lane = self if m == 1 else ProofLayout(cs, k, encoding)       # what ONE circuit of the proof looks like
        self.cs, self.k, self.n = cs, k, 1 << k
        n = self.n
        adv_q, fix_q, _ = cs.queries()
        self.P, self.nsets, self.L = len(cs.equality), cs.permutation_sets(), len(cs.lookups)
        P_, nsets, L = self.P, self.nsets, self.L
        self.pieces = cs.degree() - 1
        self.last = -(cs.blinding_factors + 1)
        last = self.last
        M = range(m)
        per = (lambda key, c: key) if m == 1 else (lambda key, c: key + (c,))   # a per-circuit key: (kind, index, circuit) when m > 1
        pts = [per(("advice", i), c) for c in M for i in range(cs.num_advice)]
        for c in M:
            for j in range(L):
                pts += [per(("lookup_a", j), c), per(("lookup_s", j), c)]
        pts += [per(("perm_z", i), c) for c in M for i in range(nsets)] + [per(("lookup_z", j), c) for c in M for j in range(L)] + [("random",)]
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
        self.point_keys = pts + [("h1",), ("h2",)]
        self.eval_keys = evs
        self.eval_index = {}
        for at, key in enumerate(evs):
            self.eval_index.setdefault(key, at)
        self.n_points, self.own_points, self.n_scalars = len(self.point_keys), len(self.point_keys) - 1, len(evs)
        self.slots = (2 if encoding == "evm" else 1) * self.n_points + self.n_scalars
        if 32 * self.slots != proof_length(cs, m, encoding):
            raise AssertionError("ProofLayout: the slots do not add up to proof_length")
        if encoding == "evm":
            table = [e for i in range(self.points_before_evals) for e in (EVM_POINT | i, EVM_SKIP)] + list(range(self.n_scalars))
            table += [EVM_POINT | (self.n_points - 2), EVM_SKIP, EVM_POINT | EVM_TAIL | (self.n_points - 1), EVM_SKIP]
        else:
            table = [VR_POINT | i for i in range(self.points_before_evals)] + list(range(self.n_scalars))
            table += [VR_POINT | (self.n_points - 2), VR_POINT | VR_TAIL | (self.n_points - 1)]
        self.slot_table = np.array(table, dtype=np.uint32)
        self.point_slots = [s for s, e in enumerate(table) if e & VR_POINT]
        self.scalar_slots = [s for s, e in enumerate(table) if not e & (VR_POINT | (EVM_SKIP if encoding == "evm" else 0))]

        # the queries in the order verifier._verify lists them; ("h",) stands for sum_i x^(n i) [h_i]
        q = []
        for c in M:
            q += [(per(("advice", i), c), r % n) for i, r in adv_q]
            q += [qq for i in range(nsets) for qq in ((per(("perm_z", i), c), 0), (per(("perm_z", i), c), 1))]
            q += [(per(("perm_z", i), c), last % n) for i in reversed(range(nsets - 1))]
            for j in range(L):
                q += [(per(("lookup_z", j), c), 0), (per(("lookup_a", j), c), 0), (per(("lookup_s", j), c), 0),
                      (per(("lookup_a", j), c), (-1) % n), (per(("lookup_z", j), c), 1)]
        q += [(("fixed", i), r % n) for i, r in fix_q] + [(("sigma", j), 0) for j in range(P_)]
        q += [(("h",), 0), (("random",), 0)]
        self.queries = q
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
        for j, (ins, tabs) in enumerate(cs.lookups):
            b = self.lookup0 + 3 * j
            exprs += ev.lookup_expressions(ins, tabs, lambda r, b=b: F(b, r), lambda r, b=b: F(b + 1, r), lambda r, b=b: F(b + 2, r),
                                           F(self.i_l0), F(self.i_last), F(self.i_active))
        self.exprs = exprs

    def transcript_schedule(self) -> List[Tuple[int, int]]:
        """The (absorb a slots, squeeze s challenges) pairs of a proof's transcript over its slots in order, from the
        counts ``transcript_challenges`` uses: advice | theta | 2L | beta, gamma | sets + L + 1 | y | pieces | x | evaluations | y', v
        | [h] | u, and a last pair that absorbs [h'] behind the last challenge, as ``Blake2bRead`` does.  The counts are SLOTS: in an
        "evm" layout a point counts twice, and with ``circuits = m`` the per-circuit counts (advice, 2L, sets + L) are taken m times."""
        w, m = 2 if self.encoding == "evm" else 1, self.circuits
        pairs = [(w * m * self.cs.num_advice, 1), (w * m * 2 * self.L, 2), (w * (m * (self.nsets + self.L) + 1), 1), (w * self.pieces, 1),
                 (self.n_scalars, 2), (w, 1), (w, 0)]
        if sum(a for a, _ in pairs) != self.slots or sum(s for _, s in pairs) != len(RECORD):
            raise AssertionError("ProofLayout: the transcript's schedule does not cover the proof's slots and the eight challenges")
        return pairs


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
    return dict(zip(RECORD, out))


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
    points(m * 2 * layout.L)
    ch["beta"] = squeeze()
    ch["gamma"] = squeeze()
    points(m * (layout.nsets + layout.L) + 1)
    ch["y"] = squeeze()
    points(layout.pieces)
    ch["x"] = squeeze()
    for _ in range(layout.n_scalars):
        at = 32 * slot[0]
        st.update(PREFIX_SCALAR + proof[at:at + 32])
        slot[0] += 1
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
    insts = _per_circuit(layout, inst_cols)
    per = (lambda key, c: key) if m == 1 else (lambda key, c: key + (c,))
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


# ---- the plan of the terms kernel (csrc/verify_terms.inc) ---------------------------------------------------------------------------------
VT_NO_SLOT, VT_T_SHARED, VT_T_H = 0xFFFFFFFF, 1 << 31, 1 << 30
VT_MAX_VALS, VT_MAX_INST_ROWS, VT_MAX_SUPER, VT_MAX_T = 256, 64, 32, 8
RECORD = ("theta", "beta", "gamma", "y", "x", "y2", "v", "u")          # then r_b: the per-proof record of hm_verify_terms_dev
VERDICT_CHUNK = 1 << 16                                                # proofs per pairing call of ``verdicts``: the largest measured size


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
        if len(layout.super_rotations) > VT_MAX_SUPER or any(len(rots) > VT_MAX_T for rots, _ in layout.sets):
            raise ValueError("TermsPlan: more rotations than the kernel's workspace holds")

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
        for rot in layout.super_rotations:
            const(w(rot))
        inst_off = [sum(inst_rows[:c]) for c in range(cs.num_instance)]
        inst_words: List[int] = []
        for col, rot in inst_queries:
            inst_words += [inst_off[col], inst_rows[col], const(w(rot))]
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
        header = 24
        off_colmap = header
        off_inst = off_colmap + len(colmap)
        off_sets = off_inst + len(inst_words)
        off_consts = off_sets + len(set_words)
        head = [layout.k, layout.n_scalars, n_vals, len(lagrange_rows), len(inst_queries), len(layout.super_rotations), len(layout.sets),
                layout.pieces, layout.own_points, len(layout.shared_keys), n_rot, n_cols, off_colmap, off_inst, off_sets, sum(inst_rows),
                c_lagrange, c_rows, c_super, s_l0, s_inst, s_hx, len(consts), off_consts]
        assert len(head) == header
        body = head + colmap + inst_words + set_words + [limb for v in consts for limb in _internal_words(v)]
        self.words = np.array(body, dtype=np.uint32)
        self.inst_rows, self.inst_queries, self.n_vals, self.n_columns = inst_rows, inst_queries, n_vals, n_cols
        self.s_l0, self.s_inst, self.s_hx = s_l0, s_inst, s_hx
        self.inst_elems = max(sum(inst_rows), 1)                  # the instance array is never empty: one zero element at least

    def instance_row(self, inst_cols) -> List[int]:
        """one proof's instance values as the kernel reads them: column after column, every column padded to the plan's rows"""
        row: List[int] = []
        for values, rows in zip(inst_cols, self.inst_rows):
            if len(values) > rows:
                raise ValueError("TermsPlan: an instance column longer than the plan's")
            row += list(values) + [0] * (rows - len(values))
        return row or [0]


VM_HDR = 12                                                       # csrc/verify_terms.inc: the words of a multi plan's header


class MultiTermsPlan:
    """What ``hm_verify_terms_multi_dev`` needs beside the proofs of a multi-circuit layout: the ``TermsPlan`` of ONE circuit
    (``lane``: every lane of the wavefront walks it on its own value row) wrapped in the words that say where circuit c stands in
    the proof -- the segments of its evaluations among the proof's scalars, the groups of own rows it answers for, and per
    rotation set how many members belong to a circuit and every member's (target, stride) in the proof's point order
    (csrc/verify_terms.inc, second half, states the layout).  ``lowered`` is the lane's: the same program as the single-circuit
    kernel runs.  ``inst_rows[c]``: the rows given of instance column c, the same for every circuit.  Needs no device."""

    def __init__(self, layout: ProofLayout, omega: int, inst_rows: Sequence[int]):
        m, one, cs = layout.circuits, layout.lane, layout.cs
        self.lane = TermsPlan(one, omega, inst_rows)
        per = (lambda key, c: key) if m == 1 else (lambda key, c: key + (c,))
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
    own, shared = terms_from_challenges(layout, vk.domain.omega, inst_cols, evals, ch)
    return ch, own, shared, points


def proof_sums_ints(vk: VerifyingKey, instance, proof: bytes, layout: Optional[ProofLayout] = None, weight: int = 1):
    """The integer twin of the per-proof sums: (L, R) of one proof as (x, y) integers (None = the identity), L = weight * [h'] and
    R = weight * (sum own[j] * points[j] + sum shared[i] * (shared point i)), from ``proof_terms_ints`` and ``g1_msm``; the proof
    verifies exactly when s * L == R, whatever the weight in [1, r).  Needs no device.  ``MalformedProof`` as ``proof_terms_ints``."""
    layout = layout or ProofLayout(vk.cs, vk.domain.k)
    _, own, shared, points = proof_terms_ints(vk, instance, proof, layout)
    w = weight % R
    scalars = [w * v % R for v in list(own) + list(shared)]
    return g1_mul(w, points[-1]), g1_msm(scalars, list(points) + shared_points(vk, layout))


def shared_points(vk: VerifyingKey, layout: ProofLayout):
    """the (x, y) points of ``layout.shared_keys``; None for a commitment that is the identity"""
    return [g1_words_to_int(c) for c in vk.fixed_commitments] + [g1_words_to_int(c) for c in vk.permutation_commitments] + [G1_GEN]


def derive_randomizer(seed, index: int) -> int:
    """r_b in [1, r) from (seed, index) by Blake2b: the same seed gives the same weights"""
    raw = seed if isinstance(seed, (bytes, bytearray)) else str(seed).encode()
    d = hashlib.blake2b(bytes(raw) + index.to_bytes(8, "little"), digest_size=64, person=b"Halo2-BatchRand").digest()
    return int.from_bytes(d, "little") % (R - 1) + 1


# ---- the public object ---------------------------------------------------------------------------------------------------------------------
class BatchVerifier:
    """Collects proofs of one ``vk`` and checks them together (the module's docstring says how): single-circuit proofs, or with
    ``circuits=m`` (2 .. 64) ``create_proof_multi`` proofs of m circuits each -- ``add_proof(instances, proof)`` then takes the m
    instances of the proof, and everything below means per PROOF what it means for single-circuit proofs.

    ``params`` needs ``g2`` / ``s_g2`` only.  ``add_proof(instance, proof)`` takes what ``verify_proof`` takes and returns the proof's
    index.  ``finalize(trapdoor=None)`` is True when every added proof verifies -- one pairing check for the whole batch, or with the
    trapdoor s * L == R in G1; an empty batch is True.  A malformed proof (wrong length, a scalar >= r, an x >= p or off the curve, an
    all-zero point, x^n = 1) makes ``finalize`` False and is kept out of the sums; it raises nothing.  ``failing(trapdoor=None)`` names
    the proofs that do not verify: the malformed ones, and among the others those found by bisection -- each step sums a contiguous
    sub-range of the batch on the device and makes one check, O(f log B) checks for f failing proofs.  ``verdicts(trapdoor=None)`` gives
    one boolean per proof without bisection -- the per-proof sums in one launch, then one pairing check per proof, all in one call with
    ``pairing="device"`` -- and ``failing(method="each")`` names its False entries: the same lists, at a cost that does not grow with
    the number of failing proofs.  Every proof has a weight r_b in
    [1, r): from ``secrets`` when ``seed`` is None, else derived from (seed, index); ``randomizers`` shows them.
    An instance column may hold 64 rows at most (the terms kernel's
    limit; ``finalize`` raises ValueError beyond it).  ``close()`` gives the numerator's program back to the library.
    ``pairing="device"`` runs the pairing of every check on the GPU (``device_pairing``) instead of on host integers: the same
    booleans, and ``timings["pairing"]`` keeps its meaning.
    ``transcript="device"`` runs the Blake2b transcripts on the GPU too (``device_transcript``): read, transcript and terms are queued
    on one stream with no wait and no copy between them, and the flags of the batch are the one download.  The same booleans, sums and
    ``failing()`` lists.  ``timings`` keeps its keys, but ``read``, ``transcript`` and ``terms`` are then the wall times of QUEUEING
    each call -- the device's work surfaces in ``terms``, which ends with the download -- and only their sum means anything.
    ``encoding="evm"`` takes proofs in the other wire format (``create_proof(..., encoding="evm")``): the device reads uncompressed
    big-endian points with a curve check in place of the square root (``hm_verify_read_proofs_evm_dev``), the transcript is Keccak
    (``hm_verify_transcript_evm_dev`` with ``transcript="device"``), and terms, sums and pairing are the same calls as before;
    multi-circuit proofs in this encoding are the one combination left out (``circuits`` > 1 with "evm": ValueError)."""

    def __init__(self, params, vk: VerifyingKey, seed=None, pairing: str = "host", transcript: str = "host", encoding: str = "halo2",
                 circuits: int = 1):
        check_encoding(encoding, "BatchVerifier")
        if pairing not in device_pairing.MODES:
            raise ValueError(f"BatchVerifier: pairing must be one of {device_pairing.MODES}, got {pairing!r}")
        if transcript not in device_transcript.MODES:
            raise ValueError(f"BatchVerifier: transcript must be one of {device_transcript.MODES}, got {transcript!r}")
        self.params, self.vk, self.seed, self.pairing, self.transcript = params, vk, seed, pairing, transcript
        self.encoding = encoding
        self.layout = ProofLayout(vk.cs, vk.domain.k, encoding, circuits)   # ValueError: circuits outside 1 .. 64, or "evm" with several
        self.circuits = self.layout.circuits
        self._digest = _vk_digest(vk)
        self._shared = shared_points(vk, self.layout)
        # verify_proof opens no identity: with a queried fixed or sigma commitment that is one, no proof of this vk verifies
        self._vk_ok = all(self._shared[self.layout.shared_index[key]] is not None for key, _ in self.layout.queries
                          if key in self.layout.shared_index)
        self._proofs: List[bytes] = []
        self._instances: list = []
        self._rand: List[int] = []
        self._state = None
        self._plans: dict = {}                                   # instance shape -> TermsPlan (the program is the same for all)
        self._program = None                                     # the hm_graph_create program of the numerator, made on first use
        self.msm_calls = 0                                       # MSMs launched so far (tests, tools/batch_verify_time.py)
        self.sums_calls = 0                                      # per-proof sums launches so far (``proof_sums``)
        self.timings: dict = {}                                  # seconds of the last preparation and check, by phase

    def __len__(self) -> int:
        return len(self._proofs)

    @property
    def randomizers(self) -> Tuple[int, ...]:
        return tuple(self._rand)

    def add_proof(self, instance, proof: bytes) -> int:
        self._instances.append(_layout_instances(self.layout, instance))
        self._proofs.append(bytes(proof))
        i = len(self._proofs) - 1
        self._rand.append(secrets.randbelow(R - 1) + 1 if self.seed is None else derive_randomizer(self.seed, i))
        self._state = None
        return i

    def malformed(self) -> List[int]:
        """The indices the HOST pre-checks refuse, without a device: the integer twins of the read kernel and of the terms."""
        out = []
        for b, (inst, proof) in enumerate(zip(self._instances, self._proofs)):
            try:
                proof_terms_ints(self.vk, inst, proof, self.layout)
            except MalformedProof:
                out.append(b)
        return out

    # ---- the device part ------------------------------------------------------------------------------------------------------------------
    def _plan_for(self, inst_rows: Sequence[int]):
        key = tuple(inst_rows) if self.circuits == 1 else (tuple(inst_rows), self.circuits)
        if key not in self._plans:
            make = TermsPlan if self.circuits == 1 else MultiTermsPlan
            self._plans[key] = make(self.layout, self.vk.domain.omega, inst_rows)
        if self._program is None:
            self._program = ev.CompiledGraph(**self._plans[key].lowered)
        return self._plans[key]

    def close(self) -> None:
        """give the numerator's program back to the library (also done when the object is collected)"""
        if self._program is not None:
            program, self._program = self._program, None
            program.destroy()

    def __del__(self):
        try:
            self.close()
        except Exception:                                        # the library may be gone at interpreter shutdown
            pass

    def _circuit_instances(self) -> list:
        """the instance columns of every circuit of every proof, proof after proof: what the plan's rows are sized and filled from"""
        return list(self._instances) if self.circuits == 1 else [one for inst in self._instances for one in inst]

    def _preamble_instances(self) -> list:
        """per proof, the columns its transcript absorbs behind the key's digest: circuit 0's, then circuit 1's, ..."""
        return self._instances if self.circuits == 1 else [[col for one in inst for col in one] for inst in self._instances]

    def _queue_terms(self, plan, B: int, d_records, d_scalars, d_inst, d_bad, d_own, d_shared, d_h2_r, d_h2_l, stream) -> None:
        """the terms kernel on ``stream``: ``hm_verify_terms_dev``, or for multi-circuit proofs ``hm_verify_terms_multi_dev``"""
        lib = _lib.load()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        u32p = ctypes.POINTER(ctypes.c_uint32)
        head = (ctypes.c_uint64(self._program.handle), plan.words.ctypes.data_as(u32p), len(plan.words), plan.n_columns, 4, B)
        tail = (vp(d_records), vp(d_scalars), vp(d_inst), ctypes.cast(vp(d_bad), u32p), vp(d_own), vp(d_shared), vp(d_h2_r), vp(d_h2_l), stream)
        if self.circuits == 1:
            _lib.check(lib.hm_verify_terms_dev(*head, *tail))
        else:
            _lib.check(lib.hm_verify_terms_multi_dev(*head, self.circuits, *tail))

    def _queue_read(self, d_proofs, d_table, d_bases, d_tail, d_ybytes, d_scalars, d_bad, stream) -> None:
        """the read kernel of the layout's encoding on the current stream; ``d_ybytes`` is None for "evm", which has no such array"""
        lay, B, lib = self.layout, d_proofs.shape[0], _lib.load()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if self.encoding == "evm":
            _lib.check(lib.hm_verify_read_proofs_evm_dev(vp(d_proofs), B, ctypes.cast(vp(d_table), u32p), lay.slots, lay.own_points,
                                                         lay.n_scalars, vp(d_bases), vp(d_tail), vp(d_scalars), ctypes.cast(vp(d_bad), u32p),
                                                         stream))
        else:
            _lib.check(lib.hm_verify_read_proofs_dev(vp(d_proofs), B, ctypes.cast(vp(d_table), u32p), lay.slots, lay.own_points, lay.n_points,
                                                     lay.n_scalars, vp(d_bases), vp(d_tail), vp(d_ybytes), vp(d_scalars),
                                                     ctypes.cast(vp(d_bad), u32p), stream))

    def _prepare(self) -> dict:
        if self._state is not None:
            return self._state
        if self.transcript == "device":
            return self._prepare_on_device()
        import torch

        lay, B = self.layout, len(self._proofs)
        lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        t0 = time.perf_counter()
        bad = [len(p) != 32 * lay.slots for p in self._proofs] if self._vk_ok else [True] * B
        raw = np.zeros((B, 32 * lay.slots), dtype=np.uint8)
        for b, p in enumerate(self._proofs):
            if len(p) == 32 * lay.slots:
                raw[b] = np.frombuffer(p, dtype=np.uint8)
        n_shared, own = len(lay.shared_keys), lay.own_points
        d_proofs = torch.from_numpy(raw).to(dev)
        d_table = torch.from_numpy(lay.slot_table.view(np.int32)).to(dev)     # uploaded once per batch: a device table, not a kernel argument
        d_bases = torch.zeros((B * own + n_shared + B, 8), dtype=torch.int64, device=dev)
        evm = self.encoding == "evm"
        d_ybytes = None if evm else torch.zeros((B, lay.n_points, 32), dtype=torch.uint8, device=dev)
        d_scalars = torch.zeros((B, lay.n_scalars, 4), dtype=torch.int64, device=dev)
        d_bad = torch.zeros(B, dtype=torch.int32, device=dev)
        d_tail = d_bases[B * own + n_shared:]
        self._queue_read(d_proofs, d_table, d_bases, d_tail, d_ybytes, d_scalars, d_bad, stream)
        shared_words = np.stack([g1_words(p) for p in self._shared]).view(np.int64)
        d_bases[B * own:B * own + n_shared] = torch.from_numpy(shared_words).to(dev)
        ybytes = None if evm else d_ybytes.cpu().numpy()
        dev_bad = d_bad.cpu().numpy()
        t1 = time.perf_counter()

        # the transcripts: everything a proof's challenges depend on is on the host now
        zero_record = [0] * (len(RECORD) + 1)
        records = [zero_record] * B
        plan = self._plan_for([max((len(inst[c]) for inst in self._circuit_instances()), default=0) for c in range(self.vk.cs.num_instance)])
        t_plan = time.perf_counter() - t1
        inst_rows = [plan.instance_row(inst) for inst in self._circuit_instances()]
        for b in range(B):
            bad[b] = bad[b] or bool(dev_bad[b])
            if not bad[b]:
                ch = transcript_challenges(lay, self._digest, self._instances[b], self._proofs[b],
                                           None if evm else [bytes(row) for row in ybytes[b]])
                records[b] = [ch[name] for name in RECORD] + [self._rand[b]]
        t2 = time.perf_counter()
        up = lambda rows: torch.from_numpy(fr_array(rows).view(np.int64)).to(dev)
        d_records, d_inst = up(records), up(inst_rows)
        d_bad.copy_(torch.tensor([int(x) for x in bad], dtype=torch.int32))
        d_own = torch.empty((B * own, 4), dtype=torch.int64, device=dev)
        d_shared = torch.empty((B, n_shared, 4), dtype=torch.int64, device=dev)
        d_h2_r, d_h2_l = torch.empty((B, 4), dtype=torch.int64, device=dev), torch.empty((B, 4), dtype=torch.int64, device=dev)
        t3 = time.perf_counter()
        self._queue_terms(plan, B, d_records, d_scalars, d_inst, d_bad, d_own, d_shared, d_h2_r, d_h2_l, stream)
        bad = [bool(x) for x in d_bad.cpu().numpy()]              # the terms kernel flags x^n = 1 and its kin
        t4 = time.perf_counter()
        st = dict(B=B, bad=bad, d_bases=d_bases, d_scalars=d_scalars, d_own=d_own, d_shared=d_shared, d_h2_r=d_h2_r, d_h2_l=d_h2_l,
                  d_sum=torch.zeros((n_shared, 4), dtype=torch.int64, device=dev), ybytes=ybytes, d_bad=d_bad)
        self.timings = dict(read=t1 - t0, plan=t_plan, transcript=t2 - t1 - t_plan, upload=t3 - t2, terms=t4 - t3, msm=0.0, pairing=0.0,
                            sums=0.0, verdict_pairing=0.0)
        self._state = st
        return st

    def _prepare_on_device(self) -> dict:
        """``_prepare`` with the transcripts on the device: everything the three kernels read is uploaded first, then read, transcript
        and terms are queued on the current stream, and the flags are downloaded once, behind the terms."""
        import torch

        lay, B = self.layout, len(self._proofs)
        lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        u32p = ctypes.POINTER(ctypes.c_uint32)
        t0 = time.perf_counter()
        bad = [len(p) != 32 * lay.slots for p in self._proofs] if self._vk_ok else [True] * B
        raw = np.zeros((B, 32 * lay.slots), dtype=np.uint8)
        for b, p in enumerate(self._proofs):
            if len(p) == 32 * lay.slots:
                raw[b] = np.frombuffer(p, dtype=np.uint8)
        n_shared, own = len(lay.shared_keys), lay.own_points
        t1 = time.perf_counter()
        plan = self._plan_for([max((len(inst[c]) for inst in self._circuit_instances()), default=0) for c in range(self.vk.cs.num_instance)])
        t2 = time.perf_counter()
        up = lambda rows: torch.from_numpy(fr_array(rows).view(np.int64)).to(dev)
        records = np.zeros((B, len(RECORD) + 1, 4), dtype=np.uint64)          # the challenges are the device's; r_b stands behind them
        records[:, len(RECORD)] = fr_array(self._rand)
        d_records, d_inst = torch.from_numpy(records.view(np.int64)).to(dev), up([plan.instance_row(inst) for inst in self._circuit_instances()])
        preamble = device_transcript.upload_preamble(self._digest, self._preamble_instances(), dev, self.encoding)
        d_proofs = torch.from_numpy(raw).to(dev)
        d_table = torch.from_numpy(lay.slot_table.view(np.int32)).to(dev)
        d_bad = torch.tensor([int(x) for x in bad], dtype=torch.int32, device=dev)   # the read kernel only ever sets a flag
        d_bases = torch.zeros((B * own + n_shared + B, 8), dtype=torch.int64, device=dev)
        shared_words = np.stack([g1_words(p) for p in self._shared]).view(np.int64)
        d_bases[B * own:B * own + n_shared] = torch.from_numpy(shared_words).to(dev)
        d_ybytes = None if self.encoding == "evm" else torch.zeros((B, lay.n_points, 32), dtype=torch.uint8, device=dev)
        d_scalars = torch.zeros((B, lay.n_scalars, 4), dtype=torch.int64, device=dev)
        d_own = torch.empty((B * own, 4), dtype=torch.int64, device=dev)
        d_shared = torch.empty((B, n_shared, 4), dtype=torch.int64, device=dev)
        d_h2_r, d_h2_l = torch.empty((B, 4), dtype=torch.int64, device=dev), torch.empty((B, 4), dtype=torch.int64, device=dev)
        d_tail = d_bases[B * own + n_shared:]
        t3 = time.perf_counter()
        self._queue_read(d_proofs, d_table, d_bases, d_tail, d_ybytes, d_scalars, d_bad, stream)
        t4 = time.perf_counter()
        device_transcript.challenges(lay, self._digest, self._preamble_instances(), d_proofs, d_ybytes, d_bad, d_records, preamble=preamble, d_table=d_table)
        t5 = time.perf_counter()
        self._queue_terms(plan, B, d_records, d_scalars, d_inst, d_bad, d_own, d_shared, d_h2_r, d_h2_l, stream)
        bad = [bool(x) for x in d_bad.cpu().numpy()]              # the one download: what the three kernels flagged
        t6 = time.perf_counter()
        st = dict(B=B, bad=bad, d_bases=d_bases, d_scalars=d_scalars, d_own=d_own, d_shared=d_shared, d_h2_r=d_h2_r, d_h2_l=d_h2_l,
                  d_sum=torch.zeros((n_shared, 4), dtype=torch.int64, device=dev), d_ybytes=d_ybytes, d_bad=d_bad,
                  d_proofs=d_proofs, d_table=d_table, d_records=d_records, preamble=preamble,   # what the transcript call took (tools/batch_verify_time.py)
                  d_inst=d_inst, plan=plan)                                                     # ... and the terms call
        self.timings = dict(read=t1 - t0 + t4 - t3, plan=t2 - t1, transcript=t5 - t4, upload=t3 - t2, terms=t6 - t5, msm=0.0, pairing=0.0,
                            sums=0.0, verdict_pairing=0.0)
        self._state = st
        return st

    def column_sum(self, lo: int, hi: int):
        """sum of rows [lo, hi) of the (B, shared) array of r_b x shared scalars, on the device: a (shared, 4) tensor"""
        import torch

        st = self._prepare()
        out = st["d_sum"]
        _lib.check(_lib.load().hm_verify_column_sum_dev(ctypes.c_void_p(st["d_shared"].data_ptr()), st["B"], len(self.layout.shared_keys), lo, hi,
                                                        ctypes.c_void_p(out.data_ptr()),
                                                        ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))
        return out

    def _sums(self, handle, lo: int, hi: int):
        """(L, R) of the proofs [lo, hi) as (x, y) integers: four MSMs over offsets into the registered array, folded on the host"""
        from .arithmetic import best_multiexp

        st, own, n_shared = self._state, self.layout.own_points, len(self.layout.shared_keys)
        B = st["B"]
        parts = [best_multiexp(st["d_own"][lo * own:hi * own], handle, offset=lo * own),
                 best_multiexp(self.column_sum(lo, hi), handle, offset=B * own),
                 best_multiexp(st["d_h2_r"][lo:hi], handle, offset=B * own + n_shared + lo)]
        left = best_multiexp(st["d_h2_l"][lo:hi], handle, offset=B * own + n_shared + lo)
        self.msm_calls += 4
        right = np.zeros(12, dtype=np.uint64)
        stacked = np.ascontiguousarray(np.stack(parts))
        u64p = ctypes.POINTER(ctypes.c_uint64)
        _lib.check(_lib.load().hm_g1_sum(stacked.ctypes.data_as(u64p), len(parts), right.ctypes.data_as(u64p)))
        return g1_words_to_int(left), g1_words_to_int(right)

    def _check(self, handle, lo: int, hi: int, trapdoor) -> bool:
        """the one check of the well-formed proofs in [lo, hi) (malformed ones hold zero rows); vacuously True when there are none"""
        if all(self._state["bad"][lo:hi]):
            return True
        t0 = time.perf_counter()
        left, right = self._sums(handle, lo, hi)
        t1 = time.perf_counter()
        if trapdoor is not None:
            ok = g1_mul(trapdoor, left) == right
        else:
            g2, s_g2 = g2_from_bytes(self.params.g2), g2_from_bytes(self.params.s_g2)
            ok = g1_on_curve(left) and device_pairing.check([(left, s_g2), (g1_neg(right), g2)], self.pairing)
        self.timings["msm"] += t1 - t0
        self.timings["pairing"] += time.perf_counter() - t1
        return ok

    def _with_bases(self, fn):
        from .arithmetic import register_bases, release_bases

        st = self._prepare()
        if all(st["bad"]):
            return fn(None)
        handle = register_bases(st["d_bases"], plain=True)
        try:
            return fn(handle)
        finally:
            release_bases(handle)

    def finalize(self, trapdoor: int = None) -> bool:
        if not self._proofs:
            return True
        st = self._prepare()
        if any(st["bad"]):
            return False
        return self._with_bases(lambda handle: self._check(handle, 0, st["B"], trapdoor))

    # ---- a verdict per proof: the per-proof sums, then one pairing check per proof in one call ---------------------------------------------
    def proof_sums(self):
        """The (B, 2, 8) device tensor of ``hm_verify_proof_sums_dev``: row [b, 0] is L_b = r_b [h']_b, row [b, 1] is -R_b, affine
        Montgomery words, (0, 0) for the identity; two zero rows for a malformed proof.  One launch for the whole batch, made once per
        prepared state (``sums_calls`` counts the launches); nothing is launched when every proof is malformed, and an empty
        batch gives an empty (0, 2, 8) tensor; ``msm_calls`` is not touched.  ``timings["sums"]`` is the wall time of QUEUEING the call: the device's work surfaces in the download behind it."""
        import torch

        if not self._proofs:                                     # nothing to prepare: an empty (0, 2, 8) tensor, no launch
            return torch.zeros((0, 2, 8), dtype=torch.int64, device="cuda" if torch.cuda.is_available() else "cpu")
        st = self._prepare()
        if "d_pairs" in st:
            return st["d_pairs"]
        lay, B = self.layout, st["B"]
        dev = st["d_bases"].device
        d_pairs = torch.zeros((B, 2, 8), dtype=torch.int64, device=dev)
        if not all(st["bad"]):
            t0 = time.perf_counter()
            vp = lambda t: ctypes.c_void_p(t.data_ptr())
            _lib.check(_lib.load().hm_verify_proof_sums_dev(vp(st["d_bases"]), B, lay.own_points, len(lay.shared_keys), vp(st["d_own"]),
                                                            vp(st["d_shared"]), vp(st["d_h2_r"]), vp(st["d_h2_l"]),
                                                            ctypes.cast(vp(st["d_bad"]), ctypes.POINTER(ctypes.c_uint32)), vp(d_pairs),
                                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            self.sums_calls += 1
            self.timings["sums"] += time.perf_counter() - t0
        st["d_pairs"] = d_pairs
        return d_pairs

    def verdicts(self, trapdoor: int = None) -> List[bool]:
        """One boolean per added proof, in order: does THIS proof verify -- what ``verify_proof`` answers, without bisection.  A
        malformed proof is False from its flag (its rows are identities, which a pairing would pass).  For the others the per-proof
        sums (``proof_sums``) are checked per proof: with ``pairing="device"`` as ONE ``device_pairing.run_device`` call over all of
        them (per 65 536 proofs, the largest measured size), two pairs per check -- (L_b, [s]G2), (-R_b, G2) --, the G2 array filled on
        the device and the status words the one download; with ``pairing="host"`` the points are downloaded and
        ``pairing.pairing_check`` runs per proof, which is correct but costs about 36 ms PER PROOF on host integers; with the trapdoor
        s * L_b == R_b on host integers.  An empty batch gives [].  ``timings["verdict_pairing"]`` is the wall time of the checks,
        the download included."""
        import torch

        if not self._proofs:
            return []
        st = self._prepare()
        B = st["B"]
        good = [b for b in range(B) if not st["bad"][b]]
        out = [False] * B
        if not good:
            return out
        d_pairs = self.proof_sums()
        t0 = time.perf_counter()
        if trapdoor is None and self.pairing == "device":
            dev = d_pairs.device
            g2_words = np.frombuffer(bytes(self.params.s_g2) + bytes(self.params.g2), dtype=np.int64).reshape(2, 16)
            d_g2_pair = torch.from_numpy(g2_words.copy()).to(dev)
            d_good = None if len(good) == B else torch.tensor(good, dtype=torch.int64, device=dev)
            status = []
            for lo in range(0, len(good), VERDICT_CHUNK):
                n = min(VERDICT_CHUNK, len(good) - lo)
                rows = d_pairs[lo:lo + n] if d_good is None else d_pairs.index_select(0, d_good[lo:lo + n])
                d_off = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=dev)
                status.append(device_pairing.run_device(rows.reshape(2 * n, 8), d_g2_pair.repeat(n, 1), d_off, n))
            for b, s in zip(good, torch.cat(status).cpu().numpy()):
                out[b] = int(s) == 1
        else:
            rows = d_pairs.cpu().numpy().view(np.uint64)
            if trapdoor is None:
                from .pairing import pairing_check

                g2, s_g2 = g2_from_bytes(self.params.g2), g2_from_bytes(self.params.s_g2)
            for b in good:
                left, neg_right = g1_words_to_int(rows[b, 0]), g1_words_to_int(rows[b, 1])
                if trapdoor is not None:
                    out[b] = g1_mul(trapdoor, left) == g1_neg(neg_right)
                else:
                    out[b] = g1_on_curve(left) and pairing_check([(left, s_g2), (neg_right, g2)])
        self.timings["verdict_pairing"] += time.perf_counter() - t0
        return out

    def failing(self, trapdoor: int = None, method: str = "bisect") -> List[int]:
        """The indices of the proofs that do not verify.  ``method="bisect"`` (the default): the malformed ones, and the others by
        bisection, O(f log B) checks of four MSMs and one pairing each -- the cheaper way for a batch expected to be clean.
        ``method="each"``: the indices where ``verdicts()`` is False, one sums launch and one pairing call whatever f is."""
        if method not in ("bisect", "each"):
            raise ValueError(f"BatchVerifier.failing: method must be 'bisect' or 'each', got {method!r}")
        if method == "each":
            return [b for b, ok in enumerate(self.verdicts(trapdoor)) if not ok]
        if not self._proofs:
            return []
        st = self._prepare()
        out = [b for b, bad in enumerate(st["bad"]) if bad]

        def bisect(handle, lo: int, hi: int, known_failing: bool) -> None:
            if not known_failing and self._check(handle, lo, hi, trapdoor):
                return
            if hi - lo == 1:
                out.append(lo)
                return
            mid = (lo + hi) // 2
            left_ok = self._check(handle, lo, mid, trapdoor)
            if not left_ok:
                bisect(handle, lo, mid, True)
            bisect(handle, mid, hi, left_ok)                        # the range failed: with a passing left half the right half fails

        self._with_bases(lambda handle: bisect(handle, 0, st["B"], False))
        return sorted(out)


def verify_proofs(params, vk: VerifyingKey, instances, proofs, seed=None, trapdoor: int = None, pairing: str = "host",
                  transcript: str = "host", encoding: str = "halo2", circuits: int = 1) -> bool:
    """True when every ``proofs[i]`` is a valid single-circuit proof of ``vk`` for ``instances[i]``: one ``BatchVerifier``, one check
    (``pairing`` / ``transcript``: where that check's pairing and the proofs' transcripts run, ``encoding``: the proofs' wire format,
    ``circuits=m``: every proof is a ``create_proof_multi`` proof and ``instances[i]`` its m instances, as on ``BatchVerifier``)"""
    check_encoding(encoding, "verify_proofs")
    instances, proofs = list(instances), list(proofs)
    if len(instances) != len(proofs):
        raise ValueError("verify_proofs: one instance per proof")
    bv = BatchVerifier(params, vk, seed, pairing=pairing, transcript=transcript, encoding=encoding, circuits=circuits)
    for instance, proof in zip(instances, proofs):
        bv.add_proof(instance, proof)
    return bv.finalize(trapdoor)


def verify_each(params, vk: VerifyingKey, instances, proofs, seed=None, trapdoor: int = None, pairing: str = "host",
                transcript: str = "host", encoding: str = "halo2", circuits: int = 1) -> List[bool]:
    """[is ``proofs[i]`` a valid single-circuit proof of ``vk`` for ``instances[i]``]: one ``BatchVerifier``, its ``verdicts`` -- the
    per-proof sums in one launch and, with ``pairing="device"``, one pairing call for all proofs (keywords as on ``verify_proofs``)"""
    check_encoding(encoding, "verify_each")
    instances, proofs = list(instances), list(proofs)
    if len(instances) != len(proofs):
        raise ValueError("verify_each: one instance per proof")
    bv = BatchVerifier(params, vk, seed, pairing=pairing, transcript=transcript, encoding=encoding, circuits=circuits)
    for instance, proof in zip(instances, proofs):
        bv.add_proof(instance, proof)
    return bv.verdicts(trapdoor)
