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

Everything that needs no device -- ``ProofLayout``, the integer twins (``proof_terms_ints`` of the whole per-proof part,
``read_proof_ints`` of the read kernel, ...), the terms plans, the constants -- lives in ``proof_layout``, which also states the two
places where this symbolic form answers differently from ``verify_proof``; the names are imported here, so ``batch_verifier.<name>``
still finds them.

``circuits=m`` (``ProofLayout``, ``BatchVerifier``, ``verify_proofs``, ``verify_each``; 2 <= m <= 64) takes ``create_proof_multi``
proofs: read, transcript, column sums, MSMs, per-proof sums and pairing are the same calls on the layout's longer lists,
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

``multiopen="gwc"`` (``ProofLayout``, ``BatchVerifier``, ``verify_proofs``; single-circuit, both encodings, all four ``pairing`` x
``transcript`` modes) takes proofs that end in the GWC multiopen (``gwc``): q witness points W_i behind the evaluations, all of them own
points, seven challenges.  Read and transcript are the same kernels on the layout's table and schedule; the terms are
``hm_verify_terms_gwc_dev`` driven by a ``GwcTermsPlan`` -- the same phase a and numerator, the point groups' phase b --, which also
leaves r_b u_b^i in ``d_w_left``.  The check is e(sum_b sum_i r_b u_b^i W_bi, [s]G2) = e(sum_b R_b, G2): the left sum ONE MSM of the W
points (copied behind the shared points, where SHPLONK's tail points stand) against ``d_w_left``, the right sum the own-points MSM
and the shared column sums -- three MSMs per check.  The gap left: a verdict per proof (``verdicts``, ``failing(method="each")``,
``verify_each``, ``proof_sums``) raises ValueError, since the per-proof sums kernel writes L_b from ONE tail point; and
multi-circuit GWC batches (``circuits`` > 1: ValueError)."""
from __future__ import annotations

import ctypes
import secrets
import time
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, device_pairing, device_transcript, evaluation as ev
from .bn256 import fr_array, g1_words
from .keygen import VerifyingKey
from .kzg import g2_from_bytes
from .pairing import g1_mul, g1_neg, g1_on_curve
from .proof_layout import (EVM_POINT, EVM_SKIP, EVM_TAIL, GWC_RECORD, MAX_CIRCUITS, RECORD, VM_HDR, VR_POINT, VR_TAIL,  # noqa: F401
                           VT_MAX_INST_ROWS, VT_MAX_SUPER, VT_MAX_T, VT_MAX_VALS, VT_NO_SLOT, VT_T_H, VT_T_SHARED, GwcTermsPlan, MalformedProof,
                           MultiTermsPlan, ProofLayout, R, TermsPlan, _instance_columns, _layout_instances, derive_randomizer, proof_sums_ints, proof_terms_ints,
                           read_proof_ints, shared_points, terms_from_challenges, transcript_challenges)
from .shplonk import g1_words_to_int
from .transcript import check_encoding, check_lookup, check_multiopen
from .verifier import _vk_digest

VERDICT_CHUNK = 1 << 16                                                # proofs per pairing call of ``verdicts``: the largest measured size


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
    ``failing()`` lists.  ``timings`` (seconds, one key set in both modes): with the host's transcripts ``read`` is staging the
    proofs, their way to the device, the read kernel and the download of the y bytes and flags, ``plan`` building the terms plan,
    ``transcript`` the hashing, ``upload`` the records' way to the device, ``terms`` the terms kernel and the download of its flags.
    With ``transcript="device"`` ``upload`` is every allocation and upload, and ``read``, ``transcript`` and ``terms`` are the wall
    times of QUEUEING each call -- the device's work surfaces in ``terms``, which ends with the download -- so only their sum means
    anything.  ``msm`` / ``pairing`` and ``sums`` / ``verdict_pairing`` are added to by the checks behind the preparation.
    ``encoding="evm"`` takes proofs in the other wire format (``create_proof(..., encoding="evm")``): the device reads uncompressed
    big-endian points with a curve check in place of the square root (``hm_verify_read_proofs_evm_dev``), the transcript is Keccak
    (``hm_verify_transcript_evm_dev`` with ``transcript="device"``), and terms, sums and pairing are the same calls as before;
    multi-circuit proofs in this encoding are the one combination left out (``circuits`` > 1 with "evm": ValueError)."""

    def __init__(self, params, vk: VerifyingKey, seed=None, pairing: str = "host", transcript: str = "host", encoding: str = "halo2",
                 circuits: int = 1, multiopen: str = "shplonk", lookup: str = "halo2"):
        check_encoding(encoding, "BatchVerifier")
        check_multiopen(multiopen, "BatchVerifier")
        if check_lookup(lookup, "BatchVerifier") != "halo2":       # also the answer of verify_proofs and verify_each, which build one
            raise ValueError("BatchVerifier: lookup=\"logup\" proofs are not batch-verified (verify_proof reads them; the terms plans and "
                             "kernels walk the permutation-based lookup argument only)")
        if multiopen == "gwc" and circuits != 1:
            raise ValueError("BatchVerifier: multi-circuit batches with the \"gwc\" multiopen are not supported (circuits > 1)")
        if pairing not in device_pairing.MODES:
            raise ValueError(f"BatchVerifier: pairing must be one of {device_pairing.MODES}, got {pairing!r}")
        if transcript not in device_transcript.MODES:
            raise ValueError(f"BatchVerifier: transcript must be one of {device_transcript.MODES}, got {transcript!r}")
        self.params, self.vk, self.seed, self.pairing, self.transcript = params, vk, seed, pairing, transcript
        self.encoding, self.multiopen = encoding, multiopen
        self.layout = ProofLayout(vk.cs, vk.domain.k, encoding, circuits, multiopen)   # ValueError: circuits outside 1 .. 64, or "evm" with several
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
            make = GwcTermsPlan if self.multiopen == "gwc" else TermsPlan if self.circuits == 1 else MultiTermsPlan
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
        """the terms kernel on ``stream``: ``hm_verify_terms_dev``, for multi-circuit proofs ``hm_verify_terms_multi_dev``, for GWC
        proofs ``hm_verify_terms_gwc_dev`` (``d_h2_r`` is then ``d_w_left`` and ``d_h2_l`` None)"""
        lib = _lib.load()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        u32p = ctypes.POINTER(ctypes.c_uint32)
        head = (ctypes.c_uint64(self._program.handle), plan.words.ctypes.data_as(u32p), len(plan.words), plan.n_columns, 4, B)
        if self.multiopen == "gwc":
            _lib.check(lib.hm_verify_terms_gwc_dev(*head, vp(d_records), vp(d_scalars), vp(d_inst), ctypes.cast(vp(d_bad), u32p), vp(d_own),
                                                   vp(d_shared), vp(d_h2_r), stream))
            return
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
        """The prepared state of the batch, made once per set of proofs: stage (raw proofs, host flags, plan, instance rows), allocate
        and upload, queue the read, the challenges -- the ONE place the two ``transcript`` modes differ --, queue the terms, download
        the flags.  One key set in both modes: B, bad, plan, every ``d_*`` array the three kernels read or wrote, ``ybytes`` (host
        mode: the y bytes the read returned, else None) and ``preamble`` (device mode: what the transcript kernel absorbed first,
        else None).  Device mode queues read, transcript and terms with no wait between them and downloads once, behind the terms."""
        if self._state is not None:
            return self._state
        import torch

        lay, B, on_device, evm = self.layout, len(self._proofs), self.transcript == "device", self.encoding == "evm"
        dev = torch.device("cuda", torch.cuda.current_device())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_shared, own, n_ch = len(lay.shared_keys), lay.own_points, len(lay.record)
        gwc = self.multiopen == "gwc"
        q = len(lay.groups) if gwc else 1                         # points per proof behind the shared ones: the W_i, or the tail [h']
        up = lambda words: torch.from_numpy(words.view(np.int64)).to(dev)
        new = lambda fill, *shape, dtype=torch.int64: fill(shape, dtype=dtype, device=dev)
        t = [time.perf_counter()]
        lap = lambda: t.append(time.perf_counter())
        bad = [len(p) != 32 * lay.slots for p in self._proofs] if self._vk_ok else [True] * B
        raw = np.zeros((B, 32 * lay.slots), dtype=np.uint8)
        for b, p in enumerate(self._proofs):
            if len(p) == 32 * lay.slots:
                raw[b] = np.frombuffer(p, dtype=np.uint8)
        lap()                                                     # t[1]: staged
        plan = self._plan_for([max((len(inst[c]) for inst in self._circuit_instances()), default=0) for c in range(self.vk.cs.num_instance)])
        lap()                                                     # t[2]: planned
        records = np.zeros((B, n_ch + 1, 4), dtype=np.uint64)     # a proof's challenges (zero while it has none), r_b behind them
        records[:, n_ch] = fr_array(self._rand)
        # the order of the allocations is kept on purpose: where the caching allocator places the arrays a kernel reads has moved the
        # multi-circuit terms kernel by 0.7 % (profiles/r19_batch_verify_refactor_ab.json)
        st = dict(B=B, plan=plan, ybytes=None,
                  d_records=up(records) if on_device else None,
                  d_inst=up(fr_array([plan.instance_row(inst) for inst in self._circuit_instances()])),
                  preamble=device_transcript.upload_preamble(self._digest, self._preamble_instances(), dev, self.encoding) if on_device else None,
                  d_proofs=torch.from_numpy(raw).to(dev),
                  d_table=torch.from_numpy(lay.slot_table.view(np.int32)).to(dev),   # a device table, not a kernel argument
                  d_bad=torch.tensor([int(x) for x in bad], dtype=torch.int32, device=dev),   # the kernels only ever set a flag
                  d_bases=new(torch.zeros, B * own + n_shared + B * q, 8))
        st["d_bases"][B * own:B * own + n_shared] = up(np.stack([g1_words(p) for p in self._shared]))
        st.update(d_ybytes=None if evm else new(torch.zeros, B, lay.n_points, 32, dtype=torch.uint8),
                  d_scalars=new(torch.zeros, B, lay.n_scalars, 4), d_own=new(torch.empty, B * own, 4),
                  d_shared=new(torch.empty, B, n_shared, 4), d_h2_r=None if gwc else new(torch.empty, B, 4),
                  d_h2_l=None if gwc else new(torch.empty, B, 4), d_sum=new(torch.zeros, n_shared, 4))
        if gwc:                                                   # the one key a "gwc" state has beyond the others: r_b u^i per witness
            st["d_w_left"] = new(torch.empty, B, q, 4)
        lap()                                                     # t[3]: allocated and uploaded
        self._queue_read(st["d_proofs"], st["d_table"], st["d_bases"], st["d_bases"][B * own + n_shared:], st["d_ybytes"], st["d_scalars"],
                         st["d_bad"], stream)
        if gwc:                                                   # no slot has a tail bit: the region behind the shared points was the tail
            # buffer nothing is routed to; now it takes the W points, proof after proof, for the left sum's one MSM
            st["d_bases"][B * own + n_shared:] = st["d_bases"][:B * own].view(B, own, 8)[:, own - q:].reshape(B * q, 8)
        if not on_device:                                         # everything a proof's challenges depend on comes to the host
            st["ybytes"] = None if evm else st["d_ybytes"].cpu().numpy()
            flagged = st["d_bad"].cpu().numpy()
        lap()                                                     # t[4]: read
        if on_device:
            device_transcript.challenges(lay, self._digest, self._preamble_instances(), st["d_proofs"], st["d_ybytes"], st["d_bad"],
                                         st["d_records"], preamble=st["preamble"], d_table=st["d_table"])
        else:
            for b in range(B):
                if not flagged[b]:
                    ch = transcript_challenges(lay, self._digest, self._instances[b], self._proofs[b],
                                               None if evm else [bytes(row) for row in st["ybytes"][b]])
                    records[b, :n_ch] = fr_array([ch[name] for name in lay.record])
        lap()                                                     # t[5]: the challenges
        if not on_device:
            st["d_records"] = up(records)
        lap()                                                     # t[6]: the host's records uploaded
        self._queue_terms(plan, B, st["d_records"], st["d_scalars"], st["d_inst"], st["d_bad"], st["d_own"], st["d_shared"],
                          st["d_w_left"] if gwc else st["d_h2_r"], st["d_h2_l"], stream)
        st["bad"] = [bool(x) for x in st["d_bad"].cpu().numpy()]  # device mode's one download: what the three kernels flagged
        lap()                                                     # t[7]: terms
        read, upload = t[1] - t[0] + t[4] - t[3], t[3] - t[2] + t[6] - t[5]
        if not on_device:                                         # the host road counts the proofs' way to the device as part of the read
            read, upload = read + t[3] - t[2], t[6] - t[5]
        self.timings = dict(read=read, plan=t[2] - t[1], transcript=t[5] - t[4], upload=upload, terms=t[7] - t[6], msm=0.0, pairing=0.0,
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
        """(L, R) of the proofs [lo, hi) as (x, y) integers: four MSMs (three under "gwc") over offsets into the registered array,
        folded on the host"""
        from .arithmetic import best_multiexp

        st, own, n_shared = self._state, self.layout.own_points, len(self.layout.shared_keys)
        B = st["B"]
        parts = [best_multiexp(st["d_own"][lo * own:hi * own], handle, offset=lo * own),
                 best_multiexp(self.column_sum(lo, hi), handle, offset=B * own)]
        if self.multiopen == "gwc":                                # three MSMs: the W rows of d_own carry r_b u^i z_i, d_w_left r_b u^i
            q = len(self.layout.groups)
            left = best_multiexp(st["d_w_left"][lo:hi].reshape((hi - lo) * q, 4), handle, offset=B * own + n_shared + lo * q)
            self.msm_calls += 3
        else:
            parts.append(best_multiexp(st["d_h2_r"][lo:hi], handle, offset=B * own + n_shared + lo))
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

        self._no_verdicts("proof_sums")
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

    def _no_verdicts(self, who: str) -> None:
        """the per-proof road is SHPLONK's: the sums kernel writes L_b from one tail point, a GWC proof has q witness points"""
        if self.multiopen == "gwc":
            raise ValueError(f"BatchVerifier.{who}: per-proof verdicts are not available with the \"gwc\" multiopen "
                             "(finalize and failing() by bisection are)")

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

        self._no_verdicts("verdicts")
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
            self._no_verdicts("failing(method=\"each\")")
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


def _batch_of(who: str, params, vk: VerifyingKey, instances, proofs, seed, **modes) -> BatchVerifier:
    """the ``BatchVerifier`` behind ``verify_proofs`` and ``verify_each``: one proof added per (instance, proof)"""
    check_encoding(modes["encoding"], who)
    check_multiopen(modes.get("multiopen", "shplonk"), who)
    instances, proofs = list(instances), list(proofs)
    if len(instances) != len(proofs):
        raise ValueError(f"{who}: one instance per proof")
    bv = BatchVerifier(params, vk, seed, **modes)
    for instance, proof in zip(instances, proofs):
        bv.add_proof(instance, proof)
    return bv


def verify_proofs(params, vk: VerifyingKey, instances, proofs, seed=None, trapdoor: int = None, pairing: str = "host",
                  transcript: str = "host", encoding: str = "halo2", circuits: int = 1, multiopen: str = "shplonk", lookup: str = "halo2") -> bool:
    """True when every ``proofs[i]`` is a valid single-circuit proof of ``vk`` for ``instances[i]``: one ``BatchVerifier``, one check
    (``pairing`` / ``transcript``: where that check's pairing and the proofs' transcripts run, ``encoding``: the proofs' wire format,
    ``circuits=m``: every proof is a ``create_proof_multi`` proof and ``instances[i]`` its m instances, ``multiopen``: the scheme
    the proofs end in, as on ``BatchVerifier``; ``lookup="logup"`` raises ValueError there: such proofs are not batch-verified)"""
    return _batch_of("verify_proofs", params, vk, instances, proofs, seed, pairing=pairing, transcript=transcript, encoding=encoding,
                     circuits=circuits, multiopen=multiopen, lookup=lookup).finalize(trapdoor)


def verify_each(params, vk: VerifyingKey, instances, proofs, seed=None, trapdoor: int = None, pairing: str = "host",
                transcript: str = "host", encoding: str = "halo2", circuits: int = 1, multiopen: str = "shplonk", lookup: str = "halo2") -> List[bool]:
    """[is ``proofs[i]`` a valid single-circuit proof of ``vk`` for ``instances[i]``]: one ``BatchVerifier``, its ``verdicts`` -- the
    per-proof sums in one launch and, with ``pairing="device"``, one pairing call for all proofs (keywords as on ``verify_proofs``;
    ``multiopen="gwc"`` raises ValueError: no verdict per proof under GWC; ``lookup="logup"`` raises it too, as on ``BatchVerifier``)"""
    check_multiopen(multiopen, "verify_each")
    if multiopen == "gwc":
        raise ValueError("verify_each: per-proof verdicts are not available with the \"gwc\" multiopen")
    return _batch_of("verify_each", params, vk, instances, proofs, seed, pairing=pairing, transcript=transcript, encoding=encoding,
                     circuits=circuits, lookup=lookup).verdicts(trapdoor)


