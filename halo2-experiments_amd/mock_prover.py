"""``MockProver`` of ``halo2_proofs::dev`` for a BATCH of witnesses on the GPU (csrc/mock.hip): does every
user's witness satisfy the constraint system -- every gate polynomial on every usable row, both cells of every copy constraint,
every lookup input in its table -- and if not, which gate, row, copy or lookup of which user fails.

    mp = MockProver(cs, layout)                       # or MockProver(cs, k=..., fixed=..., copies=..., blinding_rows=...)
    res = mp.verify(advice, instance)                 # the tensors a witness function returns, or a chunk of them
    res.ok, res.total, res.failures, res.users_failed
    mp.assert_satisfied(advice, instance)

Semantics are upstream's ``MockProver::verify``: gates and lookup inputs on the usable rows (row < n - blinding_rows), rotations
wrapping modulo n inside a user's own columns, the table of a lookup being the set of its table expression's values on the usable
rows.  ``CellNotAssigned`` and the instance-length checks are not made.  Cells, gate names and polynomial indices are those of
``layout.copies()`` and ``cs.gates``.

How the gates are checked in one read of the batch: the combined program -- every polynomial folded by a ``y`` drawn from ``seed``,
as ``GraphEvaluator.add_custom_gates`` builds it for ``evaluate_h`` -- runs on every (user, row) and appends the lanes whose value is
not zero; the per-polynomial programs then run on those lanes only and name gate and polynomial exactly.  The fold is a polynomial of
degree below the number of polynomials in ``y``, so it misses an unsatisfied row with probability at most (number of polynomials) / r
over ``seed``, r the 254-bit order of the field: the bound the proof system itself rests on.

A lookup whose table expression reads fixed columns only (every lookup of the circuits here: the u8 column) has its table evaluated
once per ``MockProver`` and sorted once per call.  Otherwise the table is evaluated and sorted per user in a loop of m calls: correct,
not fast.  A lookup over a tuple of expressions raises ``NotImplementedError``.

``total`` and ``users_failed`` are exact whatever ``max_failures``.  ``failures`` holds the smallest ``max_failures`` failures per kind
in sorted order, so a call repeated gives the same answer -- as long as no pass finds more than ``max_records`` failing lanes; beyond
that the records kept are whichever reached the buffer first (``total`` stays exact; the gates are then named by running every
polynomial over the whole batch)."""
from __future__ import annotations

import ctypes
import random
import types
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._marshal import _dev_ptr, _ptr, _stream_ptr, _u32p
from .circuits import ConstraintSystem
from .domain import FR_MODULUS, fr_words
from .evaluation import Advice, Expression, Fixed, GraphEvaluator, Instance, Negated, Product, Scaled, Sum
from .keygen import copy_pairs
from .poseidon import ints_to_words

R = FR_MODULUS
KINDS = ("gate", "copy", "lookup")


class NotSatisfied(AssertionError):
    """``assert_satisfied``: the witness batch does not satisfy the constraint system; ``result`` is the ``MockResult``."""

    def __init__(self, message: str, result: "MockResult"):
        super().__init__(message)
        self.result = result


@dataclass
class MockResult:
    ok: bool
    total: Dict[str, int]
    failures: List[Tuple]
    users_failed: List[int] = field(default_factory=list)


def decode_records(records) -> List[Tuple[int, int]]:
    """A record buffer of the device entries (u64 words: user << 32 | row, or user << 32 | copy index) -> sorted (user, index) pairs."""
    rec = np.sort(np.ascontiguousarray(records).view(np.uint64).reshape(-1))
    return list(zip((rec >> np.uint64(32)).astype(np.int64).tolist(), (rec & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()))


def _cell_text(cell) -> str:
    kind, column, row = cell
    return f"(Column('{kind.capitalize()}', {column}), outside any region, on row {row})"


def format_failure(failure: Tuple, cs: Optional[ConstraintSystem] = None) -> str:
    """One failure in the words of upstream's ``VerifyFailure`` (no regions are kept here: every location is "outside any region"),
    with the user in front."""
    kind, user = failure[0], failure[1]
    if kind == "gate":
        _, _, name, poly, row = failure
        index = next((i for i, (g, _) in enumerate(cs.gates) if g == name), "?") if cs is not None else "?"
        return f"user {user}: Constraint {poly} in gate {index} ('{name}') is not satisfied outside any region, on row {row}"
    if kind == "copy":
        return f"user {user}: Equality constraint not satisfied by cell {_cell_text(failure[2])} and cell {_cell_text(failure[3])}"
    if kind == "lookup":
        return f"user {user}: Lookup {failure[2]} is not satisfied outside any region, on row {failure[3]}"
    raise ValueError(f"not a failure: {failure!r}")


def _reads_witness(e: Expression) -> bool:
    if isinstance(e, (Advice, Instance)):
        return True
    if isinstance(e, (Sum, Product)):
        return _reads_witness(e.a) or _reads_witness(e.b)
    if isinstance(e, (Negated, Scaled)):
        return _reads_witness(e.a)
    return False


class MockProver:
    def __init__(self, cs: ConstraintSystem, layout=None, *, k: int = None, fixed=None, copies=None, blinding_rows: int = None,
                 device="cuda", max_records: int = 1 << 24):
        """``layout``: a layout of ``synthesis`` (its k, ``fixed_columns()`` and ``copies()``); or ``k``, ``fixed`` (``cs.num_fixed``
        columns of n integers, or an (num_fixed, n, 4) array of Montgomery words) and ``copies`` (pairs of (kind, column, row) cells).
        ``blinding_rows``: the rows at the end of every column that are not checked, default ``cs.blinding_factors + 1``.
        Nothing touches the device before the first ``verify``."""
        if layout is not None:
            if k is not None or fixed is not None or copies is not None:
                raise ValueError("MockProver: give a layout, or k / fixed / copies, not both")
            layout.check_constraint_system(cs)
            k, fixed, copies = layout.k, layout.fixed_columns(), layout.copies()
        if k is None or fixed is None:
            raise ValueError("MockProver: need a layout, or k and fixed")
        for li, (ins, tabs) in enumerate(cs.lookups):
            if len(ins) != 1 or len(tabs) != 1:
                raise NotImplementedError(f"MockProver: lookup {li} is over a tuple of {len(ins)} expressions; only single-expression lookups are checked")
        self.cs, self.k, self.n = cs, int(k), 1 << int(k)
        self.blinding_rows = cs.blinding_factors + 1 if blinding_rows is None else int(blinding_rows)
        self.usable = self.n - self.blinding_rows
        if not 0 <= self.k <= 30 or self.blinding_rows < 0 or self.usable < 1:
            raise ValueError(f"MockProver: k = {k} leaves no usable row beside {self.blinding_rows} blinding rows")
        if cs.num_fixed + cs.num_advice + cs.num_instance > 256:
            raise ValueError("MockProver: more than 256 columns")
        if cs.num_advice < 1:
            raise ValueError("MockProver: a constraint system without advice columns has no witness to check")
        if isinstance(fixed, np.ndarray) and fixed.ndim == 3:
            words = np.ascontiguousarray(fixed).view(np.uint64)
            if words.shape != (cs.num_fixed, self.n, 4):
                raise ValueError(f"MockProver: fixed must be ({cs.num_fixed}, {self.n}, 4) words, got {words.shape}")
        else:
            fixed = list(fixed)
            if len(fixed) != cs.num_fixed:
                raise ValueError(f"MockProver: {len(fixed)} fixed columns given, the constraint system has {cs.num_fixed}")
            for i, col in enumerate(fixed):
                if len(col) != self.n:
                    raise ValueError(f"MockProver: fixed column {i} holds {len(col)} rows, k = {self.k} means {self.n} (k too small for the layout?)")
            distinct: dict = {}
            index = np.fromiter((distinct.setdefault(int(v) % R, len(distinct)) for col in fixed for v in col), dtype=np.int64,
                                count=cs.num_fixed * self.n)
            words = ints_to_words(list(distinct))[index].reshape(cs.num_fixed, self.n, 4) if cs.num_fixed else np.zeros((0, self.n, 4), np.uint64)
        self._fixed_words = words
        self.copies = [tuple(map(tuple, c)) for c in (copies or [])]
        counts = {"fixed": cs.num_fixed, "advice": cs.num_advice, "instance": cs.num_instance}
        for a, b in self.copies:
            for kind, column, row in (a, b):
                if kind not in counts or not 0 <= column < counts[kind]:
                    raise ValueError(f"MockProver: a copy names the cell {(kind, column, row)}, which is in no column of the constraint system")
                if not 0 <= row < self.n:
                    raise ValueError(f"MockProver: a copy names row {row}, k = {self.k} has {self.n} rows (k too small for the layout)")
        self._pairs = copy_pairs(cs, types.SimpleNamespace(n=self.n, copies=lambda: self.copies))
        base = {"fixed": 0, "advice": cs.num_fixed, "instance": cs.num_fixed + cs.num_advice}
        self._perm = np.array([base[kind] + i for kind, i in cs.equality], dtype=np.uint32)
        self.polynomials = [(name, pi, p) for name, polys in cs.gates for pi, p in enumerate(polys)]
        self.device, self.max_records = device, int(max_records)
        self._dev = None

    # ---- device state, built once ----------------------------------------------------------------------------------
    def _program(self, polys: Sequence[Expression]):
        g = GraphEvaluator()
        g.add_custom_gates(list(polys))
        return g.compile(self.cs.num_fixed, self.cs.num_advice, self.cs.num_instance)

    def _state(self):
        if self._dev is None:
            import torch

            device = torch.device(self.device)
            if device.type != "cuda":
                raise ValueError("MockProver: the checker runs on a GPU; device must be a cuda device")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            with torch.cuda.device(device):
                d = types.SimpleNamespace(device=device)
                d.fixed = torch.from_numpy(self._fixed_words.view(np.int64)).to(device).contiguous()
                d.combined = self._program([p for _, _, p in self.polynomials]) if self.polynomials else None
                d.per_poly = [self._program([p]) for _, _, p in self.polynomials]
                d.pairs = torch.from_numpy(self._pairs.view(np.int32).copy()).to(device) if len(self._pairs) else None
                d.lookups = []
                for ins, tabs in self.cs.lookups:
                    entry = types.SimpleNamespace(input=self._program([ins[0]]), table=self._program([tabs[0]]), shared=None)
                    if not _reads_witness(tabs[0]):
                        filler = d.fixed[0] if self.cs.num_fixed else torch.zeros((self.n, 4), dtype=torch.int64, device=device)
                        cols = [d.fixed[i] for i in range(self.cs.num_fixed)] + [filler] * (self.cs.num_advice + self.cs.num_instance)
                        entry.shared = torch.zeros((self.n, 4), dtype=torch.int64, device=device)
                        entry.table.evaluate(cols, entry.shared)
                    d.lookups.append(entry)
            self._dev = d
        return self._dev

    # ---- arguments ---------------------------------------------------------------------------------------------------
    def _batch(self, advice, instance):
        import torch

        d = self._state()
        cs, n = self.cs, self.n
        if not (torch.is_tensor(advice) and advice.is_cuda and advice.dtype == torch.int64):
            raise ValueError("MockProver: advice must be an int64 GPU tensor")
        if advice.dim() == 3:
            advice = advice.unsqueeze(0)
        if advice.dim() != 4 or tuple(advice.shape[1:]) != (cs.num_advice, n, 4):
            raise ValueError(f"MockProver: advice must be (m, {cs.num_advice}, {n}, 4) or ({cs.num_advice}, {n}, 4), got {tuple(advice.shape)}")
        m = advice.shape[0]
        if m == 0:
            raise ValueError("MockProver: no witness in the batch")
        if advice.device != d.device or not advice.is_contiguous():
            raise ValueError(f"MockProver: advice must be contiguous and on {d.device}")
        if instance is None:
            instance = [None] * cs.num_instance
        insts = list(instance) if isinstance(instance, (list, tuple)) else [instance]
        if len(insts) != cs.num_instance:
            raise ValueError(f"MockProver: {len(insts)} instance columns given, the constraint system has {cs.num_instance}")
        out = []
        for t in insts:
            # a column without values (None, an empty list or an (m, 0, 4) tensor): every cell reads as zero, which one zero row says
            if t is None or (isinstance(t, (list, tuple)) and len(t) == 0) or (torch.is_tensor(t) and t.numel() == 0):
                out.append(torch.zeros((m, 1, 4), dtype=torch.int64, device=d.device))
                continue
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.device == d.device):
                raise ValueError(f"MockProver: an instance column must be an int64 GPU tensor on {d.device}")
            if t.dim() == 2 and m == 1:
                t = t.unsqueeze(0)
            if t.dim() != 3 or t.shape[0] != m or t.shape[2] != 4 or not 1 <= t.shape[1] <= n or not t.is_contiguous():
                raise ValueError(f"MockProver: an instance column must be a contiguous ({m}, rows <= {n}, 4) tensor, got {tuple(t.shape)}")
            out.append(t)
        return advice, out, m

    def _table(self, advice, insts, user: int = 0):
        """the batched column table from `user` on: (bases, strides, rows, count) as the entries take them"""
        cs, n, d = self.cs, self.n, self._dev
        bases = [d.fixed[i].data_ptr() for i in range(cs.num_fixed)]
        strides, rows = [0] * cs.num_fixed, [n] * cs.num_fixed
        a_stride = cs.num_advice * n * 8
        for c in range(cs.num_advice):
            bases.append(advice.data_ptr() + 4 * (user * a_stride + c * n * 8))
            strides.append(a_stride)
            rows.append(n)
        for t in insts:
            bases.append(t.data_ptr() + 4 * user * t.shape[1] * 8)
            strides.append(t.shape[1] * 8)
            rows.append(t.shape[1])
        count = len(bases)
        return ((ctypes.c_void_p * count)(*bases), (ctypes.c_uint64 * count)(*strides), (ctypes.c_uint32 * count)(*rows), count)

    # ---- the passes ---------------------------------------------------------------------------------------------------
    def _collect(self, launch, cap: int):
        """launch(records, cap, counter) -> the counter behind the call.  -> (total, device tensor of the records kept): all of them
        unless there are more than max_records."""
        import torch

        d = self._dev
        rec = torch.empty(cap, dtype=torch.int64, device=d.device)
        counter = torch.zeros(1, dtype=torch.int64, device=d.device)
        total = launch(rec, cap, counter)
        if cap < total <= self.max_records:
            cap, rec = total, torch.empty(total, dtype=torch.int64, device=d.device)
            counter.zero_()
            total = launch(rec, cap, counter)
        return total, rec[:min(total, cap)]

    def _call(self, advice, instance, seed: int):
        """what every pass of one call shares: the batch, its table, the per-call constants, the flag array"""
        import torch

        advice, insts, m = self._batch(advice, instance)
        d = self._dev
        y = random.Random(seed).randrange(1, R)
        dyn = np.ascontiguousarray(np.stack([fr_words(v) for v in (0, 0, 0, y)]))
        with torch.cuda.device(d.device):
            flags = torch.zeros(m, dtype=torch.uint8, device=d.device)
        return types.SimpleNamespace(advice=advice, insts=insts, m=m, dyn=dyn, dynp=_ptr(dyn), flags=flags,
                                     table=self._table(advice, insts), stream=ctypes.c_void_p(_stream_ptr(advice)), out=ctypes.c_uint64(0))

    def _gates(self, c, prog, lanes):
        """-> launch(records, cap, counter) of ``_collect``: program `prog` on every lane of the batch, or on the records `lanes`"""
        bases, strides, rows, count = c.table

        def launch(rec, cap, counter):
            _lib.check(_lib.load().hm_mock_gates_dev(ctypes.c_uint64(prog.handle), bases, strides, rows, count, c.dynp, 4, self.k, self.usable, c.m,
                                                     _dev_ptr(lanes), lanes.numel() if lanes is not None else 0, _dev_ptr(rec), cap,
                                                     _dev_ptr(counter), ctypes.c_void_p(c.flags.data_ptr()), ctypes.byref(c.out), c.stream))
            return c.out.value
        return launch

    def unsatisfied_lanes(self, advice, instance=None, seed: int = 0, cap: int = 4096):
        """The first pass of ``verify`` alone, the one read of the batch: -> (number of (user, row) lanes on which the gates' fold is
        not zero, a device tensor of at most ``cap`` of them as records user << 32 | row, in no order)."""
        import torch

        c = self._call(advice, instance, seed)
        d = self._dev
        if d.combined is None:
            return 0, torch.empty(0, dtype=torch.int64, device=d.device)
        with torch.cuda.device(d.device):
            rec = torch.empty(cap, dtype=torch.int64, device=d.device)
            counter = torch.zeros(1, dtype=torch.int64, device=d.device)
            total = self._gates(c, d.combined, None)(rec, cap, counter)
        return total, rec[:min(total, cap)]

    def verify(self, advice, instance=None, max_failures: int = 1024, seed: int = 0) -> MockResult:
        import torch

        if max_failures < 1:
            raise ValueError("MockProver.verify: max_failures must be at least 1")
        c = self._call(advice, instance, seed)
        advice, insts, m, flags, dynp, stream, out_total = c.advice, c.insts, c.m, c.flags, c.dynp, c.stream, c.out
        d, cs, lib = self._dev, self.cs, _lib.load()
        cap0 = max(int(max_failures), 4096)
        total = {kind: 0 for kind in KINDS}
        failures: Dict[str, List[Tuple]] = {kind: [] for kind in KINDS}
        with torch.cuda.device(d.device):
            bases, strides, rows, count = c.table
            if d.combined is not None:
                flagged_total, flagged = self._collect(self._gates(c, d.combined, None), cap0)
                if flagged_total:
                    whole = flagged_total > flagged.numel()          # more lanes than records are kept: every polynomial over the batch
                    for (name, pi, _), prog in zip(self.polynomials, d.per_poly):
                        t, rec = self._collect(self._gates(c, prog, None if whole else flagged), cap0 if whole else flagged.numel())
                        total["gate"] += t
                        failures["gate"] += [("gate", u, name, pi, row) for u, row in decode_records(rec.cpu().numpy())]
            if d.pairs is not None:
                def launch(rec, cap, counter):
                    _lib.check(lib.hm_mock_copies_dev(bases, strides, rows, count, self._perm.ctypes.data_as(_u32p), len(self._perm),
                                                      _dev_ptr(d.pairs, _u32p), len(self._pairs), self.k, m,
                                                      _dev_ptr(rec), cap, _dev_ptr(counter),
                                                      ctypes.c_void_p(flags.data_ptr()), ctypes.byref(out_total), stream))
                    return out_total.value
                total["copy"], rec = self._collect(launch, cap0)
                failures["copy"] = [("copy", u, *self.copies[ci]) for u, ci in decode_records(rec.cpu().numpy())]
            for li, lk in enumerate(d.lookups):
                def launch(rec, cap, counter, lk=lk):
                    users = [(0, m, lk.shared)] if lk.shared is not None else [(u, 1, None) for u in range(m)]
                    for u, count_u, table in users:
                        tb = (bases, strides, rows, count) if table is not None else self._table(advice, insts, u)
                        if table is None:                       # this user's table: the expression over the user's own columns
                            table = torch.zeros((self.n, 4), dtype=torch.int64, device=d.device)
                            cols = [d.fixed[i] for i in range(cs.num_fixed)] + [advice[u, c] for c in range(cs.num_advice)]
                            for t in insts:
                                col = torch.zeros((self.n, 4), dtype=torch.int64, device=d.device)
                                col[:t.shape[1]] = t[u]
                                cols.append(col)
                            lk.table.evaluate(cols, table)
                        _lib.check(lib.hm_mock_lookup_dev(ctypes.c_uint64(lk.input.handle), tb[0], tb[1], tb[2], tb[3], dynp, 4, self.k, self.usable,
                                                          count_u, u, ctypes.c_void_p(table.data_ptr()), _dev_ptr(rec), cap,
                                                          _dev_ptr(counter), ctypes.c_void_p(flags.data_ptr()),
                                                          ctypes.byref(out_total), stream))
                    return out_total.value
                t, rec = self._collect(launch, cap0)
                total["lookup"] += t
                failures["lookup"] += [("lookup", u, li, row) for u, row in decode_records(rec.cpu().numpy())]
            users_failed = flags.nonzero().flatten().tolist()
        kept: List[Tuple] = []
        for kind in KINDS:
            kept += sorted(failures[kind])[:max_failures]
        return MockResult(ok=not any(total.values()), total=total, failures=sorted(kept), users_failed=users_failed)

    def assert_satisfied(self, advice, instance=None, seed: int = 0, show: int = 8) -> None:
        """Raises ``NotSatisfied`` with the first ``show`` failures in upstream's words when the batch is not satisfied."""
        res = self.verify(advice, instance, max_failures=max(show, 1), seed=seed)
        if not res.ok:
            by_kind = sorted(res.failures, key=lambda f: KINDS.index(f[0]))          # gates first, as upstream lists them
            lines = [format_failure(f, self.cs) for f in by_kind[:show]]
            more = sum(res.total.values()) - len(lines)
            raise NotSatisfied("the witness batch is not satisfied (" + ", ".join(f"{res.total[k]} {k}" for k in KINDS) + f" failures, "
                               f"{len(res.users_failed)} users):\n  " + "\n  ".join(lines) + (f"\n  ... and {more} more" if more > 0 else ""), res)
