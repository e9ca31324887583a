"""The proof-side mutation sweep's mutants (tests/test_proof_sweep_host.py, tests/test_proof_sweep_gpu.py): every slot of a proof that
``ProofLayout`` lays out -- both encodings, SHPLONK and GWC, ``circuits=m``, ``lookup="logup"`` -- changed one slot at a time in every
way a verifier could overlook, the exchanges of two slots of one kind, and a bit flipped in every byte.  Pure Python on the project's
own codec (``transcript.g1_compress_int`` / ``g1_decompress_int`` / ``g1_uncompressed_int``, ``pairing.g1_add``): no bit position is
stated here that the codec does not state.

A mutant is a ``Mutant(label, key, slot, klass, bytes)``: ``bytes`` the whole changed proof, ``slot`` the first 32-byte slot of the
changed element (a tuple of two for a swap), ``key`` the layout's name for it -- a member of ``point_keys``, or the (commitment key,
rotation) of ``eval_keys`` (a tuple of two for a swap).

What a well-behaved verifier says to a mutant is never written down per slot.  Whether it still DECODES is what the host decoder
(``proof_layout.read_proof_ints``) answers; ``MUST_DECODE`` / ``MUST_NOT_DECODE`` pin the constructed classes against it, so that a
builder that silently made another mutant than its name says fails tests/test_proof_sweep_host.py."""
import random
from collections import Counter, namedtuple

from halo2_experiments_amd import proof_layout as pl
from halo2_experiments_amd.bn256 import FQ_MODULUS as P, FR_MODULUS as R
from halo2_experiments_amd.pairing import G1_GEN, g1_add, g1_neg, g1_on_curve
from halo2_experiments_amd.transcript import g1_compress_int, g1_decompress_int, g1_uncompressed_int

Mutant = namedtuple("Mutant", "label key slot klass bytes")

SCALAR_CLASSES = ("plus_one", "plus_r", "zero")
# x + p beside the codec's flag: the compressed form keeps one bit for the sign of y (g1_compress_int), the uncompressed one none.  The
# class exists for an encoding when EVERY x + p fits the bits the codec leaves to x -- it does for both (2p < 2^255) -- and is absent
# for the whole encoding otherwise, never for single slots.
assert g1_compress_int((0, 1)) == (1 << 255).to_bytes(32, "little")          # the codec's one flag: bit 255, so x has the 255 below it
_HALO2_X_BITS = 255
POINT_CLASSES = {
    "halo2": ("negated", "plus_g", "identity", "off_curve") + (("x_plus_p",) if 2 * P - 1 < 1 << _HALO2_X_BITS else ()),
    "evm": ("negated", "plus_g", "y_plus_one") + (("x_plus_p", "y_plus_p") if 2 * P - 1 < 1 << 256 else ()),
}
MUST_DECODE = frozenset({"plus_one", "negated", "plus_g", "swap"})
MUST_NOT_DECODE = frozenset({"plus_r", "off_curve", "x_plus_p", "y_plus_p", "y_plus_one"})
# "zero" (a canonical scalar) and "identity" (the compressed codec's all-zero bytes) are in neither: the decoder alone says


def decodes(layout, proof: bytes) -> bool:
    """does the host decoder read the proof (``read_proof_ints``: length, canonical scalars and coordinates, points on the curve)"""
    try:
        pl.read_proof_ints(layout, proof)
    except pl.MalformedProof:
        return False
    return True


# ---- the slots ----------------------------------------------------------------------------------------------------------------------------
def width(layout) -> int:
    """the 32-byte slots a point takes"""
    return 2 if layout.encoding == "evm" else 1


def elements(layout):
    """[(key, first slot, slots taken, is a point)] of every element of the proof, in the proof's order"""
    assert len(layout.point_slots) == layout.n_points == len(layout.point_keys)
    assert len(layout.scalar_slots) == layout.n_scalars == len(layout.eval_keys)
    out = [(key, s, width(layout), True) for key, s in zip(layout.point_keys, layout.point_slots)]
    out += [(key, s, 1, False) for key, s in zip(layout.eval_keys, layout.scalar_slots)]
    out.sort(key=lambda e: e[1])
    at = 0
    for _, s, w, _ in out:                                                     # the elements tile the proof
        assert s == at
        at += w
    assert at == layout.slots
    return out


def kind_of(key, is_point: bool) -> str:
    """the kind of an element: the first word of a point's key ("advice", "perm_z", "h1", "w", ...), and for an evaluation "eval:" + the
    kind of the commitment it is an evaluation of"""
    return key[0] if is_point else "eval:" + key[0][0]


def circuit_of(layout, key, is_point: bool):
    """-> (the key without its circuit, the circuit) of a per-circuit element of a multi-circuit layout, else None"""
    if layout.circuits == 1:
        return None
    inner = key if is_point else key[0]
    if len(inner) != 3:                                                        # shared keys: ("random",), ("h_piece", i), ("fixed", i), ...
        return None
    bare = inner[:2]
    return (bare if is_point else (bare, key[1])), inner[2]


def _label(key, is_point: bool) -> str:
    inner, rot = (key, None) if is_point else key
    text = "_".join(str(v) for v in inner[:2])
    if len(inner) == 3:
        text += f"@c{inner[2]}"
    return text if is_point else f"eval_{text}@rot{rot}"


def _put(proof: bytes, slot: int, data: bytes) -> bytes:
    return proof[:32 * slot] + data + proof[32 * slot + len(data):]


def _has_y(x: int) -> bool:
    rhs = (x * x * x + 3) % P
    return rhs == 0 or pow(rhs, (P - 1) // 2, P) == 1


# ---- one slot, every class ---------------------------------------------------------------------------------------------------------------
def scalar_mutants(layout, data: bytes) -> dict:
    """class -> the 32 bytes of a scalar slot"""
    order = "big" if layout.encoding == "evm" else "little"
    v = int.from_bytes(data, order)
    assert v < R
    return {"plus_one": ((v + 1) % R).to_bytes(32, order), "plus_r": (v + R).to_bytes(32, order), "zero": bytes(32)}


def point_mutants(layout, data: bytes) -> dict:
    """class -> the bytes of a point slot (32 compressed, or 64 uncompressed)"""
    if layout.encoding == "evm":
        x, y = g1_uncompressed_int(data)
        enc = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")
        out = {"negated": enc(*g1_neg((x, y))), "plus_g": enc(*g1_add((x, y), G1_GEN)), "y_plus_one": enc(x, (y + 1) % P)}
        if "x_plus_p" in POINT_CLASSES["evm"]:
            out.update(x_plus_p=enc(x + P, y), y_plus_p=enc(x, y + P))
        return out
    x, y = g1_decompress_int(data)
    xo = x + 1
    while _has_y(xo):
        xo += 1
    assert xo < P
    out = {"negated": g1_compress_int(g1_neg((x, y))), "plus_g": g1_compress_int(g1_add((x, y), G1_GEN)), "identity": g1_compress_int(None),
           "off_curve": g1_compress_int((xo, y))}                               # the flag bit as the codec sets it for this y
    if "x_plus_p" in POINT_CLASSES["halo2"]:
        out["x_plus_p"] = g1_compress_int((x + P, y))
    return out


def swap_pairs(layout):
    """[(element a, element b)] to exchange, each once: per kind with two members or more the first two and the last two; in a
    multi-circuit layout also every per-circuit element of circuit 0 with that of circuit m - 1"""
    by_kind: dict = {}
    for e in elements(layout):
        by_kind.setdefault(kind_of(e[0], e[3]), []).append(e)
    pairs, seen = [], set()

    def add(a, b):
        if (a[1], b[1]) not in seen:
            seen.add((a[1], b[1]))
            pairs.append((a, b))

    for members in by_kind.values():
        if len(members) >= 2:
            add(members[0], members[1])
            add(members[-2], members[-1])
    if layout.circuits > 1:
        where = {(e[3], circuit_of(layout, e[0], e[3])): e for e in elements(layout) if circuit_of(layout, e[0], e[3])}
        for (is_point, (bare, c)), e in where.items():
            if c == 0:
                add(e, where[(is_point, (bare, layout.circuits - 1))])
    return pairs


def swap_count(layout) -> int:
    """how many swaps the layout has, counted from its kinds alone: min(members - 1, 2) per kind, and with m >= 3 circuits one per
    per-circuit element of a circuit (with m = 2 those coincide with first <-> second where a kind has one member per circuit)"""
    kinds = Counter(kind_of(key, True) for key in layout.point_keys) + Counter(kind_of(key, False) for key in layout.eval_keys)
    count = sum(min(members - 1, 2) for members in kinds.values())
    if layout.circuits > 1:
        assert layout.circuits >= 3, "swap_count: two circuits are not counted here"
        lane = layout.lane
        own = ("advice", "lookup_a", "lookup_s", "lookup_z", "perm_z", "logup_m", "logup_phi")
        count += sum(key[0] in own for key in lane.point_keys) + sum(key[0][0] in own for key in lane.eval_keys)
    return count


def expected_count(layout) -> int:
    """the constructed mutants of one proof of the layout, swaps included, when no swap pair is byte-equal"""
    return len(SCALAR_CLASSES) * layout.n_scalars + len(POINT_CLASSES[layout.encoding]) * layout.n_points + swap_count(layout)


def mutants(layout, proof: bytes, skipped: list = None) -> list:
    """Every constructed mutant of ``proof``: the scalar classes at every scalar slot, the encoding's point classes at every point
    slot, and the swaps.  A swap of two byte-equal contents changes nothing and is left out; ``skipped``, when given, receives its
    label."""
    assert decodes(layout, proof), "mutants: the proof to mutate does not decode"
    out = []
    for key, slot, w, is_point in elements(layout):
        data = proof[32 * slot:32 * (slot + w)]
        made = point_mutants(layout, data) if is_point else scalar_mutants(layout, data)
        assert tuple(made) == (POINT_CLASSES[layout.encoding] if is_point else SCALAR_CLASSES)
        for klass, new in made.items():
            assert len(new) == 32 * w and new != data, (key, klass)
            out.append(Mutant(f"{_label(key, is_point)}:{klass}", key, slot, klass, _put(proof, slot, new)))
    for a, b in swap_pairs(layout):
        da, db = proof[32 * a[1]:32 * (a[1] + a[2])], proof[32 * b[1]:32 * (b[1] + b[2])]
        label = f"{_label(a[0], a[3])}<->{_label(b[0], b[3])}:swap"
        if da == db:
            if skipped is not None:
                skipped.append(label)
            continue
        out.append(Mutant(label, (a[0], b[0]), (a[1], b[1]), "swap", _put(_put(proof, a[1], db), b[1], da)))
    return out


def byte_flips(layout, proof: bytes, rng: random.Random) -> list:
    """for every element and every one of its bytes (32, or 64 for an uncompressed point), the proof with one bit of that byte
    flipped, the bit drawn from ``rng``"""
    out = []
    for key, slot, w, is_point in elements(layout):
        for i in range(32 * w):
            at, bit = 32 * slot + i, rng.randrange(8)
            out.append(Mutant(f"{_label(key, is_point)}:byte{i}^{1 << bit:#04x}", key, slot, "byte_flip",
                              proof[:at] + bytes([proof[at] ^ (1 << bit)]) + proof[at + 1:]))
    assert len(out) == 32 * layout.slots
    return out


def touches(m: Mutant, slot: int) -> bool:
    return slot in m.slot if isinstance(m.slot, tuple) else m.slot == slot


def kinds_covered(layout) -> set:
    """the kinds of the layout's points; "perm_z" only counts with two permutation sets or more (the last-row evaluation)"""
    return {key[0] for key in layout.point_keys if key[0] != "perm_z" or layout.nsets >= 2}


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def sweep(verify, mutants_) -> list:
    """the mutants ``verify(proof bytes)`` ACCEPTS: what must be empty for a verifier that binds every element"""
    return [m for m in mutants_ if verify(m.bytes)]


def one_per_class(mutants_) -> list:
    """the first mutant of every class, in order of appearance"""
    first = {}
    for m in mutants_:
        first.setdefault(m.klass, m)
    return list(first.values())


# ---- instance and key ---------------------------------------------------------------------------------------------------------------------
def instance_mutants(layout, instance) -> list:
    """[(label, instance)] with one value of one column of one circuit plus one, in the form ``verify_proof`` / ``verify_proof_multi``
    / ``add_proof`` take: a flat list (one column) or a list of columns per circuit"""
    def of_one(inst):
        if inst and isinstance(inst[0], (list, tuple)):
            return [(f"col{c}[{i}]", [list(col) if j != c else list(col[:i]) + [(col[i] + 1) % R] + list(col[i + 1:]) for j, col in enumerate(inst)])
                    for c, col in enumerate(inst) for i in range(len(col))]
        return [(f"[{i}]", list(inst[:i]) + [(inst[i] + 1) % R] + list(inst[i + 1:])) for i in range(len(inst))]

    if layout.circuits == 1:
        return of_one(instance)
    return [(f"c{c}{label}", [changed if j == c else one for j, one in enumerate(instance)])
            for c, inst in enumerate(instance) for label, changed in of_one(inst)]


def key_mutants(vk) -> list:
    """[(label, the key with ONE fixed or permutation commitment replaced by itself + G)], every commitment once"""
    import dataclasses

    import numpy as np

    from halo2_experiments_amd.bn256 import FQ_ONE_MONT, g1_words
    from halo2_experiments_amd.shplonk import g1_words_to_int

    out = []
    for field, name in (("fixed_commitments", "fixed"), ("permutation_commitments", "sigma")):
        rows = np.asarray(getattr(vk, field))
        for i in range(len(rows)):
            moved = g1_add(g1_words_to_int(rows[i]), G1_GEN)
            assert moved is not None and g1_on_curve(moved)
            changed = rows.copy()
            changed[i] = np.concatenate([g1_words(moved), FQ_ONE_MONT])
            assert g1_words_to_int(changed[i]) == moved
            out.append((f"{name}_{i}", dataclasses.replace(vk, **{field: changed})))
    return out
