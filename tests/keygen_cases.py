"""Copy sets for the keygen tests (tests/test_keygen.py on the host build, tests/test_keygen_gpu.py on the device), and the CPU twin's
answer for a raw set: ``synthesis.permutation_cells`` run on a stand-in layout whose columns are P advice columns."""
import random
from types import SimpleNamespace

from halo2_experiments_amd import circuits, synthesis as sy


def real_layouts():
    """(name, constraint system, layout): the reference's three circuits at their test shapes"""
    return [("merkle_sum_tree depth 5 k 9", circuits.merkle_sum_tree(), sy.MerkleSumTreeLayout(5, 9)),
            ("merkle_v3 depth 5 k 8", circuits.merkle_v3(), sy.MerkleTreeV3Layout(5, 8)),
            ("poseidon k 6", circuits.poseidon(), sy.PoseidonCircuitLayout(6))]


def twin_cells(pairs, P, k):
    """sigma as a flat list of cell ids from ``synthesis.permutation_cells``"""
    n = 1 << k
    cs = SimpleNamespace(equality=[("advice", j) for j in range(P)])
    lay = SimpleNamespace(n=n, copies=lambda: [(("advice", a // n, a % n), ("advice", b // n, b % n)) for a, b in pairs])
    return [j * n + i for col in sy.permutation_cells(cs, lay) for (j, i) in col]


def small_sets(P=3, k=4):
    """(name, pairs) over P * 2^k cells: seeded random sets, and the shapes a union-find or the link rule can get wrong"""
    cells = P << k
    rng = random.Random(1616)
    out = []
    for m in (1, 2, 7, 20, 60, 200):
        out.append((f"random m={m}", [(rng.randrange(cells), rng.randrange(cells)) for _ in range(m)]))
    out.append(("self copies only", [(c, c) for c in (0, 5, cells - 1)]))
    out.append(("self copies among others", [(3, 3), (3, 9), (9, 9), (20, 20), (41, 2)]))
    out.append(("repeated pairs", [(4, 17)] * 5 + [(17, 30)] * 3))
    out.append(("both orders of a pair", [(4, 17), (17, 4), (30, 31), (31, 30), (4, 17)]))
    chain = sorted(rng.sample(range(cells), 12))
    out.append(("chain back to front", [(chain[i + 1], chain[i]) for i in reversed(range(len(chain) - 1))]))
    out.append(("chain front to back", [(chain[i], chain[i + 1]) for i in range(len(chain) - 1)]))
    hub = 23
    out.append(("star", [(hub, c) if c % 2 else (c, hub) for c in rng.sample(range(cells), 15) if c != hub]))
    out.append(("star on the largest cell", [(cells - 1, c) for c in range(0, cells - 1, 5)]))
    everyone = list(range(cells))
    rng.shuffle(everyone)
    out.append(("all cells in one class", list(zip(everyone, everyone[1:]))))
    out.append(("two classes that meet last", [(0, 1), (1, 2), (40, 41), (41, 42), (2, 40)]))
    out.append(("first and last cell", [(0, cells - 1)]))
    out.append(("no copies", []))
    return out
