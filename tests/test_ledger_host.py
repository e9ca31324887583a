"""The ledger openings without a GPU (halo2_experiments_amd/ledger.py, csrc/ledger.inc): the challenge, the integer algebra of one
id-bound opening per user on a ledger made through the trapdoor, the attack the feature exists for, the kernel's lane function built on
the host with bound tracking (``hc_ledger_pair``: a violated bound aborts the process) against ``pairing.py`` integers word for word,
and the refusals of ``hm_kzg_ledger_pairs_bn256_dev``, which come before a device is needed."""
import ctypes
import random

import numpy as np
import pytest

from halo2_experiments_amd import _lib, ledger as lg, solvency
from halo2_experiments_amd.bn256 import FQ_MODULUS as P_MOD, FR_MODULUS as R, fr_array, fr_words, g1_words
from halo2_experiments_amd.openings import domain_omega
from halo2_experiments_amd.pairing import G1_GEN, g1_mul, g1_neg

import ledger_cases as lc

K, ASSETS = 3, 2


@pytest.fixture(scope="module")
def led():
    return lc.int_ledger(K, ASSETS, seed=1)


@pytest.fixture(scope="module")
def hc():
    return lc.load_twin()


# ---- the challenge --------------------------------------------------------------------------------------------------------------------
def test_gamma_is_deterministic_and_binds_every_input(led):
    c_id, cs = led["c_id"], led["cs"]
    base = lg.ledger_gamma(K, c_id, cs)
    assert base == lg.ledger_gamma(K, c_id, list(cs)) == led["gamma"] and 0 <= base < R
    assert base == lg.ledger_gamma(K, g1_words(c_id), [g1_words(c) for c in cs])           # the same from affine words
    other = g1_mul(12345, G1_GEN)
    changed = [lg.ledger_gamma(K + 1, c_id, cs), lg.ledger_gamma(K, other, cs), lg.ledger_gamma(K, c_id, [other, cs[1]]),
               lg.ledger_gamma(K, c_id, [cs[0], other]), lg.ledger_gamma(K, c_id, cs + [None]), lg.ledger_gamma(K, c_id, cs[:1]),
               lg.ledger_gamma(K, None, cs), lg.ledger_gamma(K, c_id, [cs[1], cs[0]])]
    assert len(set(changed + [base])) == len(changed) + 1
    assert len(lg.PERSON) == 16


def test_eta_binds_the_published_sums_too(led):
    c_id, cs = led["c_id"], led["cs"]
    base = lg.ledger_eta(K, c_id, cs, 5, [6, 7])
    assert base == lg.ledger_eta(K, c_id, cs, 5 + R, [6, 7 + R]) and base != lg.ledger_gamma(K, c_id, cs) and 0 <= base < R
    changed = [lg.ledger_eta(K, c_id, cs, 4, [6, 7]), lg.ledger_eta(K, c_id, cs, 5, [5, 7]), lg.ledger_eta(K, c_id, cs, 5, [6, 8]),
               lg.ledger_eta(K, c_id, cs, 5, [7, 6]), lg.ledger_eta(K + 1, c_id, cs, 5, [6, 7]), lg.ledger_eta(K, c_id, [cs[1], cs[0]], 5, [6, 7]),
               lg.ledger_eta(K, None, cs, 5, [6, 7])]
    assert len(set(changed + [base])) == len(changed) + 1 and len(lg.TOTALS_PERSON) == 16 and lg.TOTALS_PERSON != lg.PERSON


def test_sums_that_compensate_under_a_known_challenge_are_rejected(led):
    """The opening at 0 is of C_eta, eta hashed from the sums themselves.  Were it of C_gamma, understating T_0 by d and raising the
    unverifiable S_id by gamma d would keep the one linear equation: that forgery, and its twin under eta, must fail."""
    p, pub, n, gamma = led["params"], (led["c_id"], led["cs"]), led["n"], led["gamma"]
    s_id, sums = sum(led["ids"]) % R, [sum(col) for col in led["bal"]]
    eta = lg.ledger_eta(K, led["c_id"], led["cs"], s_id, sums)
    lag = lc.lagrange_at(K, lc.S)
    combined = [lg.combined_value(eta, led["ids"][i], [col[i] for col in led["bal"]]) for i in range(n)]
    at_s, at_0 = sum(v * l for v, l in zip(combined, lag)) % R, sum(combined) * pow(n, -1, R) % R
    opening = g1_mul((at_s - at_0) * pow(lc.S, -1, R) % R, G1_GEN)                          # [(g_eta(s) - g_eta(0)) / s]G
    assert lg.verify_ledger_totals(p, pub, s_id, sums, opening)
    assert lg.verify_ledger_totals(p, lg.ledger_statement(p, pub), s_id, sums, g1_words(opening))
    d = 1000
    assert not lg.verify_ledger_totals(p, pub, s_id, [sums[0] - d, sums[1]], opening)
    for ch in (gamma, eta):                                                                 # the compensating forgery
        assert not lg.verify_ledger_totals(p, pub, (s_id + ch * d) % R, [sums[0] - d, sums[1]], opening)
        assert not lg.verify_ledger_totals(p, pub, s_id, [sums[0] - d, (sums[1] + pow(ch, -1, R) * d) % R], opening)   # between two totals
    # the same forgery against the opening a prover WOULD make for gamma: rejected as well, nothing opens C_gamma at 0
    g_comb = led["g"]
    g_at_s, g_at_0 = sum(v * l for v, l in zip(g_comb, lag)) % R, sum(g_comb) * pow(n, -1, R) % R
    g_opening = g1_mul((g_at_s - g_at_0) * pow(lc.S, -1, R) % R, G1_GEN)
    assert not lg.verify_ledger_totals(p, pub, (s_id + gamma * d) % R, [sums[0] - d, sums[1]], g_opening)
    assert not lg.verify_ledger_totals(p, pub, s_id, sums, g_opening)
    with pytest.raises(ValueError):
        lg.verify_ledger_totals(p, pub, s_id, sums[:1], opening)


# ---- the integer algebra --------------------------------------------------------------------------------------------------------------
def test_every_row_verifies_and_every_change_is_rejected(led):
    p, pub, n = led["params"], (led["c_id"], led["cs"]), led["n"]
    row = lambda i: (led["ids"][i], [col[i] for col in led["bal"]], led["openings"][i])
    for i in range(n):                                                                      # the six zero tail rows among them
        uid, bal, pi = row(i)
        assert lg.verify_ledger_user(p, pub, i, uid, bal, pi), i
    uid, bal, pi = row(1)
    assert not lg.verify_ledger_user(p, pub, 1, (uid + 1) % R, bal, pi)                     # another id
    for a in range(ASSETS):
        wrong = list(bal)
        wrong[a] += 1
        assert not lg.verify_ledger_user(p, pub, 1, uid, wrong, pi), a                      # another balance of each asset in turn
    assert not lg.verify_ledger_user(p, pub, 2, uid, bal, pi)                               # a neighbouring index
    assert not lg.verify_ledger_user(p, pub, 1, uid, bal, led["openings"][2])               # a neighbouring opening
    assert lg.verify_ledger_user(p, pub, 1, fr_words(uid), [fr_words(b) for b in bal], g1_words(pi))     # the same from words
    proof = lg.LedgerProof(led["c_id"], led["cs"], [], 0, [], None)
    assert lg.verify_ledger_user(p, proof, 1, uid, bal, pi)                                 # public as a LedgerProof
    st = lg.ledger_statement(p, pub)
    assert st.gamma == led["gamma"] and st.c_gamma == led["c_gamma"] and lg.verify_ledger_user(p, st, 1, uid, bal, pi)
    with pytest.raises(ValueError):
        lg.verify_ledger_user(p, st, 1, uid, bal, pi, k=K + 1)                              # a statement made for another k
    with pytest.raises(ValueError):
        lg.verify_ledger_user(p, pub, n, uid, bal, pi)
    with pytest.raises(ValueError):
        lg.verify_ledger_user(p, pub, 1, uid, bal[:1], pi)
    with pytest.raises(ValueError):
        lg.verify_ledger_user(p, (led["c_id"], []), 1, uid, [], pi)


def test_one_row_cannot_be_handed_to_two_customers():
    """Two customers with equal balances are both pointed at row 0.  solvency.verify_user accepts both -- it cannot tell them apart --;
    the ledger opening accepts only the one whose id is in the row."""
    led = lc.int_ledger(K, 1, seed=2)
    p, i = led["params"], 0
    balance, mine, yours = led["bal"][0][i], led["ids"][i], (led["ids"][i] + 7) % R
    # the balance column's own opening at omega^i, as solvency.py hands it out
    lag = lc.lagrange_at(K, lc.S)
    at_s = sum(v * l for v, l in zip(led["bal"][0], lag)) % R
    own = g1_mul((at_s - balance) * pow(lc.S - pow(domain_omega(K), i, R), -1, R) % R, G1_GEN)
    for customer in (mine, yours):
        assert solvency.verify_user(p, led["cs"][0], i, balance, own)                       # no id enters: both pass
    pub = (led["c_id"], led["cs"])
    assert lg.verify_ledger_user(p, pub, i, mine, [balance], led["openings"][i])
    assert not lg.verify_ledger_user(p, pub, i, yours, [balance], led["openings"][i])


# ---- the lane function under bound tracking ---------------------------------------------------------------------------------------------
def _check(hc, k, gamma, c_gamma, index, uid, bal, pi):
    """the twin on the Montgomery words of these integers against the integer oracle -> the rows"""
    flag, rows = lc.twin_rows(hc, k, gamma, c_gamma, index, fr_words(uid), fr_array(bal), g1_words(pi))
    expect = lc.expected_rows(k, gamma, c_gamma, index, uid, bal, pi)
    assert flag == 0 and np.array_equal(rows, expect), (index, uid, bal, pi)
    return rows


def test_twin_equals_the_integers_on_generic_and_edge_rows(hc, led):
    rng = random.Random("ledger twin")
    k, gamma, c_gamma, n = K, led["gamma"], led["c_gamma"], led["n"]
    w = domain_omega(k)
    point = lambda: g1_mul(rng.randrange(1, R), G1_GEN)
    rnd = lambda: rng.randrange(R)
    for i in (5, 0, n - 1):                                                                 # a generic row, the first, the last
        assert _check(hc, k, gamma, c_gamma, i, rnd(), [rnd(), rnd()], point())[1].any()
    for i in range(n):                                                                      # the ledger's own rows: true openings
        _check(hc, k, gamma, c_gamma, i, led["ids"][i], [col[i] for col in led["bal"]], led["openings"][i])
    b = [rnd(), rnd()]
    y0 = (-lg.combined_value(gamma, 0, b)) % R
    assert lg.combined_value(gamma, y0, b) == 0
    _check(hc, k, gamma, c_gamma, 3, y0, b, point())                                        # y = 0: the generator's term drops out
    _check(hc, k, gamma, c_gamma, 3, rnd(), b, None)                                        # pi = the identity
    _check(hc, k, gamma, None, 3, rnd(), b, point())                                        # C_gamma = the identity
    _check(hc, k, gamma, c_gamma, 3, R - 1, [R - 1, R - 1], point())                        # the largest canonical scalars
    _check(hc, k, gamma, c_gamma, 3, 0, [0, 0], point())
    _check(hc, k, gamma, c_gamma, 3, rnd(), [], point())                                    # no asset: y is the id
    _check(hc, 0, gamma, c_gamma, 0, rnd(), b, point())                                     # a domain of one row: omega^0 = 1
    _check(hc, 20, gamma, c_gamma, (1 << 20) - 1, rnd(), b, point())                        # a 20-bit row


def test_twin_doubles_cancels_and_reaches_the_identity(hc, led):
    rng = random.Random("ledger twin specials")
    k, gamma, i = K, led["gamma"], 3
    wi = pow(domain_omega(k), i, R)
    b = [rng.randrange(R), rng.randrange(R)]
    c = rng.randrange(1, R)
    c_gamma = g1_mul(c, G1_GEN)
    id_for = lambda y: (y - lg.combined_value(gamma, 0, b)) % R                              # the id that makes the combined value y
    # pi = G makes the ladder's third addend G + pi a doubling, and R = [c - y + omega^i]G: twice [omega^i]G, or the identity
    rows = _check(hc, k, gamma, c_gamma, i, id_for((c - wi) % R), b, G1_GEN)
    assert np.array_equal(rows[1], g1_words(g1_neg(g1_mul(2 * wi % R, G1_GEN))))
    assert not _check(hc, k, gamma, c_gamma, i, id_for((c + wi) % R), b, G1_GEN)[1].any()
    # pi = -G makes G + pi the identity: the joint bits add nothing
    assert not _check(hc, k, gamma, c_gamma, i, id_for((c - wi) % R), b, g1_neg(G1_GEN))[1].any()
    _check(hc, k, gamma, c_gamma, i, id_for((c + wi) % R), b, g1_neg(G1_GEN))
    _check(hc, k, gamma, c_gamma, i, rng.randrange(R), b, G1_GEN)
    # [r - y]G equal and opposite to C_gamma; the last addition meeting its own operand: C_gamma = [omega^i t - y]G with pi = [t]G
    _check(hc, k, gamma, c_gamma, i, id_for((-c) % R), b, g1_mul(5, G1_GEN))
    _check(hc, k, gamma, c_gamma, i, id_for(c), b, g1_mul(5, G1_GEN))
    assert np.array_equal(_check(hc, k, gamma, c_gamma, i, id_for(c), b, None), np.zeros((2, 8), dtype=np.uint64))     # both rows zero, flag 0
    _check(hc, k, gamma, c_gamma, i, id_for((wi * 5 - c) % R), b, g1_mul(5, G1_GEN))
    # inside the ladder: with r - y = 2 and omega^0 = 1 the accumulator [2]G meets the addend pi = [2]G (a doubling) or -[2]G (the identity)
    for pi in (g1_mul(2, G1_GEN), g1_neg(g1_mul(2, G1_GEN))):
        _check(hc, 0, gamma, c_gamma, 0, id_for(R - 2), b, pi)
    assert not _check(hc, 0, gamma, None, 0, id_for(R - 2), b, g1_neg(g1_mul(2, G1_GEN)))[1].any()
    _check(hc, 0, gamma, c_gamma, 0, id_for(R - 3), b, g1_mul(2, G1_GEN))                    # the addend G + pi is taken
    # through the trapdoor: pi = [t]G and C_gamma = [y - omega^i t]G make R the identity
    t, y = rng.randrange(1, R), rng.randrange(R)
    rows = _check(hc, k, gamma, g1_mul((y - wi * t) % R, G1_GEN), i, id_for(y), b, g1_mul(t, G1_GEN))
    assert rows[0].any() and not rows[1].any()


def test_twin_flags_malformed_users(hc, led):
    k, gamma, c_gamma = K, led["gamma"], led["c_gamma"]
    uid, bal, pi = fr_words(led["ids"][1]), fr_array([col[1] for col in led["bal"]]), g1_words(led["openings"][1])
    zero = np.zeros((2, 8), dtype=np.uint64)
    assert lc.twin_rows(hc, k, gamma, c_gamma, 1, uid, bal, pi)[0] == 0
    cases = []
    for pattern in (R, R + 1, (1 << 256) - 1):                                              # a scalar word pattern >= r
        cases.append((1, lc.raw_words(pattern), bal, pi))
        for a in range(ASSETS):
            wrong = bal.copy()
            wrong[a] = lc.raw_words(pattern)
            cases.append((1, uid, wrong, pi))
    off = pi.copy()
    off[4] ^= np.uint64(1)                                                                  # pi off the curve
    cases.append((1, uid, bal, off))
    only_x = pi.copy()
    only_x[4:] = 0                                                                          # (x, 0) with x != 0: not the identity, not on the curve
    cases.append((1, uid, bal, only_x))
    for coord in (0, 4):
        for pattern in (P_MOD, (1 << 256) - 1):                                             # a coordinate equal to p, and above
            bad = pi.copy()
            bad[coord:coord + 4] = lc.raw_words(pattern)
            cases.append((1, uid, bal, bad))
    cases.append((1 << k, uid, bal, pi))                                                    # a row outside the domain
    for index, u, b, o in cases:
        flag, rows = lc.twin_rows(hc, k, gamma, c_gamma, index, u, b, o)
        assert flag == 1 and np.array_equal(rows, zero)
    # r - 1 as a word pattern is canonical (it stands for some element): not flagged
    assert lc.twin_rows(hc, k, gamma, c_gamma, 1, lc.raw_words(R - 1), bal, pi)[0] == 0


# ---- the entry point's refusals ---------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_before_the_device(led):
    lib = _lib.load()
    vp = ctypes.c_void_p
    a, b, c, d, e, f = (vp(0x100000 * j) for j in range(1, 7))
    u32 = lambda v: ctypes.cast(v, lc.u32p)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    keep = [np.ascontiguousarray(w) for w in (fr_words(led["gamma"]), fr_words(domain_omega(K)), g1_words(led["c_gamma"]))]
    gm, om, cg = (w.ctypes.data_as(u64p) for w in keep)
    call = lambda *args: lib.hm_kzg_ledger_pairs_bn256_dev(*args)
    good = [a, u32(b), c, d, gm, om, cg, K, ASSETS, 5, e, u32(f), None]
    for slot in (0, 1, 2, 3, 4, 5, 6, 10, 11):
        args = list(good)
        args[slot] = None
        assert call(*args) == -1 and b"null" in lib.hm_last_error(), slot
    change = lambda **kw: [kw.get(name, v) for name, v in zip("open idx ids bal gamma omega cg k assets users g1 flags stream".split(), good)]
    assert call(*change(users=0)) == -1 and call(*change(users=(1 << 20) + 1)) == -1 and b"n_users" in lib.hm_last_error()
    assert call(*change(k=29)) == -1 and b"log_n" in lib.hm_last_error()
    assert call(*change(assets=(1 << 16) + 1)) == -1 and b"assets" in lib.hm_last_error()
    assert call(*change(open=vp(0x100008))) == -1 and b"aligned" in lib.hm_last_error()
    assert call(*change(flags=u32(vp(0x600002)))) == -1 and b"aligned" in lib.hm_last_error()
    big = np.ascontiguousarray(lc.raw_words(R))
    assert call(*change(gamma=big.ctypes.data_as(u64p))) == -1 and b"below r" in lib.hm_last_error()
    assert call(*change(omega=big.ctypes.data_as(u64p))) == -1
    bad_c = keep[2].copy()
    bad_c[4:] = lc.raw_words(P_MOD)
    assert call(*change(cg=bad_c.ctypes.data_as(u64p))) == -1 and b"below p" in lib.hm_last_error()
    if lib.hm_device_count() == 0:
        assert call(*good) == -2                                                            # no device: an error, never a fallback
