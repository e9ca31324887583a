"""The tests' own Poseidon: written from the description of the construction (the issue text and the Poseidon paper), on Python
integers, sharing no code with halo2_experiments_amd.poseidon -- the product must not be its own judge.  Constants are arguments.

    state = [m_0 .. m_{RATE-1}, RATE * 2^64]
    round r:  state += rc[r];  x -> x^5 on every word (first and last R_F/2 rounds) or on word 0 only (the R_P rounds between);
              state = MDS . state
    digest = state[0]
"""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def matvec(m, v):
    out = []
    for row in m:
        acc = 0
        for a, b in zip(row, v):
            acc += a * b
        out.append(acc % R)
    return out


def permutation(state, rc, mds, r_f, r_p):
    t = len(state)
    assert len(rc) == r_f + r_p and len(mds) == t
    state = list(state)
    for r in range(r_f + r_p):
        for j in range(t):
            state[j] = (state[j] + rc[r][j]) % R
        is_full = r < r_f // 2 or r >= r_f // 2 + r_p
        for j in range(t if is_full else 1):
            x = state[j]
            x2 = x * x % R
            state[j] = x2 * x2 % R * x % R
        state = matvec(mds, state)
    return state


def inverse_permutation(state, rc, mds_inv, r_f, r_p):
    """undoes `permutation`: fifth roots by the exponent 5^-1 mod (r - 1)"""
    t = len(state)
    root = pow(5, -1, R - 1)
    state = list(state)
    for r in reversed(range(r_f + r_p)):
        state = matvec(mds_inv, state)
        is_full = r < r_f // 2 or r >= r_f // 2 + r_p
        for j in range(t if is_full else 1):
            state[j] = pow(state[j], root, R)
        for j in range(t):
            state[j] = (state[j] - rc[r][j]) % R
    return state


def digest(message, rc, mds, r_f, r_p):
    rate = len(message)
    assert len(mds) == rate + 1
    return permutation(list(message) + [rate << 64], rc, mds, r_f, r_p)[0]


def sum_tree(leaves, rc, mds, r_f, r_p):
    """leaves: [(hash, balance)] -> list of levels, each a list of (hash, balance); the last level is [root]"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([(digest([below[2 * i][0], below[2 * i][1], below[2 * i + 1][0], below[2 * i + 1][1]], rc, mds, r_f, r_p),
                        (below[2 * i][1] + below[2 * i + 1][1]) % R) for i in range(len(below) // 2)])
    return levels


def plain_tree(leaves, rc, mds, r_f, r_p):
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([digest([below[2 * i], below[2 * i + 1]], rc, mds, r_f, r_p) for i in range(len(below) // 2)])
    return levels


def to_words(values):
    """canonical integers -> rows of 4 little-endian u64 Montgomery words (radix 2^256)"""
    import numpy as np
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (v % R) * (1 << 256) % R
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_words(words):
    import numpy as np
    w = np.asarray(words).view(np.uint64).reshape(-1, 4)
    rinv = pow(1 << 256, -1, R)
    return [sum(int(row[k]) << (64 * k) for k in range(4)) * rinv % R for row in w]
