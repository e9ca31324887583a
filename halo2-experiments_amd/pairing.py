"""The optimal ate pairing on BN256 in Python integers: what ``verify_proof`` needs for its one final check, and nothing faster
than that.  Fq2 = Fq[u] / (u^2 + 1) (``kzg``'s helpers), Fq6 = Fq2[v] / (v^3 - xi) with xi = 9 + u, Fq12 = Fq6[w] / (w^2 - v); G2 lives
on the D-type twist y^2 = x^3 + 3 / xi and is untwisted by (x, y) -> (x w^2, y w^3).  The Miller loop runs over 6 x + 2 for the
curve parameter x = 4965661367192848881 in affine twist coordinates (a line through T with twist slope m, evaluated at P in G1, is
y_P - m x_P w + (m x_T - y_T) w^3; vertical lines and Fq factors die in the final exponentiation), then takes the two Frobenius
lines; the final exponentiation is the easy part by conjugation and Frobenius and the hard part (p^4 - p^2 + 1) / r by plain
square-and-multiply.  One pairing takes well under a second; a check of several pairs shares the final exponentiation.

Also here: G1 on host integers (affine tuples, ``None`` = identity) for the verifier's small MSM.  Checked by tests/test_pairing.py
through bilinearity, non-degeneracy and e(P, Q)^r = 1, which no wrong Miller loop or exponent survives."""
from __future__ import annotations

from .bn256 import FQ_MODULUS, FR_MODULUS
from .kzg import G2_GENERATOR, _fq2_inv, _fq2_mul, _fq2_sub, g2_on_curve

P = FQ_MODULUS
R = FR_MODULUS
BN_X = 4965661367192848881
ATE_LOOP = 6 * BN_X + 2
G1_GEN = (1, 2)
XI = (9, 1)

# ---- G1 on integers ------------------------------------------------------------------------------------------------------------------


def g1_on_curve(p) -> bool:
    return p is None or (p[1] * p[1] - p[0] * p[0] * p[0] - 3) % P == 0


def g1_neg(p):
    return None if p is None else (p[0], -p[1] % P)


def g1_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x3 = (lam * lam - p[0] - q[0]) % P
    return (x3, (lam * (p[0] - x3) - p[1]) % P)


def _jac_double(t):
    x, y, z = t
    if y == 0:
        return (1, 1, 0)
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return (x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P)


def _jac_add_affine(t, q):
    x, y, z = t
    if z == 0:
        return (q[0], q[1], 1)
    zz = z * z % P
    u2, s2 = q[0] * zz % P, q[1] * zz % P * z % P
    if u2 == x:
        return _jac_double(t) if s2 == y else (1, 1, 0)
    h, r = (u2 - x) % P, (s2 - y) % P
    hh = h * h % P
    hhh, v = hh * h % P, x * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - y * hhh) % P, z * h % P)


def g1_mul(k: int, p=G1_GEN):
    """[k mod r] p by double-and-add in Jacobian coordinates (one inversion at the end)"""
    if p is None:
        return None
    acc = (1, 1, 0)
    for bit in bin(k % R)[2:]:
        acc = _jac_double(acc)
        if bit == "1":
            acc = _jac_add_affine(acc, p)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, P)
    return (acc[0] * zi * zi % P, acc[1] * zi * zi % P * zi % P)


def g1_msm(scalars, points):
    """sum_i scalars[i] * points[i] on host integers (the verifier's few dozen terms)."""
    acc = None
    for k, p in zip(scalars, points):
        acc = g1_add(acc, g1_mul(k, p))
    return acc


# ---- the tower -------------------------------------------------------------------------------------------------------------------------
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def _f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def _f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def _f2_conj(a):
    return (a[0], -a[1] % P)


def _f2_mul_xi(a):
    return ((9 * a[0] - a[1]) % P, (a[0] + 9 * a[1]) % P)


def _f2_pow(a, e: int):
    acc = F2_ONE
    for bit in bin(e)[2:]:
        acc = _fq2_mul(acc, acc)
        if bit == "1":
            acc = _fq2_mul(acc, a)
    return acc


F6_ZERO, F6_ONE = (F2_ZERO, F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO, F2_ZERO)


def _f6_add(a, b):
    return (_f2_add(a[0], b[0]), _f2_add(a[1], b[1]), _f2_add(a[2], b[2]))


def _f6_sub(a, b):
    return (_fq2_sub(a[0], b[0]), _fq2_sub(a[1], b[1]), _fq2_sub(a[2], b[2]))


def _f6_neg(a):
    return (_f2_neg(a[0]), _f2_neg(a[1]), _f2_neg(a[2]))


def _f6_mul(a, b):
    m = _fq2_mul
    c0 = _f2_add(m(a[0], b[0]), _f2_mul_xi(_f2_add(m(a[1], b[2]), m(a[2], b[1]))))
    c1 = _f2_add(_f2_add(m(a[0], b[1]), m(a[1], b[0])), _f2_mul_xi(m(a[2], b[2])))
    c2 = _f2_add(_f2_add(m(a[0], b[2]), m(a[1], b[1])), m(a[2], b[0]))
    return (c0, c1, c2)


def _f6_mul_v(a):
    return (_f2_mul_xi(a[2]), a[0], a[1])


def _f6_inv(a):
    m = _fq2_mul
    t0 = _fq2_sub(m(a[0], a[0]), _f2_mul_xi(m(a[1], a[2])))
    t1 = _fq2_sub(_f2_mul_xi(m(a[2], a[2])), m(a[0], a[1]))
    t2 = _fq2_sub(m(a[1], a[1]), m(a[0], a[2]))
    d = _fq2_inv(_f2_add(m(a[0], t0), _f2_mul_xi(_f2_add(m(a[2], t1), m(a[1], t2)))))
    return (m(t0, d), m(t1, d), m(t2, d))


F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    t0, t1 = _f6_mul(a[0], b[0]), _f6_mul(a[1], b[1])
    mid = _f6_sub(_f6_sub(_f6_mul(_f6_add(a[0], a[1]), _f6_add(b[0], b[1])), t0), t1)
    return (_f6_add(t0, _f6_mul_v(t1)), mid)


def f12_conj(a):
    """a^(p^6)"""
    return (a[0], _f6_neg(a[1]))


def f12_inv(a):
    d = _f6_inv(_f6_sub(_f6_mul(a[0], a[0]), _f6_mul_v(_f6_mul(a[1], a[1]))))
    return (_f6_mul(a[0], d), _f6_neg(_f6_mul(a[1], d)))


def f12_pow(a, e: int):
    acc = F12_ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


# w^p = w * xi^((p - 1) / 6): the coefficient of w^i picks up GAMMA[i] under Frobenius
GAMMA = [_f2_pow(XI, i * (P - 1) // 6) for i in range(6)]


def f12_frobenius(a):
    """a^p.  In the basis 1, w, .., w^5 the coefficients are a0.c0, a1.c0, a0.c1, a1.c1, a0.c2, a1.c2."""
    (a0, a1, a2), (b0, b1, b2) = a
    g = GAMMA
    c = _f2_conj
    return ((c(a0), _fq2_mul(c(a1), g[2]), _fq2_mul(c(a2), g[4])),
            (_fq2_mul(c(b0), g[1]), _fq2_mul(c(b1), g[3]), _fq2_mul(c(b2), g[5])))


def _line(t, m, p):
    """y_P - m x_P w + (m x_T - y_T) w^3 as an Fq12 element"""
    c1 = _f2_neg((m[0] * p[0] % P, m[1] * p[0] % P))
    c3 = _fq2_sub(_fq2_mul(m, t[0]), t[1])
    return (((p[1] % P, 0), F2_ZERO, F2_ZERO), (c1, c3, F2_ZERO))


def _g2_step(t, q):
    """(the twist slope of the line through t and q -- the tangent when they are equal --, t + q); slope None for a vertical line"""
    if t[0] == q[0]:
        if t[1] != q[1] or t[1] == F2_ZERO:
            return None, None
        m = _fq2_mul(_fq2_mul((3, 0), _fq2_mul(t[0], t[0])), _fq2_inv(_fq2_mul((2, 0), t[1])))
    else:
        m = _fq2_mul(_fq2_sub(q[1], t[1]), _fq2_inv(_fq2_sub(q[0], t[0])))
    x3 = _fq2_sub(_fq2_sub(_fq2_mul(m, m), t[0]), q[0])
    return m, (x3, _fq2_sub(_fq2_mul(m, _fq2_sub(t[0], x3)), t[1]))


def _g2_frobenius(q):
    return (_fq2_mul(_f2_conj(q[0]), GAMMA[2]), _fq2_mul(_f2_conj(q[1]), GAMMA[3]))


def miller_loop(p, q):
    """f_{6x+2, Q}(P) times the two Frobenius lines, before the final exponentiation; 1 when either point is the identity."""
    if p is None or q is None:
        return F12_ONE
    f, t = F12_ONE, q
    for bit in bin(ATE_LOOP)[3:]:
        m, t2 = _g2_step(t, t)
        f = f12_mul(f12_mul(f, f), _line(t, m, p))
        t = t2
        if bit == "1":
            m, t2 = _g2_step(t, q)
            f = f12_mul(f, _line(t, m, p))
            t = t2
    q1 = _g2_frobenius(q)
    q2 = _g2_frobenius(q1)
    nq2 = (q2[0], _f2_neg(q2[1]))
    m, t2 = _g2_step(t, q1)
    f = f12_mul(f, _line(t, m, p))
    m, _ = _g2_step(t2, nq2)
    return f12_mul(f, _line(t2, m, p))


HARD_EXPONENT = (P ** 4 - P ** 2 + 1) // R
assert (P ** 4 - P ** 2 + 1) % R == 0


def final_exponentiation(f):
    """f^((p^12 - 1) / r) = ((f^(p^6 - 1))^(p^2 + 1))^((p^4 - p^2 + 1) / r)"""
    f = f12_mul(f12_conj(f), f12_inv(f))
    f = f12_mul(f12_frobenius(f12_frobenius(f)), f)
    return f12_pow(f, HARD_EXPONENT)


def pairing(p, q=G2_GENERATOR):
    """e(P, Q) for P in G1 (an (x, y) tuple of integers) and Q in G2 (``kzg``'s ((x0, x1), (y0, y1))); None is the identity."""
    if not g1_on_curve(p) or not g2_on_curve(q):
        raise ValueError("pairing: a point is not on its curve")
    return final_exponentiation(miller_loop(p, q))


def pairing_check(pairs) -> bool:
    """prod_i e(P_i, Q_i) == 1, with one shared final exponentiation"""
    f = F12_ONE
    for p, q in pairs:
        if not g1_on_curve(p) or not g2_on_curve(q):
            return False
        f = f12_mul(f, miller_loop(p, q))
    return final_exponentiation(f) == F12_ONE
