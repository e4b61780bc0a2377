"""A Python big-integer model of the BN254 optimal ate pairing as the reference's Dory prover computes it (src/field/pairing.zig,
src/poly/commitment/dory.zig:673-690) — the checker of tests/test_gpu_pairing.py, pinned by tests/test_pairing_model.py.

Fp12 is held flat: six Fp2 coefficients of w with w^6 = xi = 9 + u. The reference's tower Fp12 = Fp6[w]/(w^2 - v), Fp6 = Fp2[v]/(v^3 - xi)
maps onto it by c0.c_i -> w^(2i), c1.c_i -> w^(2i+1). Fp2 and the G2 law come from g2_model. Plain module: no fixtures, no pytest hooks."""
import numpy as np

from tests import g2_model as g2m
from tests.g2_model import MONT, P, R, G, f2_add, f2_sub, f2_neg, f2_mul, f2_sqr, f2_inv, fp_limbs, _unlimbs  # noqa: F401

X = 4965661367192848881  # BN_X (pairing.zig:1697)
XI = (9, 1)
G1_GEN = (1, 2)  # the G1 generator the reference pairs in its own test (pairing.zig:2193, 2203)

ZERO = ((0, 0),) * 6
ONE = ((1, 0),) + ((0, 0),) * 5


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


# ---- Fp12 = Fp2[w] / (w^6 - xi) (the values of pairing.zig:279-620)
def mul(a, b):
    t = [(0, 0)] * 11
    for i, x in enumerate(a):
        if x == (0, 0):
            continue
        for j, y in enumerate(b):
            if y != (0, 0):
                t[i + j] = f2_add(t[i + j], f2_mul(x, y))
    return tuple(f2_add(t[k], f2_mul(t[k + 6], XI)) if k < 5 else t[k] for k in range(6))


def sqr(a):
    return mul(a, a)


def conj(a):  # Fp12.conjugate: c1 -> -c1, the odd powers of w; = a^(p^6)
    return tuple(f2_neg(x) if k & 1 else x for k, x in enumerate(a))


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = sqr(a)
        e >>= 1
    return r


# w^(p - 1) = xi^((p - 1) / 6): (c w^k)^p = conj(c) * GAMMA[k] * w^k
GAMMA = [f2_pow(XI, k * (P - 1) // 6) for k in range(6)]


def frobenius(a, n=1):  # frobenius / frobenius2 / frobenius3: a^(p^n)
    for _ in range(n):
        a = tuple(f2_mul(f2_conj(x), GAMMA[k]) for k, x in enumerate(a))
    return a


def inv(a):
    """a^-1 through the norms Fp12 -> Fp6 -> Fp2 (the value of Fp12.inverse, pairing.zig:586-614); inverse(0) -> 0 (null there)"""
    c = conj(a)
    n6 = mul(a, c)  # in Fp6: even powers of w only
    n6b = mul(frobenius(n6, 2), frobenius(n6, 4))
    n2 = mul(n6, n6b)  # in Fp2
    s = f2_inv(n2[0])
    return tuple(f2_mul(x, s) for x in mul(c, n6b))


def mul_by_034(f, c0, c3, c4):  # fp12MulBy034 (pairing.zig:1156-1189): the sparse element c0 + c3 w + c4 v w = c0 + c3 w + c4 w^3
    return mul(f, (c0, c3, (0, 0), c4, (0, 0), (0, 0)))


def exp_by_x(f):  # expByX (:1786-1800)
    return power(f, X)


# ---- the Miller loop (millerLoopArkworks, :1561-1628)
def naf(n):
    """the non-adjacent form, LSB first, except that a leading 3 stays (1, 1): the digit count is then the bit length of n, which is the
    form arkworks' ATE_LOOP_COUNT has"""
    out = []
    while n:
        if n == 3:
            return out + [1, 1]
        d = 0
        if n & 1:
            d = 2 - (n & 3)
            n -= d
        out.append(d)
        n >>= 1
    return out


ATE_LOOP_COUNT = naf(6 * X + 2)  # 65 signed digits, LSB first (:1288-1298)
TWO_INV = pow(2, -1, P)
TWIST_MUL_BY_Q_X = GAMMA[2]  # xi^((p-1)/3) (:1062-1072)
TWIST_MUL_BY_Q_Y = GAMMA[3]  # xi^((p-1)/2) (:1074-1084)


def _scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def _double_in_place(r):  # :948-997 -> (point, (c0, c1, c2))
    x, y, z = r
    a = _scale(f2_mul(x, y), TWO_INV)
    b, c = f2_sqr(y), f2_sqr(z)
    e = f2_mul(g2m.B_TWIST, f2_add(f2_add(c, c), c))
    f = f2_add(f2_add(e, e), e)
    g = _scale(f2_add(b, f), TWO_INV)
    h = f2_sub(f2_sqr(f2_add(y, z)), f2_add(b, c))
    i = f2_sub(e, b)
    j = f2_sqr(x)
    e2 = f2_sqr(e)
    pt = (f2_mul(a, f2_sub(b, f)), f2_sub(f2_sqr(g), f2_add(f2_add(e2, e2), e2)), f2_mul(b, h))
    return pt, (f2_neg(h), f2_add(f2_add(j, j), j), i)


def _add_in_place(r, q):  # :1001-1032
    x, y, z = r
    theta = f2_sub(y, f2_mul(q[1], z))
    lam = f2_sub(x, f2_mul(q[0], z))
    c, d = f2_sqr(theta), f2_sqr(lam)
    e = f2_mul(lam, d)
    f = f2_mul(z, c)
    g = f2_mul(x, d)
    h = f2_sub(f2_add(e, f), f2_add(g, g))
    pt = (f2_mul(lam, h), f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, y)), f2_mul(z, e))
    return pt, (lam, f2_neg(theta), f2_sub(f2_mul(theta, q[0]), f2_mul(lam, q[1])))


def mul_by_char(q):  # :1088-1100
    return (f2_mul(f2_conj(q[0]), TWIST_MUL_BY_Q_X), f2_mul(f2_conj(q[1]), TWIST_MUL_BY_Q_Y))


def _ell(f, coeffs, p):  # the line at P: c0 * y_P at w^0, c1 * x_P at w^1, c2 at w^3 (:1586-1589)
    return mul_by_034(f, _scale(coeffs[0], p[1]), _scale(coeffs[1], p[0]), coeffs[2])


def miller_loop(p, q):
    """p = (x, y) in Fp or None, q a g2_model point or None -> the unreduced Miller value"""
    if p is None or q is None:
        return ONE
    r = (q[0], q[1], (1, 0))
    neg_q = g2m.neg(q)
    f = ONE
    for idx in range(len(ATE_LOOP_COUNT) - 1, 0, -1):
        if idx != len(ATE_LOOP_COUNT) - 1:
            f = sqr(f)
        r, co = _double_in_place(r)
        f = _ell(f, co, p)
        bit = ATE_LOOP_COUNT[idx - 1]
        if bit:
            r, co = _add_in_place(r, q if bit == 1 else neg_q)
            f = _ell(f, co, p)
    q1 = mul_by_char(q)
    r, co = _add_in_place(r, q1)
    f = _ell(f, co, p)
    q2 = g2m.neg(mul_by_char(q1))
    r, co = _add_in_place(r, q2)
    return _ell(f, co, p)


# ---- the final exponentiation (finalExponentiation :1653-1681, hardPartExponentiationArkworks :1812-1880)
HARD_C = 2 * X * (6 * X * X + 3 * X + 1)
HARD_EXPONENT = HARD_C * ((P ** 4 - P ** 2 + 1) // R)  # what the chain below realises, modulo the order p^4 - p^2 + 1 of its input
FINAL_EXPONENT = (P ** 6 - 1) * (P ** 2 + 1) * HARD_EXPONENT


def _exp_by_neg_x(f):  # :1804-1808
    return conj(exp_by_x(f))


def hard_part(r):  # :1812-1880, step by step
    y0 = _exp_by_neg_x(r)
    y1 = sqr(y0)
    y2 = sqr(y1)
    y3 = mul(y2, y1)
    y4 = _exp_by_neg_x(y3)
    y5 = sqr(y4)
    y6 = _exp_by_neg_x(y5)
    y3 = conj(y3)
    y6 = conj(y6)
    y7 = mul(y6, y4)
    y8 = mul(y7, y3)
    y9 = mul(y8, y1)
    y10 = mul(y8, y4)
    y11 = mul(y10, r)
    y12 = frobenius(y9)
    y13 = mul(y12, y11)
    y8 = frobenius(y8, 2)
    y14 = mul(y8, y13)
    y15 = frobenius(mul(conj(r), y9), 3)
    return mul(y15, y14)


def final_exponentiation(f):
    if f == ZERO:  # :1654-1656; a non-zero element of the field Fp12 is always invertible (:1664 cannot trigger)
        return ONE
    r = mul(conj(f), inv(f))  # f^(p^6 - 1)
    r = mul(frobenius(r, 2), r)  # ^(p^2 + 1)
    return hard_part(r)


def pairing(p, q):  # pairingFp (:1276-1286)
    if p is None or q is None:
        return ONE
    return final_exponentiation(miller_loop(p, q))


def multi_pairing(ps, qs):
    """multiPairG1G2 (dory.zig:673-690): the product of the pairings of min(len) pairs — here as ONE final exponentiation of the product
    of the Miller values, with a zero Miller value counted as one as the per-pair finalExponentiation would"""
    m = ONE
    for p, q in zip(ps, qs):
        v = miller_loop(p, q)
        m = mul(m, ONE if v == ZERO else v)
    return final_exponentiation(m)


# ---- G1 over Fp (affine; only what the tests need to build operands)
def g1_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def g1_neg(a):
    return None if a is None else (a[0], -a[1] % P)


def g1_mul(a, s):
    r = None
    for bit in bin(s)[2:] if s else "":
        r = g1_add(r, r)
        if bit == "1":
            r = g1_add(r, a)
    return r


# ---- layouts: Fp12.toBytes (pairing.zig:624-690) and the ABI's 48-word GT element, both in the order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2
TOWER_ORDER = (0, 2, 4, 1, 3, 5)  # the power of w at each of the six Fp2 places


def to_bytes(f):
    return b"".join(f[k][0].to_bytes(32, "little") + f[k][1].to_bytes(32, "little") for k in TOWER_ORDER)


def from_bytes(b):
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(12)]
    f = [None] * 6
    for i, k in enumerate(TOWER_ORDER):
        f[k] = (v[2 * i], v[2 * i + 1])
    return tuple(f)


def gt_pack(elems):
    """[Fp12] -> (n, 48) uint64 Montgomery limbs"""
    return np.array([[w for k in TOWER_ORDER for c in f[k] for w in fp_limbs(c)] for f in elems], dtype=np.uint64).reshape(-1, 48)


def gt_unpack(arr):
    inv_m = pow(MONT, -1, P)
    out = []
    for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 48):
        v = [_unlimbs(row[4 * i:4 * i + 4]) * inv_m % P for i in range(12)]
        f = [None] * 6
        for i, k in enumerate(TOWER_ORDER):
            f[k] = (v[2 * i], v[2 * i + 1])
        out.append(tuple(f))
    return out


def g1_pack(points):
    """[(x, y) or None] -> (xy (n, 8) uint64, inf (n,) uint8); an identity is written x = y = 0"""
    xy = np.zeros((len(points), 8), dtype=np.uint64)
    inf = np.zeros(len(points), dtype=np.uint8)
    for i, p in enumerate(points):
        if p is None:
            inf[i] = 1
        else:
            xy[i] = fp_limbs(p[0]) + fp_limbs(p[1])
    return xy, inf


def g1_unpack(xy, inf):
    inv_m = pow(MONT, -1, P)
    out = []
    for row, f in zip(np.asarray(xy, dtype=np.uint64).reshape(-1, 8), np.asarray(inf).reshape(-1)):
        out.append(None if f else (_unlimbs(row[:4]) * inv_m % P, _unlimbs(row[4:]) * inv_m % P))
    return out
