"""The wave pairing engine's decomposition (zolt_amd/csrc/fp12_wave_map.hip.h, fp12_wave.hip.h, pairing_wave.hip.h) restated in Python
integers over 64 simulated lanes, for tests/test_pairing_wave_model.py to hold to tests/pairing_model.py.

An Fp12 is a list of 64 Fp2 values, lane L holding the coefficient of w^(L % 6). A product: lane L = 6 i + j (the 36 busy lanes) forms
a_i * b_j with a_i fetched from lane i, multiplies it by xi where i + j >= 6, and every lane of column k sums the six lanes
(t, (k - t) mod 6). A Miller step's Fp2 products are grouped in levels; product s of a level is formed by lane 36 + s only, and a level
may share its instructions with an Fp12 product (mul_side). Plain module: no fixtures, no pytest hooks."""
from tests import g2_model as g2m
from tests import pairing_model as M
from tests.g2_model import P, f2_add, f2_sub, f2_neg, f2_mul

LANES, DEG, BUSY, SIDE0 = 64, 6, 36, 36
ZERO2 = (0, 0)


# ---- the lane map (fp12_wave_map.hip.h)
def col(lane):
    return lane % DEG


def row(lane):
    return (lane // DEG) % DEG


def busy(lane):
    return lane < BUSY


def xi(lane):
    return row(lane) + col(lane) >= DEG


def src(c, t):
    return DEG * t + (c + DEG - t) % DEG


def sparse_slot(c):
    return {0: 0, 1: 1, 3: 2}.get(c, -1)


def mem_slot(c):
    return (c & 1) * 3 + (c >> 1)


DBL_PRODUCTS, ADD_PRODUCTS = (5, 3, 4), (2, 6, 3, 4)


# ---- an Fp12 over the lanes
def spread(f):
    """a pairing_model element -> its 64 lane values"""
    return [f[col(L)] for L in range(LANES)]


def collect(w):
    """lanes 0..5 hold the element (the lanes fpw_store writes); every other lane of a column must agree with them"""
    assert all(w[L] == w[col(L)] for L in range(LANES))
    return tuple(w[:DEG])


def _gather(t):
    t = [f2_mul(v, M.XI) if xi(L) else v for L, v in enumerate(t)]
    out = []
    for L in range(LANES):
        s = t[src(col(L), 0)]
        for k in range(1, DEG):
            s = f2_add(s, t[src(col(L), k)])
        out.append(s)
    return out


def mul(a, b):
    return _gather([f2_mul(a[row(L)], b[L]) for L in range(LANES)])


def mul_side(a, b, u, v):
    """a * b in the busy lanes and u[L] * v[L] in the others -> (the product, every lane's raw product)"""
    t = [f2_mul(a[row(L)], b[L]) if busy(L) else f2_mul(u[L], v[L]) for L in range(LANES)]
    return _gather(t), t


def sqr(a):
    return mul(a, a)


def line(c0, c3, c4):
    return [(c0, c3, c4)[sparse_slot(col(L))] if sparse_slot(col(L)) >= 0 else ZERO2 for L in range(LANES)]


def mul_by_034(f, c0, c3, c4):
    return mul(f, line(c0, c3, c4))


# ---- the Miller loop (pairing_wave.hip.h): R, P and Q replicated, product s of a level in lane 36 + s
def half(a):
    return tuple((c + P if c & 1 else c) >> 1 for c in a)  # a conditional addition of p and a shift (on the Montgomery form in the kernel)


def _pick(*ops):
    """lane 36 + s gets ops[s]; every other lane ops[0]"""
    return [ops[L - SIDE0] if 0 <= L - SIDE0 < len(ops) else ops[0] for L in range(LANES)]


def _level(us, vs):
    t = [f2_mul(u, v) for u, v in zip(_pick(*us), _pick(*vs))]
    return [t[SIDE0 + s] for s in range(len(us))]


def _times3(a):
    return f2_add(f2_add(a, a), a)


def miller_loop(p, q):
    px, py = (p[0], 0), (p[1], 0)
    x, y, z = q[0], q[1], (1, 0)
    f = spread(M.ONE)
    qc = q
    for idx in range(64, -2, -1):
        dbl = idx >= 1
        if dbl:
            yz = f2_add(y, z)
            f, t = mul_side(f, f, _pick(x, y, z, yz, x), _pick(y, y, z, yz, x))
            xy, b, c, yz2, j = (t[SIDE0 + s] for s in range(5))
            h = f2_sub(yz2, f2_add(b, c))
            e, l0, l1 = _level((_times3(c), f2_neg(h), _times3(j)), (g2m.B_TWIST, py, px))
            a, f3 = half(xy), _times3(e)
            g = half(f2_add(b, f3))
            e2, nx, gg, nz = _level((e, a, g, b), (e, f2_sub(b, f3), g, h))
            x, y, z = nx, f2_sub(gg, _times3(e2)), nz
            ln = line(l0, l1, f2_sub(e, b))
            digit = M.ATE_LOOP_COUNT[idx - 1]
            add = digit != 0
            qa = q if digit >= 0 else g2m.neg(q)
        else:
            qc = M.mul_by_char(qc)
            add, qa = True, (qc if idx == 0 else g2m.neg(qc))
        u0 = _pick(qa[1], qa[0])
        if dbl:
            f, t = mul_side(f, ln, u0, [z] * LANES)
        else:
            t = [f2_mul(u, z) for u in u0]
        if not add:
            continue
        theta, lam = f2_sub(y, t[SIDE0]), f2_sub(x, t[SIDE0 + 1])
        c, d, tq, lq, l0, l1 = _level((theta, lam, theta, lam, lam, f2_neg(theta)), (theta, lam, qa[0], qa[1], py, px))
        ln = line(l0, l1, f2_sub(tq, lq))
        e, ff, g = _level((lam, z, x), (d, c, d))
        h = f2_sub(f2_add(e, ff), f2_add(g, g))
        nx, ty, ey, nz = _level((lam, theta, e, z), (h, f2_sub(g, h), y, e))
        x, y, z = nx, f2_sub(ty, ey), nz
        f = mul(f, ln)
    return collect(f)


# ---- the final exponentiation (pairing_wave.hip.h, pairw_final_exp): every product the 36-product form, a square the product of a
# value with itself; conjugation and the Frobenius maps act on each lane's own coefficient, the inverse is the tower's
def conj(a):
    return [f2_neg(v) if col(L) & 1 else v for L, v in enumerate(a)]


def frobenius(a, n):
    for _ in range(n):
        a = [f2_mul(M.f2_conj(v), M.GAMMA[col(L)]) for L, v in enumerate(a)]
    return a


def exp_by_x(a):
    r = None
    for bit in bin(M.X)[2:]:
        if r is not None:
            r = mul(r, r)
        if bit == "1":
            r = a if r is None else mul(r, a)
    return r


def final_exponentiation(f):
    """a pairing_model element -> its final exponentiation, pairw_final_exp's chain step for step"""
    if f == M.ZERO:
        return M.ONE
    a = spread(f)
    t = mul(conj(a), spread(M.inv(f)))
    r = mul(frobenius(t, 2), t)
    t = conj(exp_by_x(r))  # y0
    y1 = mul(t, t)
    t = mul(y1, y1)  # y2
    y3 = mul(t, y1)
    y4 = conj(exp_by_x(y3))
    t = mul(y4, y4)  # y5
    y6 = exp_by_x(t)
    y3 = conj(y3)
    t = mul(y6, y4)  # y7
    y8 = mul(t, y3)
    y9 = mul(y8, y1)
    t = mul(y8, y4)  # y10
    t = mul(t, r)  # y11
    y1 = frobenius(y9, 1)  # y12
    t = mul(y1, t)  # y13
    y8 = frobenius(y8, 2)
    t = mul(y8, t)  # y14
    y9 = frobenius(mul(conj(r), y9), 3)  # y15
    return collect(mul(y9, t))
