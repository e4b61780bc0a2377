"""A Python big-integer model of BN254 G2 as the reference's prover uses it (src/field/pairing.zig:182-272, 749-925;
src/poly/commitment/dory.zig:179-210, 320-370, 693-703) — the checker of tests/test_gpu_g2.py, pinned by tests/test_g2_model.py.

Fp2 elements are pairs of ints (c0, c1) = c0 + c1 u, u^2 = -1; a point is ((x0, x1), (y0, y1)) or None for the identity. The affine
chord-and-tangent law and double-and-add restate G2Point.add / double / scalarMul; a Jacobian double-and-add with one inversion at the
end gives the same points faster and is checked against the affine one. Plain module: no fixtures, no pytest hooks."""
import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256

# G2Point.generator (pairing.zig:774-777)
G = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
     (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


# ---- Fp2
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):  # pairing.zig:212-223
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_inv(a):  # pairing.zig:255-263; inverse(0) is null in the reference, (0, 0) here
    norm = (a[0] * a[0] + a[1] * a[1]) % P
    if norm == 0:
        return (0, 0)
    ni = pow(norm, -1, P)
    return (a[0] * ni % P, -a[1] * ni % P)


B_TWIST = f2_mul((3, 0), f2_inv((9, 1)))  # 3 / (9 + u), dory.zig getG2BTwist


def is_on_curve(p):
    return p is None or f2_sqr(p[1]) == f2_add(f2_mul(f2_sqr(p[0]), p[0]), B_TWIST)


# ---- G2Point, affine (pairing.zig:830-919)
def neg(p):
    return None if p is None else (p[0], f2_neg(p[1]))


def double(p):  # :861-875
    if p is None or p[1] == (0, 0):
        return None
    xx = f2_sqr(p[0])
    lam = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(p[1], p[1])))
    x3 = f2_sub(f2_sub(f2_sqr(lam), p[0]), p[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(p[0], x3)), p[1]))


def add(p, q):  # :839-859
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] == f2_neg(q[1]):
            return None
        return double(p)
    lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x3 = f2_sub(f2_sub(f2_sqr(lam), p[0]), q[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(p[0], x3)), p[1]))


def scalar_mul_affine(p, s):  # :880-919, s the integer the scalar stands for
    if p is None or s == 0:
        return None
    res = None
    for bit in bin(s)[2:]:
        res = double(res)
        if bit == "1":
            res = add(res, p)
    return res


# ---- the same group in Jacobian coordinates (X/Z^2, Y/Z^3), one inversion at the end
def _jdbl(p):
    X, Y, Z = p
    if Z == (0, 0) or Y == (0, 0):
        return ((1, 0), (1, 0), (0, 0))
    A, B = f2_sqr(X), f2_sqr(Y)
    C = f2_sqr(B)
    t = f2_sub(f2_sub(f2_sqr(f2_add(X, B)), A), C)
    D = f2_add(t, t)
    E = f2_add(f2_add(A, A), A)
    X3 = f2_sub(f2_sqr(E), f2_add(D, D))
    c8 = f2_add(C, C)
    c8 = f2_add(c8, c8)
    c8 = f2_add(c8, c8)
    yz = f2_mul(Y, Z)
    return (X3, f2_sub(f2_mul(E, f2_sub(D, X3)), c8), f2_add(yz, yz))


def _jmadd(p, q):  # p Jacobian, q affine and not the identity
    X, Y, Z = p
    if Z == (0, 0):
        return (q[0], q[1], (1, 0))
    zz = f2_sqr(Z)
    H = f2_sub(f2_mul(q[0], zz), X)
    r = f2_sub(f2_mul(q[1], f2_mul(zz, Z)), Y)
    if H == (0, 0):
        return _jdbl(p) if r == (0, 0) else ((1, 0), (1, 0), (0, 0))
    hh = f2_sqr(H)
    hhh = f2_mul(H, hh)
    v = f2_mul(X, hh)
    X3 = f2_sub(f2_sub(f2_sqr(r), hhh), f2_add(v, v))
    return (X3, f2_sub(f2_mul(r, f2_sub(v, X3)), f2_mul(Y, hhh)), f2_mul(Z, H))


def _jaffine(p):
    X, Y, Z = p
    if Z == (0, 0):
        return None
    zi = f2_inv(Z)
    zi2 = f2_sqr(zi)
    return (f2_mul(X, zi2), f2_mul(Y, f2_mul(zi2, zi)))


def scalar_mul(p, s):
    if p is None or s == 0:
        return None
    acc = ((1, 0), (1, 0), (0, 0))
    for bit in bin(s)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jmadd(acc, p)
    return _jaffine(acc)


def msm(points, scalars):  # msmG2, dory.zig:693-703
    res = None
    for p, s in zip(points, scalars):
        res = add(res, scalar_mul(p, s))
    return res


# ---- compressG2 (dory.zig:179-210; fp2IsPositive :320-344 compares c1 first, then c0; equal counts as positive)
def compress(p):
    if p is None:
        return bytes(63) + bytes([0x40])
    out = bytearray(p[0][0].to_bytes(32, "little") + p[0][1].to_bytes(32, "little"))
    y, ny = p[1], f2_neg(p[1])
    positive = (y[1], y[0]) <= (ny[1], ny[0])
    out[63] = (out[63] & 0x3F) | (0 if positive else 0x80)
    return bytes(out)


# ---- Montgomery limb packing: the ABI's layouts
def _limbs(v):
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def _unlimbs(l):
    return sum(int(x) << (64 * i) for i, x in enumerate(l))


def fp_limbs(v):
    return _limbs(v * MONT % P)


def fr_limbs(v):
    return _limbs(v % R * MONT % R)


def fr_pack(vals):
    return np.array([fr_limbs(int(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def fr_unpack(arr):
    inv = pow(MONT, -1, R)
    return [_unlimbs(row) * inv % R for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


def f2_pack(vals):
    """[(c0, c1)] -> (n, 8) Montgomery limbs"""
    return np.array([fp_limbs(a) + fp_limbs(b) for a, b in vals], dtype=np.uint64).reshape(-1, 8)


def f2_unpack(arr):
    inv = pow(MONT, -1, P)
    return [(_unlimbs(row[:4]) * inv % P, _unlimbs(row[4:]) * inv % P) for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 8)]


IDENTITY_WORDS = [0] * 8 + fp_limbs(1) + [0] * 4  # G2Point.identity(): x = 0, y = (one, 0) (pairing.zig:754-760)


def pack(points):
    """[point or None] -> (xy (n, 16) uint64, inf (n,) uint8); an identity is written as G2Point.identity() writes it"""
    xy = np.zeros((len(points), 16), dtype=np.uint64)
    inf = np.zeros(len(points), dtype=np.uint8)
    for i, p in enumerate(points):
        if p is None:
            xy[i], inf[i] = IDENTITY_WORDS, 1
        else:
            xy[i] = fp_limbs(p[0][0]) + fp_limbs(p[0][1]) + fp_limbs(p[1][0]) + fp_limbs(p[1][1])
    return xy, inf


def unpack(xy, inf):
    xy = np.asarray(xy, dtype=np.uint64).reshape(-1, 16)
    inf = np.asarray(inf).reshape(-1)
    out = []
    for row, f in zip(xy, inf):
        if f:
            out.append(None)
        else:
            c = f2_unpack(row.reshape(2, 8))
            out.append((c[0], c[1]))
    return out
