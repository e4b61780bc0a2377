"""The canonical XYZZ group law (zolt_amd/csrc/xyzz.hip.h) held to big integers: the affine arithmetic of BN254 G1 (tests/lazy_model.py) and
G2 (tests/g2_model.py), the records of zg_selftest_xyzz (zolt_amd/csrc/xyzz_selftest.hip.h) with the representative (l^2 x, l^3 y, l^2, l^3) of
every XYZZ operand chosen here, and the checker of what comes back. Shared by tests/test_xyzz_group_law_host.py (the header compiled for the
CPU), tests/test_xyzz_mutants_host.py (the same with one line of a header changed) and tests/test_gpu_xyzz_group_law.py (the device).

A field value is an int (Fp) or a pair of ints (Fp2), never in Montgomery form: pack and the checker convert. A point is (x, y) or None for the
identity. An item is (kind, a, b, scalar, flags, want): a and b are lists of four field values (x, y, zz, zzz; an affine operand uses the first
two), want is the expected group element, or the expected words for the ops compared word for word. Plain module: no fixtures, no hooks."""
import os
import random
import shutil
import subprocess

import numpy as np

from tests import g2_model as M
from tests import lazy_model as lm

P, R = M.P, M.R
RINV = pow(M.MONT, -1, P)
(DBL_AFFINE, DBL, MADD, ADD, NEG, TO_AFFINE, SCALAR_MUL, AXPY, INV) = range(9)
OP_NAMES = ["dbl_affine", "dbl", "madd", "add", "neg", "to_affine", "scalar_mul", "axpy", "inv"]
P_INF, A_INF, B_INF, OUT_IS_B, OUT_IS_A, NO_OUT_INF, CHAINED = 1, 1, 2, 1 << 4, 2 << 4, 1 << 6, 1 << 8  # xyzz_selftest.hip.h: XS_*
G1, G2 = 0, 1


class _Fp:
    W, zero, one = 4, 0, 1
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    neg = staticmethod(lambda a: -a % P)
    inv = staticmethod(lambda a: pow(a, -1, P) if a else 0)
    rand = staticmethod(lambda rng: rng.randrange(1, P))
    words = staticmethod(lambda v: M.fp_limbs(v))
    unwords = staticmethod(lambda w: M._unlimbs(w) * RINV % P)
    canonical = staticmethod(lambda w: M._unlimbs(w) < P)


class _Fp2:
    W, zero, one = 8, (0, 0), (1, 0)
    add, sub, mul, neg, inv = staticmethod(M.f2_add), staticmethod(M.f2_sub), staticmethod(M.f2_mul), staticmethod(M.f2_neg), staticmethod(M.f2_inv)
    rand = staticmethod(lambda rng: (rng.randrange(1, P), rng.randrange(1, P)))
    words = staticmethod(lambda v: M.fp_limbs(v[0]) + M.fp_limbs(v[1]))
    unwords = staticmethod(lambda w: (M._unlimbs(w[:4]) * RINV % P, M._unlimbs(w[4:]) * RINV % P))
    canonical = staticmethod(lambda w: M._unlimbs(w[:4]) < P and M._unlimbs(w[4:]) < P)


class Group:
    def __init__(self, gid):
        self.gid, self.name = gid, ("g1", "g2")[gid]
        self.F = (_Fp, _Fp2)[gid]
        mod = (lm, M)[gid]
        self.G, self.add, self.double, self.neg = mod.G, mod.add, mod.double, mod.neg
        self.W = self.F.W
        self.IN_WORDS, self.OUT_WORDS = 8 * self.W + 6, 4 * self.W + 2
        # how the group's reference writes an identity: G1 (0, 0), G2 (0, (one, 0))
        self.identity_words = [0] * 8 if gid == G1 else list(M.IDENTITY_WORDS)

    # Jacobian double-and-add, one inversion at the end (dbl-2009-l, madd-2007-bl shapes); complete
    def _jdbl(self, p):
        F = self.F
        X, Y, Z = p
        if Z == F.zero or Y == F.zero:
            return (F.one, F.one, F.zero)
        A, B = F.mul(X, X), F.mul(Y, Y)
        C = F.mul(B, B)
        t = F.sub(F.sub(F.mul(F.add(X, B), F.add(X, B)), A), C)
        D = F.add(t, t)
        E = F.add(F.add(A, A), A)
        X3 = F.sub(F.mul(E, E), F.add(D, D))
        c8 = F.add(C, C)
        c8 = F.add(c8, c8)
        c8 = F.add(c8, c8)
        yz = F.mul(Y, Z)
        return (X3, F.sub(F.mul(E, F.sub(D, X3)), c8), F.add(yz, yz))

    def _jmadd(self, p, q):
        F = self.F
        X, Y, Z = p
        if Z == F.zero:
            return (q[0], q[1], F.one)
        zz = F.mul(Z, Z)
        H = F.sub(F.mul(q[0], zz), X)
        r = F.sub(F.mul(q[1], F.mul(zz, Z)), Y)
        if H == F.zero:
            return self._jdbl(p) if r == F.zero else (F.one, F.one, F.zero)
        hh = F.mul(H, H)
        hhh = F.mul(H, hh)
        v = F.mul(X, hh)
        X3 = F.sub(F.sub(F.mul(r, r), hhh), F.add(v, v))
        return (X3, F.sub(F.mul(r, F.sub(v, X3)), F.mul(Y, hhh)), F.mul(Z, H))

    def mul(self, p, s):
        """[s] p for any integer s >= 0 (s is not reduced: the walk may pass through the identity, as the device's does)"""
        F = self.F
        if p is None or s == 0:
            return None
        acc = (F.one, F.one, F.zero)
        for bit in bin(s)[2:]:
            acc = self._jdbl(acc)
            if bit == "1":
                acc = self._jmadd(acc, p)
        X, Y, Z = acc
        if Z == F.zero:
            return None
        zi = F.inv(Z)
        zi2 = F.mul(zi, zi)
        return (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi)))

    def on_curve(self, p):
        return lm.on_curve(p) if self.gid == G1 else M.is_on_curve(p)

    def rep(self, p, lam):
        """the XYZZ representative of p with Z = lam"""
        F = self.F
        l2 = F.mul(lam, lam)
        l3 = F.mul(l2, lam)
        return [F.mul(p[0], l2), F.mul(p[1], l3), l2, l3]

    def affine_words(self, p):
        return self.identity_words if p is None else self.F.words(p[0]) + self.F.words(p[1])


GROUPS = [Group(G1), Group(G2)]


class Gen:
    def __init__(self, grp, seed):
        self.g, self.rng = grp, random.Random(seed)

    def point(self):
        return self.g.mul(self.g.G, self.rng.randrange(2, 1 << 20))

    def lam(self):
        return self.g.F.rand(self.rng)

    def rep(self, p, lam=None):
        return self.g.rep(p, self.lam() if lam is None else lam)

    def one_rep(self, p):
        return self.g.rep(p, self.g.F.one)

    def identity(self):
        """zz == 0 with non-zero garbage in x, y and zzz"""
        F = self.g.F
        return [F.rand(self.rng), F.rand(self.rng), F.zero, F.rand(self.rng)]

    def aff(self, p):
        return [p[0], p[1], self.g.F.zero, self.g.F.zero]

    def garbage_aff(self):
        F = self.g.F
        return [F.rand(self.rng), F.rand(self.rng), F.zero, F.zero]


def _zeros(grp):
    return [grp.F.zero] * 4


def _into(fam):
    def deco(f):
        fam[f.__name__] = f
        return f
    return deco


# ---- the families of each op: name -> builder(gen) -> (a, b, scalar, flags, want)
def _add_families(grp):
    fam = {}
    add, neg, dbl = grp.add, grp.neg, grp.double

    def two(g):
        p, q = g.point(), g.point()
        while q[0] == p[0]:
            q = g.point()
        return p, q

    @_into(fam)
    def regular(g):
        p, q = two(g)
        return g.rep(p), g.rep(q), 0, 0, add(p, q)

    @_into(fam)
    def regular_one(g):  # one side fresh from an affine point
        p, q = two(g)
        return g.one_rep(p), g.rep(q), 0, 0, add(p, q)

    @_into(fam)
    def identity_a(g):
        q = g.point()
        return g.identity(), g.rep(q), 0, 0, q

    @_into(fam)
    def identity_b(g):
        p = g.point()
        return g.rep(p), g.identity(), 0, 0, p

    @_into(fam)
    def identity_both(g):
        return g.identity(), g.identity(), 0, 0, None

    @_into(fam)
    def same_same_rep(g):
        p = g.point()
        r = g.rep(p)
        return r, list(r), 0, 0, dbl(p)

    @_into(fam)
    def same_other_rep(g):
        p = g.point()
        return g.rep(p), g.rep(p), 0, 0, dbl(p)

    @_into(fam)
    def same_one_rep_a(g):
        p = g.point()
        return g.one_rep(p), g.rep(p), 0, 0, dbl(p)

    @_into(fam)
    def same_one_rep_b(g):
        p = g.point()
        return g.rep(p), g.one_rep(p), 0, 0, dbl(p)

    @_into(fam)
    def opposite_same_rep(g):
        p = g.point()
        lam = g.lam()
        return g.rep(p, lam), g.rep(neg(p), lam), 0, 0, None

    @_into(fam)
    def opposite_other_rep(g):
        p = g.point()
        return g.rep(p), g.rep(neg(p)), 0, 0, None

    @_into(fam)
    def opposite_one_rep(g):
        p = g.point()
        return g.rep(p), g.one_rep(neg(p)), 0, 0, None

    @_into(fam)
    def chained_regular(g):
        p, q = two(g)
        return g.rep(p), g.rep(q), 0, CHAINED, add(add(p, q), q)

    @_into(fam)
    def chained_double(g):  # a == b: (2 b) + b
        p = g.point()
        return g.rep(p), g.rep(p), 0, CHAINED, add(dbl(p), p)

    @_into(fam)
    def chained_through_identity(g):  # a == -b: identity + b
        p = g.point()
        return g.rep(neg(p)), g.rep(p), 0, CHAINED, p

    @_into(fam)
    def chained_to_identity(g):  # a == -2 b: (-b) + b, the first sum in whatever representative the addition gives it
        p = g.point()
        return g.rep(neg(dbl(p))), g.rep(p), 0, CHAINED, None

    @_into(fam)
    def chained_to_double(g):  # a the identity: (identity + b) + b, a doubling of b's own representative
        p = g.point()
        return g.identity(), g.rep(p), 0, CHAINED, dbl(p)

    return fam


def _madd_families(grp):
    fam = {}
    add, neg, dbl = grp.add, grp.neg, grp.double

    @_into(fam)
    def acc_identity(g):
        p = g.point()
        return g.identity(), g.aff(p), 0, 0, p

    @_into(fam)
    def regular(g):
        p, q = g.point(), g.point()
        while q[0] == p[0]:
            q = g.point()
        return g.rep(p), g.aff(q), 0, 0, add(p, q)

    @_into(fam)
    def regular_zz_one(g):
        p, q = g.point(), g.point()
        while q[0] == p[0]:
            q = g.point()
        return g.one_rep(p), g.aff(q), 0, 0, add(p, q)

    @_into(fam)
    def same(g):
        p = g.point()
        return g.rep(p), g.aff(p), 0, 0, dbl(p)

    @_into(fam)
    def opposite(g):
        p = g.point()
        return g.rep(neg(p)), g.aff(p), 0, 0, None

    @_into(fam)
    def same_zz_one(g):
        p = g.point()
        return g.one_rep(p), g.aff(p), 0, 0, dbl(p)

    @_into(fam)
    def opposite_zz_one(g):
        p = g.point()
        return g.one_rep(neg(p)), g.aff(p), 0, 0, None

    return fam


def _dbl_families(grp, affine):
    F = grp.F

    def regular(g):
        p = g.point()
        return (g.aff(p) if affine else g.rep(p)), _zeros(grp), 0, 0, grp.double(p)

    def raw_y0(g):
        # not a group element: y == 0 has order two, and the groups have odd prime order. The header's statement is the expectation:
        # "doubling a point with y = 0 gives zz = 0 = the identity"
        x = F.rand(g.rng)
        if affine:
            return [x, F.zero, F.zero, F.zero], _zeros(grp), 0, 0, None
        lam = g.lam()
        l2 = F.mul(lam, lam)
        return [F.mul(x, l2), F.zero, l2, F.mul(l2, lam)], _zeros(grp), 0, 0, None

    fam = {"regular": regular, "raw_y0": raw_y0}
    if not affine:
        fam["identity"] = lambda g: (g.identity(), _zeros(grp), 0, 0, None)
        fam["regular_zz_one"] = lambda g: (lambda p: (g.one_rep(p), _zeros(grp), 0, 0, grp.double(p)))(g.point())
    return fam


def _neg_families(grp):
    fam = {}
    @_into(fam)
    def regular(g):
        p = g.point()
        return g.rep(p), _zeros(grp), 0, 0, grp.neg(p)

    @_into(fam)
    def identity(g):
        return g.identity(), _zeros(grp), 0, 0, None

    return fam


def _to_affine_families(grp):
    fam = {}
    @_into(fam)
    def identity(g):
        return g.identity(), _zeros(grp), 0, 0, (grp.affine_words(None), 1)

    @_into(fam)
    def zz_one(g):
        p = g.point()
        return g.one_rep(p), _zeros(grp), 0, 0, (grp.affine_words(p), 0)

    @_into(fam)
    def general(g):
        p = g.point()
        return g.rep(p), _zeros(grp), 0, 0, (grp.affine_words(p), 0)

    return fam


ALL_BUT_BIT_255 = (1 << 255) - 1  # only bit 31 of limb 7 clear
SCALARS = ([("s%d" % s, s) for s in (0, 1, 2, 3)] + [("r-1", R - 1), ("r-2", R - 2)] +
           [("2^%d" % k, 1 << k) for k in (32, 64, 96, 128, 160, 192, 224, 253)] +
           [("2^%d-1" % k, (1 << k) - 1) for k in (32, 64, 96, 128, 160, 192, 224, 253)] +
           [("all-but-bit-255", ALL_BUT_BIT_255), ("limb0", 0xdeadbeef), ("limb0-top-bit", 0x80000001), ("limb7", 0x12345678 << 224),
            ("limb7-bit-0", 1 << 224), ("limb7-top-bit", 1 << 255)])


def _scalar_mul_families(grp):
    fam = {}
    for name, s in SCALARS:
        def f(g, s=s):
            p = g.point()
            return g.aff(p), _zeros(grp), s, 0, grp.mul(p, s)
        fam[name] = f

    def p_inf(g):
        return g.garbage_aff(), _zeros(grp), g.rng.randrange(1, R), P_INF, None

    def uniform(g):
        p, s = g.point(), g.rng.randrange(1, R)
        return g.aff(p), _zeros(grp), s, 0, grp.mul(p, s)

    fam["p_inf"], fam["uniform"] = p_inf, uniform
    return fam


def _axpy_families(grp):
    add, neg, mul = grp.add, grp.neg, grp.mul

    def small(g):
        return g.rng.randrange(2, 1 << 24)  # the loop runs all 256 bits whatever s is; a short s keeps the model quick

    def case(g, a, b, s, flags):
        """a, b points or None (the flag set, garbage coordinates)"""
        want = add(mul(a, s), b)
        fl = flags | (A_INF if a is None else 0) | (B_INF if b is None else 0)
        status = 0xAA if fl & NO_OUT_INF else (1 if want is None else 0)
        return (g.garbage_aff() if a is None else g.aff(a)), (g.garbage_aff() if b is None else g.aff(b)), s, fl, (grp.affine_words(want), status)

    fam = {
        "inf_none": lambda g: case(g, g.point(), g.point(), small(g), 0),
        "inf_a": lambda g: case(g, None, g.point(), small(g), 0),
        "inf_b": lambda g: case(g, g.point(), None, small(g), 0),
        "inf_both": lambda g: case(g, None, None, small(g), 0),
        "s_zero": lambda g: case(g, g.point(), g.point(), 0, 0),
        "s_zero_b_inf": lambda g: case(g, g.point(), None, 0, 0),
        "full_scalar": lambda g: case(g, g.point(), g.point(), g.rng.randrange(1, R), 0),
        "out_is_b": lambda g: case(g, g.point(), g.point(), small(g), OUT_IS_B),
        "out_is_a": lambda g: case(g, g.point(), g.point(), small(g), OUT_IS_A),
        "out_is_b_identity": lambda g: case(g, None, None, small(g), OUT_IS_B),
        "no_out_inf": lambda g: case(g, g.point(), g.point(), small(g), NO_OUT_INF),
        "no_out_inf_identity": lambda g: case(g, None, None, small(g), NO_OUT_INF),
    }

    def cancels(g):  # s a == -b
        a, s = g.point(), small(g)
        return case(g, a, neg(mul(a, s)), s, 0)

    def doubles(g):  # s a == b
        a, s = g.point(), small(g)
        return case(g, a, mul(a, s), s, 0)

    def cancels_in_place(g):
        a, s = g.point(), small(g)
        return case(g, a, neg(mul(a, s)), s, OUT_IS_B)

    fam.update(cancels=cancels, doubles=doubles, cancels_in_place=cancels_in_place)
    return fam


def inv_structured(mod=P):
    """the values of tests/test_gpu_field.py::test_inversion_variants_on_structured_values, as raw 256-bit patterns below the modulus"""
    vals = [0, 1, 2, 3, 4, 7, 255, 256, mod - 1, mod - 2, mod - 3, (mod - 1) // 2, (mod + 1) // 2, (1 << 253) % mod, (1 << 253) - 1,
            (1 << 254) % mod, (1 << 255) % mod, (1 << 128), (1 << 128) - 1, (1 << 192) + 1, (1 << 64), (1 << 32), (1 << 30),
            (1 << 60) - 1, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, ((1 << 256) - 1) % mod]
    vals += [(1 << k) % mod for k in range(1, 254, 7)] + [((1 << k) + 1) % mod for k in range(29, 254, 30)]
    return vals


def families(grp, op):
    return {DBL_AFFINE: lambda: _dbl_families(grp, True), DBL: lambda: _dbl_families(grp, False), MADD: lambda: _madd_families(grp),
            ADD: lambda: _add_families(grp), NEG: lambda: _neg_families(grp), TO_AFFINE: lambda: _to_affine_families(grp),
            SCALAR_MUL: lambda: _scalar_mul_families(grp), AXPY: lambda: _axpy_families(grp)}[op]()


# the families the issue names, by the names above; records_for asserts that each is present
REQUIRED = {
    ADD: ["regular", "identity_a", "identity_b", "identity_both", "same_same_rep", "same_other_rep", "same_one_rep_a", "same_one_rep_b",
          "opposite_same_rep", "opposite_other_rep", "opposite_one_rep", "chained_regular", "chained_double", "chained_through_identity",
          "chained_to_identity", "chained_to_double"],
    MADD: ["acc_identity", "regular", "same", "opposite", "same_zz_one", "opposite_zz_one"],
    DBL: ["regular", "identity", "raw_y0"],
    DBL_AFFINE: ["regular", "raw_y0"],
    NEG: ["regular", "identity"],
    TO_AFFINE: ["identity", "zz_one", "general"],
    SCALAR_MUL: ["p_inf", "uniform"] + [name for name, _ in SCALARS],
    AXPY: ["inf_none", "inf_a", "inf_b", "inf_both", "s_zero", "cancels", "doubles", "out_is_b", "out_is_a", "no_out_inf"],
    INV: ["structured-raw", "structured-mont", "random"],
}

_CACHE = {}


def records_for(gid, op, seed, n):
    """n items of an op, the families taken in turn so that every wave holds every branch. Cached: the items are never changed."""
    key = (gid, op, seed, n)
    if key in _CACHE:
        return _CACHE[key]
    grp = GROUPS[gid]
    g = Gen(grp, seed * 1000 + 10 * op + gid)
    items = []
    if op == INV:
        items = inv_records(grp, g, n)
    else:
        fam = families(grp, op)
        while len(items) < n:
            for name in fam:
                if len(items) < n:
                    items.append((name,) + tuple(fam[name](g)))
    kinds = {it[0] for it in items}
    assert set(REQUIRED[op]) <= kinds, (OP_NAMES[op], sorted(set(REQUIRED[op]) - kinds))
    _CACHE[key] = items
    return items


def inv_records(grp, g, n):
    """fe_inv_safegcd: the structured values as raw patterns and as Montgomery images, then uniform values. Fp2 inverts its norm: the
    structured value sits in either component, and in both"""
    F, items = grp.F, []

    def put(kind, v):
        items.append((kind, [v, F.zero, F.zero, F.zero], _zeros(grp), 0, 0, (F.words(F.inv(v)) + [0] * (3 * F.W), 0)))

    for kind, conv in (("structured-raw", lambda w: w * RINV % P), ("structured-mont", lambda w: w)):
        vals = inv_structured()
        for j, w in enumerate(vals):
            v = conv(w)
            if grp.gid == G1:
                put(kind, v)
            else:
                put(kind, (v, 0))
                put(kind, (0, v))
                put(kind, (v, conv(vals[(j + 1) % len(vals)])))
    assert len(items) <= n, (len(items), n)
    while len(items) < n:
        put("random", F.rand(g.rng) if g.rng.random() < 0.9 else (g.rng.randrange(1, 1 << 64) if grp.gid == G1 else (g.rng.randrange(1, 1 << 64), 0)))
    return items


def pack(grp, items):
    out = np.zeros((len(items), grp.IN_WORDS), dtype=np.uint64)
    W, F = grp.W, grp.F
    for row, (_, a, b, s, flags, _want) in zip(out, items):
        for k in range(4):
            row[W * k:W * (k + 1)] = F.words(a[k])
            row[W * (4 + k):W * (5 + k)] = F.words(b[k])
        row[8 * W:8 * W + 4] = M._limbs(s)
        row[8 * W + 4] = flags
    return out


def check(grp, op, items, out):
    """every record of `out` against the model: group elements as X / ZZ, Y / ZZZ with ZZ^3 == ZZZ^2, ZZ != 0 and the identity flag; the
    ops that write affine coordinates (TO_AFFINE, AXPY, INV) word for word, the way each group writes an identity included"""
    F, W = grp.F, grp.W
    out = np.asarray(out, dtype=np.uint64)
    assert out.shape == (len(items), grp.OUT_WORDS), (out.shape, len(items))
    for i, (it, row) in enumerate(zip(items, out)):
        kind, want = it[0], it[5]
        what = f"{grp.name} {OP_NAMES[op]} record {i} ({kind})"
        row = [int(x) for x in row]
        status, pad = row[4 * W], row[4 * W + 1]
        assert pad == 0, what
        if op in (TO_AFFINE, AXPY, INV):
            words, flag = want
            assert row[:len(words)] == list(words), f"{what}: words"
            assert not any(row[len(words):4 * W]), f"{what}: words past the result"
            assert status == flag, f"{what}: status {status:#x}, expected {flag:#x}"
            continue
        c = [row[W * k:W * (k + 1)] for k in range(4)]
        assert all(F.canonical(w) for w in c), f"{what}: a coordinate is not below p"
        x, y, zz, zzz = (F.unwords(w) for w in c)
        if want is None:
            assert zz == F.zero, f"{what}: expected the identity, zz != 0"
            assert status == 1, f"{what}: identity flag {status}"
            continue
        assert zz != F.zero, f"{what}: zz == 0, expected a point"
        assert status == 0, f"{what}: identity flag {status}"
        assert F.mul(F.mul(zz, zz), zz) == F.mul(zzz, zzz), f"{what}: zz^3 != zzz^2"
        assert F.mul(x, F.inv(zz)) == want[0], f"{what}: x"
        assert F.mul(y, F.inv(zzz)) == want[1], f"{what}: y"


ALL_OPS = (DBL_AFFINE, DBL, MADD, ADD, NEG, TO_AFFINE, SCALAR_MUL, AXPY)
COUNTS = {DBL_AFFINE: 128, DBL: 256, MADD: 256, ADD: 320, NEG: 128, TO_AFFINE: 192, SCALAR_MUL: 256, AXPY: 256}
INV_RANDOM = 1 << 16


def inv_total(gid):
    """the structured values (raw and Montgomery; three placements over Fp2) and 2^16 uniform ones"""
    return 2 * len(inv_structured()) * (1 if gid == G1 else 3) + INV_RANDOM


# ---- the host harness (tests/cpp/xyzz_host.cpp): the kernels' own headers compiled for the CPU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MAX_RECORDS = 1 << 16  # of one call, host and device


def compile_host(exe, include_first=None, extra=()):
    """-> run(gid, op, items) -> (n, OUT_WORDS) uint64. include_first: a directory of headers that stands in for zolt_amd/csrc (one of them changed)"""
    inc = ["-I", include_first or os.path.join(ROOT, "zolt_amd", "csrc")]
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *extra, *inc, os.path.join(ROOT, "tests", "cpp", "xyzz_host.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)

    def run(gid, op, items):
        grp, outs = GROUPS[gid], []
        for lo in range(0, len(items), MAX_RECORDS):
            part = items[lo:lo + MAX_RECORDS]
            res = subprocess.run([exe], input=f"{gid} {op} {len(part)}\n".encode() + pack(grp, part).tobytes(), capture_output=True, check=True)
            outs.append(np.frombuffer(res.stdout, dtype=np.uint64).reshape(len(part), grp.OUT_WORDS))
        return np.concatenate(outs)

    return run
