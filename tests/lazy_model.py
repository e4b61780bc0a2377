"""A Python big-integer model of the MSM's lazy 29-bit-limb arithmetic (zolt_amd/csrc/fp29.hip.h) and of BN254 G1, a generator of
IN-CLASS worst-case records for zg_selftest_lazy_g1 (zolt_amd/csrc/lazy_selftest.hip.h), and the checker of what comes back. Shared by
tests/test_gpu_lazy_group_law.py (the device) and tests/test_lazy_group_law_host.py (the same headers compiled for the CPU).

Every bound below is quoted from the headers with its line; this file invents none. A record is 91 u32 in (ten operands of nine raw
limbs, a flags word) and 146 u32 out (sixteen results, a status word, an aux word). Plain module: no fixtures, no pytest hooks."""
import random
from fractions import Fraction

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
B = 3  # y^2 = x^3 + 3
G = (1, 2)
MONT = 1 << 261  # fp29.hip.h:10 "Montgomery form with R' = 2^261"
MONT_INV = pow(MONT, -1, P)
MASK = (1 << 29) - 1
NEAR = (1 << 29) + 8  # fp29.hip.h:13 'Limbs are "near-normalised" (< 2^29 + 8) except the top limb'
IN_WORDS, OUT_WORDS = 91, 146

MADD, START, ADD, DBL, JDBL, PROD, LIN, MADD4, ADD4, DBL4 = range(10)
OP_NAMES = ["madd", "start", "add", "dbl", "jdbl", "prod", "lin", "madd4", "add4", "dbl4"]
(LIN_SUB2, LIN_SUB4, LIN_SUB7, LIN_PMSUB_POS, LIN_PMSUB_NEG, LIN_NEG2, LIN_NEG4, LIN_X3, LIN_SUB4_2C, LIN_TIMES2, LIN_TIMES3, LIN_TIMES4,
 LIN_TO_FP, LIN_IS_ZERO) = range(14)


def kp(k):
    """the integer bound k * p for a decimal k of the headers (exact: k is a Fraction)"""
    return int(Fraction(k) * P)


# ---- the class table, g1_29.hip.h:6-15 (and :115 "X < 6.6p, Y < 1.4p, ZZ, ZZZ < 1.6p"; :151 for the Jacobian doubling)
ROW = kp("1.1")      # :7  point x, y < 1.1 p (table rows)
NEG_Y = kp(2)        # :7  negated y = 2p - y <= 2p: the y of a run-start accumulator (fp29.hip.h:445 "b <= 2p")
MUL_OUT = kp("1.6")  # :8  M (mul output) < 1.6 p
ACC_X = kp("6.6")    # :9  acc.x < 6.6 p
ACC_Y = kp("1.4")    # :10 acc.y < 1.4 p
CLS_P = kp("8.6")    # :11 P = U2 + 7p - X1 < 8.6 p; Q + 7p - X3 < 8.6 p
CLS_R = kp("5.6")    # :11 R = S2 + 4p - Y1 < 5.6 p
DBL_X = kp("5.6")    # :141 r.x = f29_sub4_2c(f29_sqr(M), S);   // < 5.6p
JAC_X, JAC_Y, JAC_Z = kp("5.3"), kp("1.3"), kp("1.1")  # :151 X < 5.3p, Y < 1.3p, Z < 1.1p (closed under jac29_dbl)
NEG4_OUT = kp(4)      # g1_29.hip.h:10 the second product of Y3 is (4p - Y1) * PPP: f29_neg4 outputs are <= 4p
ZERO_DOMAIN = 16     # fp29.hip.h:511 "x < 16p", and the filter of :515 (k > 16 is refused)
TO_FP_IN = kp(16)    # fp29.hip.h:565 "lazy (value < 16p) -> canonical"
MUL_DEN = Fraction("168.9")  # fp29.hip.h:12 inputs < A*p and < B*p give a product < (A*B/168.9 + 1)*p


def mul_bound(*ab):
    """fp29.hip.h:12 and :128: ((A*B [+ C*D]) / 168.9 + 1) * p for operand class bounds given as integers"""
    s = sum(Fraction(a, P) * Fraction(b, P) for a, b in ab)
    return int((s / MUL_DEN + 1) * P)


# ---- G1, affine; None is the identity
def neg(p):
    return None if p is None else (p[0], -p[1] % P)


def double(p):
    if p is None or p[1] == 0:
        return None
    lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    x3 = (lam * lam - 2 * p[0]) % P
    return (x3, (lam * (p[0] - x3) - p[1]) % P)


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        return double(p) if p[1] == q[1] else None
    lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x3 = (lam * lam - p[0] - q[0]) % P
    return (x3, (lam * (p[0] - x3) - p[1]) % P)


def on_curve(p):
    return p is None or (p[1] * p[1] - p[0] ** 3 - B) % P == 0


# ---- limbs
def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def limbs(v):
    """the exact encoding: limbs 0..7 < 2^29, the top limb keeps the rest"""
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def to_mont(v):
    return v * MONT % P


def from_mont(v):
    return v * MONT_INV % P


def near_encodings(v, keep0, limit=None):
    """every near-normalised encoding of v: a limb <= 7 becomes + 2^29 with the next limb decremented (limb 0 stays exact if keep0).
    The exact one comes first. Most values have no other; small multiples of 2^29i have many."""
    out = [limbs(v)]
    seen = {tuple(out[0])}
    todo = [out[0]]
    while todo and (limit is None or len(out) < limit):
        cur = todo.pop()
        for i in range(1 if keep0 else 0, 8):
            if cur[i] <= 7 and cur[i + 1] >= 1 and (i + 1 == 8 or cur[i + 1] - 1 < NEAR):
                nxt = list(cur)
                nxt[i] += 1 << 29
                nxt[i + 1] -= 1
                if tuple(nxt) not in seen:
                    seen.add(tuple(nxt))
                    out.append(nxt)
                    todo.append(nxt)
    return out


def sqrt_mod(a):  # p = 3 mod 4
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


_CB_M = P - 1
while _CB_M % 3 == 0:
    _CB_M //= 3
_CB_K = pow(3, -1, _CB_M)


def cbrt_mod(a):
    """a cube root for the cubes whose order is prime to 3 (one element in (p - 1) / m of the cubes): callers retry"""
    if pow(a, _CB_M, P) != 1:
        return None
    r = pow(a, _CB_K, P)
    assert pow(r, 3, P) == a % P
    return r


# ---- the generator
class Gen:
    """in-class operands from a seeded stream; points come from the chain P_{i+1} = P_i + G"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.cur = add(double(G), G)

    def point(self):
        self.cur = add(self.cur, G)
        return self.cur

    def rep(self, v, bound, mode):
        """a representative of v (mod p) below `bound`: "zero" = v itself, "top" = the largest, "rand" = any, or an integer j"""
        jmax = (bound - 1 - v) // P
        j = {"zero": 0, "top": jmax}.get(mode, mode) if mode != "rand" else self.rng.randint(0, jmax)
        assert 0 <= j <= jmax
        return v + j * P

    def enc(self, v, keep0):
        e = near_encodings(v, keep0, limit=4)
        return e[self.rng.randrange(len(e))]

    def forced(self, bound, keep0):
        """raw limbs first: limbs 0..7 from {2^29 - 1, 2^29 + 7, 2^29 + r, r}, the top limb the largest that stays below `bound`"""
        r = self.rng
        lo = []
        for i in range(8):
            c = [MASK, r.getrandbits(29)] if (i == 0 and keep0) else [MASK, (1 << 29) + 7, (1 << 29) + r.randrange(8), r.getrandbits(29)]
            lo.append(r.choice(c))
        top = (bound - 1 - val(lo)) >> 232
        return lo + [top]

    def row(self, pt, mode="zero"):
        """a table row: x, y < 1.1p with exact limbs (f29_unpack outputs)"""
        out = []
        for c in pt:
            v = to_mont(c)
            out.append(limbs(self.rep(v, ROW, mode if v + P < ROW else "zero")))
        return out

    def acc(self, pt, xmode="rand", ymode="rand", zmode="rand", force=None, ybound=ACC_Y):
        """an accumulator (x, y, zz, zzz as limbs) for the affine point pt, with zz = z^2, zzz = z^3. force in (None, "x", "y", "zz", "zzz"):
        that coordinate's limbs are chosen first (Gen.forced) and z is solved for, retrying where no root exists."""
        ax, ay = pt
        while True:
            fl = None
            if force == "x":
                fl = self.forced(ACC_X, True)
                z = sqrt_mod(from_mont(val(fl)) * pow(ax, -1, P) % P)
            elif force == "y":
                fl = self.forced(ybound, False)
                z = cbrt_mod(from_mont(val(fl)) * pow(ay, -1, P) % P)
            elif force == "zz":
                fl = self.forced(MUL_OUT, False)
                z = sqrt_mod(from_mont(val(fl)))
            elif force == "zzz":
                fl = self.forced(MUL_OUT, False)
                z = cbrt_mod(from_mont(val(fl)))
            else:
                z = self.rng.randrange(1, P)
            if z:
                break
        zz, zzz = z * z % P, z * z * z % P
        vals = [to_mont(ax * zz % P), to_mont(ay * zzz % P), to_mont(zz), to_mont(zzz)]
        out = [self.enc(self.rep(vals[0], ACC_X, xmode), True), self.enc(self.rep(vals[1], ybound, ymode), False),
               self.enc(self.rep(vals[2], MUL_OUT, zmode), False), self.enc(self.rep(vals[3], MUL_OUT, zmode), False)]
        if force:
            k = ["x", "y", "zz", "zzz"].index(force)
            assert val(fl) % P == vals[k]
            out[k] = fl
        return out

    def run_start(self, pt, negated):
        """the accumulator xyzz29_start leaves: (px, py or 2p - py, one, one); y <= 2p"""
        x, y = self.row(pt)
        if negated:
            y = limbs(2 * P - val(y))
        one = limbs(MONT % P)
        return [x, y, one, one]


def acc_point(c):
    """(x, y, zz, zzz) limbs -> the affine point, None for the identity encoding (zz all-zero limbs, g1_29.hip.h:114)"""
    if not any(c[2]):
        return None
    x, y, zz, zzz = (from_mont(val(l)) for l in c)
    assert zz and zzz
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


IDENTITY = [[0] * 9] * 4


def record(ops, flags=0):
    r = np.zeros(IN_WORDS, dtype=np.uint32)
    for i, l in enumerate(ops):
        assert len(l) == 9 and all(0 <= int(x) < 1 << 32 for x in l)
        r[9 * i:9 * i + 9] = l
    r[90] = flags
    return r


def branch(kind):
    """the branch a record takes, from its kind: what one wave must hold side by side"""
    for b in ("double", "infinity", "identity", "start"):
        if b in kind and not kind.startswith("run-start"):
            return b
    return "regular"


def _round_robin(lists):
    lists = [list(reversed(l)) for l in lists if l]
    out = []
    while lists:
        for l in lists:
            out.append(l.pop())
        lists = [l for l in lists if l]
    return out


def interleave(groups, seed, run=64):
    """[(kind, record, ...)] lists per kind -> one list in which the branches sit side by side: round-robin over the kinds of a branch,
    round-robin over the branches, then a seeded shuffle inside each run of `run` records (64: one wave of single-lane records; 16: the
    sixteen adjacent quads of one wave)"""
    rng = random.Random(seed)
    by_branch = {}
    for g in groups:
        if g:
            by_branch.setdefault(branch(g[0][0]), []).append(g)
    out = _round_robin([_round_robin(gs) for gs in by_branch.values()])
    for s in range(0, len(out), run):
        blk = out[s:s + run]
        rng.shuffle(blk)
        out[s:s + run] = blk
    return out


# ---- record sets. Every item is (kind, record, expectation ...); kinds name the branch and the edge a record aims at.
def madd_records(seed, n, quad=False):
    """MADD / MADD4. Expectation: (effective point, accumulator's point). xyzz29_madd4 has no neg and takes the identity flag instead."""
    g = Gen(seed)
    kinds = {}

    def put(kind, acc, q, negf, inf=False):
        a = None if inf else acc_point(acc)
        eff = neg(q) if negf else q
        flags = (1 if negf else 0) | (4 if inf else 0)
        kinds.setdefault(kind, []).append((kind, record((IDENTITY if inf else acc) + g.row(q), flags), eff, a))

    signs = (0,) if quad else (0, 1)
    per = max(1, -(-n // (22 if quad else 44)))
    for _ in range(per):
        for s in signs:
            sg = "-" if s else "+"
            for xm in ("zero", "top", "rand"):
                a = g.point()
                put(f"regular{sg}", g.acc(a, xm, g.rng.choice(["zero", "top", "rand"]), g.rng.choice(["zero", "top", "rand"])), g.point(), s)
            # P = acc and P = -acc, so that the effective point is +-acc under either sign of neg; every representative of acc.x
            for j in range((ACC_X - 1) // P):
                a = g.point()
                put(f"double{sg}", g.acc(a, j), neg(a) if s else a, s)
                put(f"infinity{sg}", g.acc(a, j, "top"), a if s else neg(a), s)
            a = g.point()
            put(f"double{sg}", g.acc(a, "top"), neg(a) if s else a, s)
            for f in ("x", "y", "zz", "zzz"):
                a = g.point()
                put(f"forced-{f}{sg}", g.acc(a, force=f), g.point(), s)
            a = g.point()
            put(f"forced-x-double{sg}", g.acc(a, force="x"), neg(a) if s else a, s)
            a = g.point()
            put(f"forced-x-infinity{sg}", g.acc(a, force="x"), a if s else neg(a), s)
            if not quad:
                a = g.point()
                put(f"run-start{sg}", g.run_start(a, g.rng.random() < 0.5), g.point(), s)
                put(f"forced-y-2p{sg}", _start_like(g), g.point(), s)
        if quad:
            put("start", None, g.point(), 0, inf=True)
    return interleave(list(kinds.values()), seed, 16 if quad else 64)[:n]


def _start_like(g):
    """a run-start accumulator (zz = zzz = one) whose y limbs are forced and <= 2p: the point is solved for instead of z"""
    while True:
        fl = g.forced(NEG_Y + 1, True)  # f29_neg2 is a carry output: limb 0 exact
        y = from_mont(val(fl))
        x = cbrt_mod((y * y - B) % P)
        if x:
            one = limbs(MONT % P)
            return [limbs(to_mont(x)), fl, one, one]


def start_records(seed, n):
    """START: first point (s4, s5) with its neg (flags bit 0), then one madd of a second point (bit 1). Expectation as MADD."""
    g = Gen(seed)
    kinds = {}
    for _ in range(max(1, n // 10)):
        for s1 in (0, 1):
            for s2 in (0, 1):
                a = g.point()
                for kind, q in (("regular", g.point()), ("double", neg(a) if s1 != s2 else a), ("infinity", a if s1 != s2 else neg(a))):
                    k = f"{kind}{'-' if s1 else '+'}{'-' if s2 else '+'}"
                    rec = record(IDENTITY + g.row(a, "top") + g.row(q, "top"), s1 | (s2 << 1))
                    kinds.setdefault(k, []).append((k, rec, neg(q) if s2 else q, neg(a) if s1 else a))
    return interleave(list(kinds.values()), seed)[:n]


def add_records(seed, n, run=64):
    """ADD / ADD4 (a, b) and, with b absent, DBL / DBL4. Expectation: the two points."""
    g = Gen(seed)
    kinds = {}

    def put(kind, a, b):
        kinds.setdefault(kind, []).append((kind, record(a + b), acc_point(a), acc_point(b)))

    modes = ["zero", "top", "rand"]
    for _ in range(max(1, -(-n // 14))):
        r = g.rng
        for xm in modes:
            put("regular", g.acc(g.point(), xm, r.choice(modes), r.choice(modes)), g.acc(g.point(), r.choice(modes), xm, r.choice(modes)))
        a = g.point()
        put("double", g.acc(a, r.choice(modes), r.choice(modes)), g.acc(a, r.choice(modes), r.choice(modes)))
        put("double-same", *(2 * [g.acc(a, "top", "top", "top")]))  # add(a, a)
        put("infinity", g.acc(a, r.choice(modes), "top"), g.acc(neg(a), "top", r.choice(modes)))
        put("identity-a", IDENTITY, g.acc(g.point(), "top", "top", "top"))
        put("identity-b", g.acc(g.point(), "top", "top", "top"), IDENTITY)
        put("identity-both", IDENTITY, IDENTITY)
        for f in ("x", "y", "zz", "zzz"):
            put(f"forced-{f}", g.acc(g.point(), force=f), g.acc(g.point(), force=f))
        put("forced-x-double", g.acc(a, force="x"), g.acc(a, force="x"))
        put("forced-x-infinity", g.acc(a, force="x"), g.acc(neg(a), force="x"))
    return interleave(list(kinds.values()), seed, run)[:n]


def dbl_records(seed, n, run=64):
    g = Gen(seed)
    kinds = {}
    modes = ["zero", "top", "rand"]
    for _ in range(max(1, n // 8)):
        for xm in modes:
            a = g.acc(g.point(), xm, g.rng.choice(modes), g.rng.choice(modes))
            kinds.setdefault("regular", []).append(("regular", record(a), acc_point(a)))
        for f in ("x", "y", "zz", "zzz"):
            a = g.acc(g.point(), force=f)
            kinds.setdefault(f"forced-{f}", []).append((f"forced-{f}", record(a), acc_point(a)))
        kinds.setdefault("identity", []).append(("identity", record(IDENTITY), None))
    return interleave(list(kinds.values()), seed, run)[:n]


def jdbl_records(seed, n):
    """JDBL: (X, Y, Z) with x = X / Z^2, y = Y / Z^3 in the classes of g1_29.hip.h:151. Expectation: the point."""
    g = Gen(seed)
    kinds = {}
    for i in range(n):
        pt = g.point()
        kind = ["zero", "top", "rand", "forced-x", "forced-z", "forced-y"][i % 6]
        while True:
            if kind == "forced-x":
                fl = g.forced(JAC_X, False)
                z = sqrt_mod(from_mont(val(fl)) * pow(pt[0], -1, P) % P)
            elif kind == "forced-y":
                fl = g.forced(JAC_Y, False)
                z = cbrt_mod(from_mont(val(fl)) * pow(pt[1], -1, P) % P)
            elif kind == "forced-z":
                fl = g.forced(JAC_Z, False)
                z = from_mont(val(fl)) % P
            else:
                z = g.rng.randrange(1, P)
            if z:
                break
        vals = [to_mont(pt[0] * z * z % P), to_mont(pt[1] * z * z * z % P), to_mont(z)]
        mode = kind if kind in ("zero", "top") else "rand"
        c = [g.enc(g.rep(v, b, mode), False) for v, b in zip(vals, (JAC_X, JAC_Y, JAC_Z))]
        if kind.startswith("forced"):
            c["xyz".index(kind[-1])] = fl
        kinds.setdefault(kind, []).append((kind, record(c), pt))
    return interleave(list(kinds.values()), seed)[:n]


PROD_CLASSES = (CLS_P, CLS_R, NEG4_OUT, MUL_OUT, ACC_X, MUL_OUT)  # A B C D E F: the class products g1_29.hip.h:10-11 lists —
# 8.6p x 5.6p (+ 4p x 1.6p in the two-product form, "(5.6*8.6 + 4*1.6)/168.9 + 1") and 6.6p x 1.6p (Q = X1 * PP)


def prod_records(seed, n):
    g = Gen(seed)
    kinds = {}
    for i in range(n):
        kind = ["worst", "forced", "rand", "top-exact"][i % 4]
        ops = []
        for b in PROD_CLASSES:
            if kind == "worst":  # all eight low limbs at 2^29 + 7, the top limb at its class maximum
                lo = [(1 << 29) + 7] * 8
                ops.append(lo + [(b - 1 - val(lo)) >> 232])
            elif kind == "forced":
                ops.append(g.forced(b, False))
            elif kind == "top-exact":
                ops.append(limbs(b - 1 - g.rng.randrange(1 << 20)))
            else:
                ops.append(g.enc(g.rng.randrange(b), False))
        kinds.setdefault(kind, []).append((kind, record(ops)))
    return interleave(list(kinds.values()), seed)[:n]


def lin_records(seed, n):
    """LIN: (a, b, c) and the mask of the functions whose stated preconditions the record meets"""
    g = Gen(seed)
    r = g.rng
    fixed, rand = [], []
    bit = lambda *ks: sum(1 << k for k in ks)
    z9 = [0] * 9

    def put(dst, kind, a, b, c, mask):
        dst.append((kind, record([a, b, c], mask)))

    # the zero test: k*p for k = 0..16 in every near-normalised encoding (limb 0 exact), k*p +- 1, k*p +- 2^(29 i), and 17p
    for k in range(0, 18):
        cands = [(f"zero-{k}p", k * P)]
        if k <= 16:
            cands += [(f"near-{k}p", k * P + d) for d in (1, -1)] + [(f"near-{k}p", k * P + s * (1 << (29 * i))) for i in range(1, 9) for s in (1, -1)]
        for kind, v in cands:
            if v < 0:
                continue
            for e in near_encodings(v, True, limit=128):
                mask = bit(LIN_IS_ZERO, LIN_TIMES2, LIN_TIMES3, LIN_TIMES4) | (bit(LIN_TO_FP) if v < TO_FP_IN else 0)
                put(fixed, kind + ("-raised" if e != limbs(v) else ""), e, z9, z9, mask)
    # the subtractions at their stated extremes: subtrahend limbs all 2^29 + 7 / the subtrahend at the top of its class
    hi = [(1 << 29) + 7] * 8
    for a in (z9, limbs(MUL_OUT - 1), hi + [(MUL_OUT - 1 - val(hi)) >> 232], g.forced(MUL_OUT, False)):
        # the subtrahend classes are those of the group law's call sites: U1, S1, py, B < 1.6p under the 2p bias (g1_29.hip.h:95, :166,
        # :179-180, :190), acc.y <= 2p under 4p / 5p (:61, :71, :83), acc.x and X3 < 6.6p under 7p (:60, :83)
        for bound, fn in ((MUL_OUT, bit(LIN_SUB2, LIN_NEG2)), (NEG_Y + 1, bit(LIN_SUB4, LIN_NEG4, LIN_PMSUB_POS, LIN_PMSUB_NEG)), (ACC_X, bit(LIN_SUB7))):
            for b in (hi + [(bound - 1 - val(hi)) >> 232], limbs(bound - 1), g.forced(bound, False)):
                put(fixed, "sub-extreme", a, b, z9, fn)
        # f29_x3 / f29_sub4_2c: "b, c exactly normalised mul outputs" (fp29.hip.h:470, :478)
        for b in (limbs(MUL_OUT - 1), limbs(r.randrange(MUL_OUT))):
            put(fixed, "x3-extreme", a, b, limbs(MUL_OUT - 1), bit(LIN_X3, LIN_SUB4_2C))
            put(fixed, "x3-extreme", a, b, [MASK] * 8 + [((MUL_OUT - 1) >> 232) - 1], bit(LIN_X3, LIN_SUB4_2C))
    # f29_to_fp up to just below 16p
    for v in (TO_FP_IN - 1, TO_FP_IN - P, P, P - 1, 0, 1):
        put(fixed, "to-fp-edge", limbs(v), z9, z9, bit(LIN_TO_FP, LIN_IS_ZERO))
    put(fixed, "to-fp-edge", hi + [(TO_FP_IN - 1 - val(hi)) >> 232], z9, z9, bit(LIN_TO_FP))
    while len(fixed) + len(rand) < n:
        a = g.enc(r.randrange(MUL_OUT), True) if r.random() < 0.5 else limbs(r.randrange(MUL_OUT))
        b = g.forced(NEG_Y + 1, False) if r.random() < 0.5 else g.enc(r.randrange(NEG_Y + 1), False)
        mask = bit(LIN_SUB4, LIN_SUB7, LIN_PMSUB_POS, LIN_PMSUB_NEG, LIN_NEG4, LIN_TIMES2, LIN_TIMES3, LIN_TIMES4, LIN_TO_FP)
        if val(b) < MUL_OUT:
            mask |= bit(LIN_SUB2, LIN_NEG2)
        if a[0] <= MASK:
            mask |= bit(LIN_IS_ZERO)
        c = limbs(r.randrange(MUL_OUT))
        if val(b) < MUL_OUT and all(x <= MASK for x in b[:8]):
            mask |= bit(LIN_X3)
        put(rand, "random", a, b, c, mask | bit(LIN_SUB4_2C))
    return interleave([fixed, rand], seed)[:n]


def pack(items):
    return np.ascontiguousarray(np.stack([it[1] for it in items]), dtype=np.uint32)


def assert_in_class(op, items):
    """the generator's own contract: every operand of every record lies inside the class the headers admit, every limb 0..7 is
    near-normalised, every accumulator is a point of the curve with zz^3 = zzz^2"""
    base = {MADD4: MADD, ADD4: ADD, DBL4: DBL}.get(op, op)
    one = limbs(MONT % P)

    def f(rec, k):
        return [int(x) for x in rec[9 * k:9 * k + 9]]

    def point(rec, k, what):
        c = [f(rec, k + j) for j in range(4)]
        if not any(sum(c, [])):
            return
        start = c[2] == one and c[3] == one  # a run-start accumulator: y <= 2p
        for l, bound in zip(c, (ACC_X, NEG_Y + 1 if start else ACC_Y, MUL_OUT, MUL_OUT)):
            assert val(l) < bound and all(x < NEAR for x in l[:8]), what
        assert c[0][0] <= MASK, what  # acc.x is a carry output
        zz, zzz = from_mont(val(c[2])), from_mont(val(c[3]))
        assert pow(zz, 3, P) == zzz * zzz % P and on_curve(acc_point(c)), what

    def row(rec, k, what):
        x, y = f(rec, k), f(rec, k + 1)
        assert val(x) < ROW and val(y) < ROW and all(v <= MASK for v in x[:8] + y[:8]), what
        assert on_curve((from_mont(val(x)), from_mont(val(y)))), what

    for idx, it in enumerate(items):
        rec, what = it[1], (OP_NAMES[op], idx, it[0])
        if base == MADD:
            if not int(rec[90]) & 4:
                point(rec, 0, what)
            row(rec, 4, what)
        elif base == START:
            row(rec, 4, what)
            row(rec, 6, what)
        elif base in (ADD, DBL):
            point(rec, 0, what)
            if base == ADD:
                point(rec, 4, what)
        elif base == JDBL:
            c = [f(rec, k) for k in range(3)]
            for l, bound in zip(c, (JAC_X, JAC_Y, JAC_Z)):
                assert val(l) < bound and all(x < NEAR for x in l[:8]), what
        elif base == PROD:
            for k, bound in enumerate(PROD_CLASSES):
                assert val(f(rec, k)) < bound and all(x < NEAR for x in f(rec, k)[:8]), what
        else:
            for k in range(3):
                assert all(x < NEAR for x in f(rec, k)[:8]), what


# ---- the checker
class Maxima(dict):
    def see(self, op, coord, v):
        k = f"{OP_NAMES[op]}.{coord}"
        self[k] = max(self.get(k, 0.0), round(v / P, 3))


def _res(out, slot):
    return [int(x) for x in out[9 * slot:9 * slot + 9]]


def _check_limbs(l, carry_output, what):
    """fp29.hip.h:74 mul outputs: "output limbs exactly < 2^29"; :53 carry outputs: "limbs < 2^29 + 8 out", limb 0 masked (:56)"""
    lim = NEAR if carry_output else 1 << 29
    assert l[0] < 1 << 29 and all(x < lim for x in l[1:8]), (what, [hex(x) for x in l])


def _check_point(op, out, base, want, xbound, mx, what, y_carry=False):
    c = [_res(out, base + k) for k in range(4)]
    for name, l, bound, carry in (("x", c[0], xbound, True), ("y", c[1], ACC_Y, y_carry), ("zz", c[2], MUL_OUT, False), ("zzz", c[3], MUL_OUT, False)):
        _check_limbs(l, carry, (what, name))
        assert val(l) < bound, (what, name, val(l) / P)  # inside its stated class
        mx.see(op, name, val(l))
    zz, zzz = from_mont(val(c[2])), from_mont(val(c[3]))
    assert zz and pow(zz, 3, P) == zzz * zzz % P, (what, "zz^3 != zzz^2")
    assert acc_point(c) == want, (what, "group element")
    return c


def check(op, items, out, device):
    """every record of `items` against its row of `out` ((n, 146) u32). Returns the largest value seen per (op, coordinate) / p."""
    out = np.asarray(out, dtype=np.uint32).reshape(len(items), OUT_WORDS)
    mx = Maxima()
    quad = op >= MADD4
    base_op = {MADD4: MADD, ADD4: ADD, DBL4: DBL}.get(op, op)
    for idx, (it, o) in enumerate(zip(items, out)):
        kind, rec = it[0], it[1]
        what = (OP_NAMES[op], idx, kind)
        status, aux = int(o[144]), int(o[145])
        lanes = range(4) if quad else range(1)
        if quad:  # all four lanes return identical limbs
            for q in range(1, 4):
                assert np.array_equal(o[36 * q:36 * q + 36], o[:36]), (what, "lane", q)
            assert status in (0, 15), (what, "lanes disagree on infinity", status)
            status, aux = 0, 1 if status else 0
        if base_op in (MADD, START):
            eff, a = it[2], it[3]
            if a is None:  # MADD4 on the identity: the accumulator becomes the point
                want, exc = eff, 0
            elif a == eff:
                want, exc = double(a), 2
            elif a == neg(eff):
                want, exc = None, 1
            else:
                want, exc = add(a, eff), 0
            if not quad:
                assert status == exc, (what, "exc code", status, exc)
            assert aux == (1 if want is None else 0), (what, "inf flag", aux)
            if want is not None:
                # the run-start form leaves y as it came: a table row (< 1.1p, below the class bound asserted here)
                _check_point(op, o, 0, want, ACC_X, mx, what)
        elif base_op in (ADD, DBL):
            want = add(it[2], it[3]) if base_op == ADD else double(it[2])
            assert aux == (1 if want is None else 0), (what, "identity flag", aux)
            if want is None:
                assert not o[:36].any(), (what, "identity encoding")
            elif base_op == ADD and (it[2] is None or it[3] is None):
                assert np.array_equal(o[:36], rec[36:72] if it[2] is None else rec[:36]), (what, "the other operand, unchanged")
            else:
                # xyzz29_add may double (g1_29.hip.h:182), so its x is the class bound; xyzz29_dbl states its own (:141)
                _check_point(op, o, 0, want, DBL_X if base_op == DBL else ACC_X, mx, what)
        elif op == JDBL:
            c = [_res(o, k) for k in range(3)]
            for name, l, bound, carry in (("x", c[0], JAC_X, True), ("y", c[1], JAC_Y, False), ("z", c[2], JAC_Z, False)):
                _check_limbs(l, carry, (what, name))
                assert val(l) < bound, (what, name, val(l) / P)
                mx.see(op, name, val(l))
            x, y, z = (from_mont(val(l)) for l in c)
            zi = pow(z, -1, P)
            assert (x * zi * zi % P, y * zi * zi * zi % P) == double(it[2]), (what, "group element")
        elif op == PROD:
            A, Bv, C, D, E, F = (val(rec[9 * k:9 * k + 9]) for k in range(6))
            ba, bb, bc, bd, be, bf = PROD_CLASSES
            want = {9: ((A * Bv), mul_bound((ba, bb))), 10: (C * D, mul_bound((bc, bd))), 11: (E * F, mul_bound((be, bf))),
                    12: (A * A, mul_bound((ba, ba))), 13: (C * C, mul_bound((bc, bc))), 14: (A * Bv + C * D, mul_bound((ba, bb), (bc, bd)))}
            for slot, (prod, bound) in want.items():
                l = _res(o, slot)
                _check_limbs(l, False, (what, slot))
                assert val(l) % P == prod * MONT_INV % P, (what, slot, "value")
                assert val(l) < bound, (what, slot, val(l) / P, bound / P)
                mx.see(op, f"r{slot}", val(l))
            assert status == (1 if device else 0), (what, "device forms", status)
            if device:  # the asm forms are bit-identical to the compiler forms (fp29.hip.h:167-168)
                for asm, ref in ((0, 9), (1, 10), (2, 9), (3, 10), (4, 11), (5, 12), (6, 13), (7, 14), (8, 11)):
                    assert _res(o, asm) == _res(o, ref), (what, "asm form", asm, "differs from compiler form", ref)
        elif op == LIN:
            a, b, c = (val(rec[9 * k:9 * k + 9]) for k in range(3))
            mask = int(rec[90])
            exact = {LIN_SUB2: a + 2 * P - b, LIN_SUB4: a + 4 * P - b, LIN_SUB7: a + 7 * P - b, LIN_PMSUB_POS: a + 4 * P - b,
                     LIN_PMSUB_NEG: 5 * P - a - b, LIN_NEG2: 2 * P - b, LIN_NEG4: 4 * P - b, LIN_X3: a + 5 * P - b - 2 * c,
                     LIN_SUB4_2C: a + 4 * P - 2 * c, LIN_TIMES2: 2 * a, LIN_TIMES3: 3 * a, LIN_TIMES4: 4 * a}
            for k, v in exact.items():
                l = _res(o, k)
                if not mask >> k & 1:
                    assert not any(l), (what, k, "not asked for")
                    continue
                _check_limbs(l, True, (what, k))
                assert val(l) == v, (what, k, "value", val(l) / P, v / P)
                mx.see(op, f"r{k}", val(l))
            if mask >> LIN_PMSUB_POS & 1:  # fp29.hip.h:445-446 "the class of R (< 5.6p) holds for both signs"
                assert val(_res(o, LIN_PMSUB_POS)) < CLS_R and val(_res(o, LIN_PMSUB_NEG)) < CLS_R, (what, "class of R")
            if mask >> LIN_TO_FP & 1:  # canonical Montgomery-2^256: the lazy value is x * 2^261, so the words are x * 2^-5 mod p
                got = sum(int(w) << (32 * i) for i, w in enumerate(o[9 * LIN_TO_FP:9 * LIN_TO_FP + 8]))
                assert got == a * pow(32, -1, P) % P, (what, "f29_to_fp")
            if mask >> LIN_IS_ZERO & 1:  # fp29.hip.h:511-515: k * p for k <= 16, nothing else
                assert status == (1 if a % P == 0 and a // P <= ZERO_DOMAIN else 0), (what, "f29_is_zero_modp", status, a / P)
        else:
            raise ValueError(op)
    return mx


def records_for(op, seed, n):
    base = {MADD4: MADD, ADD4: ADD, DBL4: DBL}.get(op, op)
    if base == MADD:
        return madd_records(seed, n, quad=op == MADD4)
    if base in (ADD, DBL):
        return (add_records if base == ADD else dbl_records)(seed, n, 16 if op >= MADD4 else 64)
    return {START: start_records, JDBL: jdbl_records, PROD: prod_records, LIN: lin_records}[base](seed, n)
