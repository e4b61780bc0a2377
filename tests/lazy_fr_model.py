"""A Python big-integer model of the sumcheck kernels' lazy Fr arithmetic (the Fr side of zolt_amd/csrc/fp29.hip.h) and of their lazy 288-bit
sums (zolt_amd/csrc/acc9.hip.h, sc_common.hip.h), a generator of records AT THE EDGES of the operand classes those headers state in their
comments, and the checker of what comes back from zg_selftest_lazy_fr (zolt_amd/csrc/lazy_fr_selftest.hip.h). Shared by
tests/test_gpu_lazy_fr.py (the device) and tests/test_lazy_fr_host.py (the same headers compiled for the CPU).

Every bound below is quoted from a header comment; this file invents none. A record is 146 u32 in (sixteen slots of nine words, a flags
word, a length word) and 146 u32 out (sixteen slots, a status word, an aux word). Plain module: no fixtures, no pytest hooks."""
import random
from collections import defaultdict
from fractions import Fraction

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # the scalar field's modulus r
ABI = 1 << 256   # table entries: canonical Montgomery-2^256
MONT = 1 << 261  # the lazy multiplier's Montgomery radix (fp29.hip.h: "Montgomery product a*b*2^-261")
MASK = (1 << 29) - 1
IN_WORDS = OUT_WORDS = 146
PAIR_WORDS = 18

MUL, MUL_SHORT5, MUL_SHORT3, CANON, SUM64, SUM32, CARRY, ACC9, BLOCKSUM = range(9)
OP_NAMES = ["mul", "mul_short5", "mul_short3", "canon", "sum64", "sum32", "carry", "acc9", "blocksum"]
CANON_MUL29, CANON_MUL29V, CANON_FRMUL, CANON_IN_SHIFT, CANON_FROM_U64, CANON_FROM_MONT, CANON_FE_MUL, CANON_TO_MONT = range(8)
CANON_ALL = 0xff
SC_LANE_G0, SC_LANE_G1 = 15, 47
BLOCK_SIZES = (64, 128, 192, 256, 320, 512, 1024)

# ---- the constants of the sources, restated (tests/test_lazy_fr_host.py derives each from r and compares it with the source text)
NINV = 0x0fffffff  # Fr29::NINV = -r^-1 mod 2^29
R29 = [0x10000001, 0x1f0fac9f, 0x0e5c2450, 0x07d090f3, 0x1585d283, 0x02db40c0, 0x00a6e141, 0x0e5c2634, 0x0030644e]  # Fr29::P
R2PRE = [0x142db4df, 0x19d6990e, 0x1472f48c, 0x06dbe7e3, 0x0b84d579, 0x10f9faf7, 0x121f4380, 0x17a112de, 0x001275c7]
C261 = [0x0fffff57, 0x1ea70ab4, 0x052c068b, 0x17504f49, 0x0aa8075b, 0x1d4240ce, 0x11d54c07, 0x052ac7a8, 0x000dc836]  # 2^261 mod r
K343 = [0x02a7c5ae, 0x0efc10bf, 0x01057868, 0x0a968059, 0x10b7c2c3, 0x04d6a71f, 0x075f0711, 0x1678993c, 0x0024e88b]  # 2^343 mod r
BIAS64R = [0x40000040, 0x43eb27de, 0x5709143c, 0x54243cda, 0x4174a0cd, 0x56d03029, 0x49b85043, 0x57098cff, 0x0c19139a]  # poly.hip: 64 r, limbs raised
MAGIC = 0x54a474622  # acc9_reduce: floor(2^64 / ceil(r / 2^224))
FR29_ACC_MAX = 64    # fp29.hip.h: "at most FR29_ACC_MAX values (< 2 r each) between two reductions"

# ---- the classes, quoted
MUL_DEN = Fraction("168.9")  # fp29.hip.h: "value < (A*B/168.9 + 1)*p for a < A*p, b < B*p"
LIMB_IN = 1 << 30            # fp29.hip.h: "limbs of a, b < 2^30"
CHAIN_A = 4                  # fp29.hip.h: "a < A r (A <= 4), b = fr29_in_shift(y)"
SHIFT_B = 32                 # fp29.hip.h: "32 * y < 32 r, limbs < 2^29 (top < 2^27)"
OUT_MAX = 2                  # fp29.hip.h: fr29_out takes "a lazy chain value (< 2 r, exact limbs)"
SUM_MAX = 128                # fp29.hip.h: fr29_sum_reduce "x: near-normalised limbs (any f29_carry output), value < 128 r"
NEAR = (1 << 29) + 8         # fp29.hip.h: f29_carry "limbs < 2^32 in, limbs < 2^29 + 8 out (top limb keeps the rest)"
ACC9_MAX = 1 << 284          # acc9.hip.h: "S mod r for S < 2^284"
NARROW_B = 1 << 145          # fp29.hip.h: "H * 2^17 < 2^145: five limbs"
SPARTAN_E, SPARTAN_W = Fraction("1.2"), Fraction("71.1")  # poly.hip, eq_spartan_kernel: "W = AB - 32c + 64r" (< 71.1 r), E < 1.2 r
PAIR_SUM = Fraction("2.4")   # psc.hip, psc_expr_kernel: lazily added pair products (< 2.4 r, limbs < 2^30)
H_MAX = R >> 128             # the largest H with H * 2^128 canonical
U64_EDGES = [0, 1, (1 << 29) - 1, 1 << 29, (1 << 58) - 1, 1 << 58, 1 << 63, (1 << 64) - 1]


def kr(k):
    return int(Fraction(k) * R)


def mul_bound(a_cls, b_cls):
    """(A*B/168.9 + 1) r for class bounds A, B (Fractions, in units of r)"""
    return int((Fraction(a_cls) * Fraction(b_cls) / MUL_DEN + 1) * R)


# ---- limbs and words
def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def limbs(v):
    """the exact encoding: limbs 0..7 < 2^29, the top limb keeps the rest"""
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def raised(v):
    """the same integer with limbs 0..7 as large as the 2^30 class allows: + 2^29, borrowed from the next limb wherever that limb has it"""
    l = limbs(v)
    for i in range(8):
        if l[i + 1] >= 1:
            l[i] += 1 << 29
            l[i + 1] -= 1
    assert val(l) == v and max(l) < LIMB_IN
    return l


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def wval(ws):
    return sum(int(x) << (32 * i) for i, x in enumerate(ws))


def in_shift(y):
    """fr29_in_shift / fr29_prescale: 32 y as exact limbs"""
    return limbs(32 * y)


def carry_step(x):
    """f29_carry: ONE parallel step"""
    return [x[0] & MASK] + [(x[i] & MASK) + (x[i - 1] >> 29) for i in range(1, 8)] + [x[8] + (x[7] >> 29)]


# ---- the multiplier, column by column as the header has it (the accumulator widths are part of the contract: 64-bit words)
def mont_columns(a, b, nb=9):
    """f29t_mul<Fr29> (nb = 9) / f29t_mul_short<Fr29, nb>: returns (result limbs, widest column accumulator in bits)"""
    m, out, acc, widest = [], [0] * 9, 0, 0
    for k in range(9 + nb - 1):
        for i in range(max(0, k - (nb - 1)), min(k, 8) + 1):
            acc += a[i] * b[k - i]
        for i in range(max(0, k - 8), (k - 1 if k < nb else nb - 1) + 1):
            acc += m[i] * R29[k - i]
        if k < nb:
            m.append(((acc & 0xffffffff) * NINV) & MASK)
            acc += m[k] * R29[0]
        else:
            out[k - nb] = acc & MASK
        widest = max(widest, acc.bit_length())
        acc >>= 29
    out[8] = acc
    return out, widest


def mont_exact(av, bv, nb=9):
    """the same result in closed form: (a b + m r) / 2^(29 nb) with the one m < 2^(29 nb) that makes the division exact"""
    radix = 1 << (29 * nb)
    m = (-av * bv * pow(R, -1, radix)) % radix
    t = av * bv + m * R
    assert t % radix == 0
    return t >> (29 * nb)


def canon_of_lazy(t):
    """fr29_out: one conditional subtraction"""
    return t - R if t >= R else t


def acc9_reduce_model(s):
    """acc9_reduce as acc9.hip.h has it: two estimate-and-subtract passes, two conditional subtractions. Asserts what its comment states:
    the estimate fits 32 bits (< 2^31), never exceeds the true quotient, and two passes leave a value < 3 r"""
    for _ in range(2):
        q = ((s >> 224) * MAGIC) >> 64
        assert q < 1 << 31 and q * R <= s, (hex(s), q)
        s -= q * R
    assert s < 3 * R, hex(s)
    for _ in range(2):
        if s >= R:
            s -= R
    return s


# ---- records
def rec(kind, slots, flags=0, length=0, **meta):
    w = np.zeros(IN_WORDS, dtype=np.uint32)
    for k, s in slots.items():
        assert len(s) <= 9 and all(0 <= int(x) < 1 << 32 for x in s), (kind, k, s)
        w[9 * k:9 * k + len(s)] = s
    w[144], w[145] = flags, length
    return (kind, w, meta)


def pack(items):
    return np.stack([it[1] for it in items])


def slot(row, k, n=9):
    return [int(x) for x in row[9 * k:9 * k + n]]


class Gen:
    def __init__(self, seed):
        self.rng = random.Random(seed)

    def below(self, n):
        return self.rng.randrange(n)

    def fr(self):
        return self.rng.randrange(R)

    def lazy(self, bound=None):
        """a chain value: exact limbs, below the bound (default 2 r)"""
        return self.rng.randrange(bound or OUT_MAX * R)


def _mul_records(g, n):
    out = []
    top_b = 32 * (R - 1)

    def add(kind, a, b, a_cls, b_cls):
        out.append(rec(kind, {0: a, 1: b}, a_cls=Fraction(a_cls), b_cls=Fraction(b_cls)))

    for A in (1, 2, 4):
        a = A * R - 1
        add(f"top-A{A}", limbs(a), limbs(top_b), A, SHIFT_B)
        add(f"raised-a-A{A}", raised(a), limbs(top_b), A, SHIFT_B)
        add(f"raised-both-A{A}", raised(a), raised(top_b), A, SHIFT_B)
    # the output bound itself: operands at the top of their classes whose quotient m is within 2^-12 of 2^261 (b odd, a solved for)
    b_odd, j = SHIFT_B * R - 1, 0
    while True:
        j += 1
        a = -(MONT - j) * R * pow(b_odd, -1, MONT) % MONT
        if kr("3.99") <= a < CHAIN_A * R:
            break
    assert j < 1 << 249
    add("top-A4-largest-quotient", limbs(a), limbs(b_odd), CHAIN_A, SHIFT_B)
    add("top-A4-largest-quotient-raised", raised(a), raised(b_odd), CHAIN_A, SHIFT_B)
    for k in range(5):  # k r is < (k + 1) r: the k = 4 record is one step outside the chain's A <= 4, inside the multiplier's A B <= 168.9
        add(f"kr-{k}", limbs(k * R), limbs(top_b), k + 1, SHIFT_B)
        add(f"kr-{k}-raised", raised(k * R), in_shift(g.fr()), k + 1, SHIFT_B)
        add(f"kr-b-{k}", limbs(g.fr()), limbs(k * R), 1, SHIFT_B)
    for i in range(9):
        la, lb = [0] * 9, [0] * 9
        la[i] = MASK if i < 8 else (CHAIN_A * R - 1) >> 232
        lb[i] = MASK if i < 8 else (SHIFT_B * R - 1) >> 232
        add("top-limb" if i == 8 else f"single-limb-{i}", la, lb, CHAIN_A, SHIFT_B)
        add("top-limb-x-exact" if i == 8 else f"single-limb-{i}-x-exact", la, limbs(top_b), CHAIN_A, SHIFT_B)
    # eq_spartan_kernel: E * f29_carry(AB + BIAS64R - 32 c) with AB at the top of a product of two shifted factors and c = 0, then random
    ab_top = mul_bound(SHIFT_B, SHIFT_B) - 1
    for j in range(12):
        ab = limbs(ab_top) if j == 0 else mont_columns(in_shift(g.fr()), in_shift(g.fr()))[0]
        cs = [0] * 9 if j < 2 else in_shift(g.fr())
        w = [x + bias - c for x, bias, c in zip(ab, BIAS64R, cs)]
        e = limbs(kr(SPARTAN_E) - 1) if j == 0 else mont_columns(limbs(g.fr()), in_shift(g.fr()))[0]
        add("spartan-W-top" if j == 0 else "spartan-W", e, carry_step(w), SPARTAN_E, SPARTAN_W)
    # psc_expr_kernel: two chain products added limb-wise, multiplied on without a carry pass
    for j in range(12):
        p0, p1 = (limbs(kr("1.2") - 1),) * 2 if j == 0 else (mont_columns(limbs(g.fr()), in_shift(g.fr()))[0] for _ in range(2))
        add("pair-sum-top" if j == 0 else "pair-sum", [x + y for x, y in zip(p0, p1)], limbs(top_b) if j == 0 else in_shift(g.fr()), PAIR_SUM, SHIFT_B)
    while len(out) < n:
        A = g.rng.choice((1, 2, 4))
        a, y = g.below(A * R), g.fr()
        add("rand", limbs(a) if g.below(2) else raised(a), in_shift(y), A, SHIFT_B)
    return out[:n]


def _short_records(g, n, nb):
    out = []
    radix = 1 << (29 * nb)
    b_max = NARROW_B if nb == 5 else 1 << 64  # H * 2^17 < 2^145; a u64

    def add(kind, a, b, junk=False):
        bl = limbs(b)
        assert b < radix
        if junk:  # "b: NB limbs used": the others are not read
            bl = bl[:nb] + [g.below(1 << 32) for _ in range(9 - nb)]
        out.append(rec(kind, {0: a, 1: bl}, nb=nb))

    if nb == 5:
        for H in (0, 1, (1 << 64) - 1, H_MAX - 2, H_MAX - 1, H_MAX):
            add(f"H-{H if H < 2 else hex(H)}", limbs(R - 1), H << 17)
            add("H-rand-x", limbs(g.fr()), H << 17)
        add("b-top", limbs(R - 1), NARROW_B - 1)
        add("b-top-raised-a", raised(R - 1), NARROW_B - 1)
    else:
        for u in U64_EDGES:
            add(f"k343-u-{hex(u)}", K343, u)
            add("x-top-u", limbs(R - 1), u)
        add("b-top", limbs(R - 1), b_max - 1)
        add("b-top-raised-a", raised(R - 1), b_max - 1)
    for k in range(2):
        add(f"kr-{k}", limbs(k * R - (1 if k else 0)), b_max - 1)
    for _ in range(16):
        add("junk-high", limbs(g.fr()), g.below(b_max), junk=True)
    while len(out) < n:
        x = g.fr()
        add("rand", limbs(x) if g.below(2) else raised(x), g.below(b_max))
    return out[:n]


def _canon_records(g, n):
    out = []

    def add(kind, x, y, u=None):
        u = g.below(1 << 64) if u is None else u
        out.append(rec(kind, {0: words(x), 1: words(y), 2: words(u, 2)}, flags=CANON_ALL, x=x, y=y, u=u))

    for H in (0, 1, (1 << 64) - 1, H_MAX - 2, H_MAX - 1, H_MAX):
        for x in (R - 1, g.fr()):
            add(f"narrow-H-{H if H < 2 else hex(H)}", x, H << 128)
    for i in range(4):  # exactly one non-zero low word: the wide path, the same result
        for wv in (1, 0xffffffff, 1 + g.below(0xffffffff)):
            add(f"one-low-word-{i}", g.fr(), (g.below(H_MAX) << 128) | (wv << (32 * i)))
            add(f"one-low-word-{i}", R - 1, wv << (32 * i))
    add("y-zero", g.fr(), 0)
    add("y-one-mont", g.fr(), ABI % R)
    add("x-zero", 0, g.fr())
    add("xy-top", R - 1, R - 1)
    add("y-top", g.fr(), R - 1)
    for u in U64_EDGES:
        add(f"u-{hex(u)}", g.fr(), g.fr(), u)
    while len(out) < n:
        narrow = g.below(4) == 0
        add("rand-narrow" if narrow else "rand", g.fr(), g.below(H_MAX) << 128 if narrow else g.fr())
    return out[:n]


def _ones(top):
    return [MASK] * 8 + [top]


ONES_TOP = (OUT_MAX * R >> 232) - 1  # the largest top limb under which eight limbs of 2^29 - 1 stay below 2 r


def _sum_values(g, kind, count):
    if kind == "max":
        return limbs(OUT_MAX * R - 1)
    if kind == "zero":
        return [0] * 9
    if kind == "ones":
        return _ones(ONES_TOP)
    return limbs(g.lazy())


def _sum64_records(g, n):
    out = []
    counts = (1, 2, 3, 4, 5, 63, 64)
    while len(out) < n:
        for count in counts:
            for kind in ("max", "zero", "ones", "rand"):
                length = 1 if kind != "rand" else 1 + g.below(16)
                vals = [_sum_values(g, kind, count) for _ in range(length)]
                out.append(rec(f"{kind}-{count}", dict(enumerate(vals)), flags=count, length=length))
        counts = tuple(1 + g.below(64) for _ in range(7))
    return out[:n]


def _sum32_records(g, n):
    out = []
    counts = (1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68)
    while len(out) < n:
        for count in counts:
            for kind in ("max", "zero", "ones", "rand", "mixed"):
                length = 1 if kind in ("max", "zero", "ones") else 1 + g.below(4)
                vals = {}
                for j in range(length):
                    for t in range(4):
                        k = kind if kind != "mixed" else ("max", "zero", "ones", "rand")[(t + j) % 4]
                        vals[4 * j + t] = _sum_values(g, k, count)
                out.append(rec(f"{kind}-{count}", vals, flags=count, length=length))
        counts = tuple(1 + g.below(68) for _ in range(11))
    return out[:n]


def _carry_records(g, n):
    out = [rec("all-max", {0: [0xffffffff] * 8 + [0xffffffff - 7]}), rec("zero", {0: [0] * 9}),
           rec("four-additions", {0: [NEAR - 1 + 4 * MASK] * 9}), rec("limb0-only", {0: [0xffffffff] + [0] * 8}),
           rec("limb7-only", {0: [0] * 7 + [0xffffffff, 0]})]
    while len(out) < n:
        out.append(rec("rand", {0: [g.below(1 << 32) for _ in range(8)] + [g.below((1 << 32) - 7)]}))
    return out[:n]


K_MAX = ACC9_MAX // R


def _acc9_records(g, n):
    out = []

    def add(kind, s, v=None, w=None, t=None):
        v, w = g.fr() if v is None else v, g.fr() if w is None else w
        t = g.below(ACC9_MAX) if t is None else t
        out.append(rec(kind, {0: words(s, 9), 1: words(v), 2: words(w), 3: words(t, 9)}, s=s, v=v, w=w, t=t))

    while len(out) < n:
        for name, k in (("2^10", g.below(1 << 10)), ("2^20", g.below(1 << 20)), ("2^30", g.below(1 << 30)), ("max", K_MAX)):
            for dname, d in (("-1", -1), ("+0", 0), ("+1", 1), ("+r-1", R - 1), ("+r/2", R // 2)):
                s = k * R + d
                if 0 <= s < ACC9_MAX:
                    add(f"kr-{name}{dname}", s)
        add("top", ACC9_MAX - 1, R - 1, R - 1, ACC9_MAX - 1)
        for v in (1, R - 1, None):  # limbs 0..7 all ones: the addition carries through every limb into the ninth
            s = ((g.below(1 << 27)) << 256) | (ABI - 1)
            add("carry-through", s, v, 1 if v is None else v, (g.below(1 << 27) << 256) | (1 if v is None else ABI - 1))
        add("zero", 0, 0, 0, 0)
        for _ in range(16):
            add("rand", g.below(1 << g.rng.choice((64, 200, 256, 257, 284))))
    return out[:n]


def records_for(op, seed, n):
    g = Gen(seed)
    if op == MUL:
        return _mul_records(g, n)
    if op in (MUL_SHORT5, MUL_SHORT3):
        return _short_records(g, n, 5 if op == MUL_SHORT5 else 3)
    return {CANON: _canon_records, SUM64: _sum64_records, SUM32: _sum32_records, CARRY: _carry_records, ACC9: _acc9_records}[op](g, n)


# ---- the operand classes (what the comments of the headers promise the functions, nothing more)
def _sum_cycle(row, t=None):
    count, length = int(row[144]), int(row[145])
    if t is None:
        return count, [slot(row, j) for j in range(length)]
    return count, [slot(row, 4 * j + t) for j in range(length)]


def assert_in_class(op, items):
    for kind, row, meta in items:
        if op == MUL:
            a, b = slot(row, 0), slot(row, 1)
            assert max(a) < LIMB_IN and max(b) < LIMB_IN, kind
            assert val(a) < meta["a_cls"] * R and val(b) < meta["b_cls"] * R, kind
            assert meta["a_cls"] * meta["b_cls"] <= MUL_DEN, kind  # the product is < 2 r: what fr29_out and every later step take
        elif op in (MUL_SHORT5, MUL_SHORT3):
            a, b = slot(row, 0), slot(row, 1)[:meta["nb"]]
            assert max(a) < LIMB_IN and val(a) < R and max(b) <= MASK, kind
            assert val(b) < (NARROW_B if op == MUL_SHORT5 else 1 << 64), kind
        elif op == CANON:
            assert wval(slot(row, 0, 8)) < R and wval(slot(row, 1, 8)) < R, kind
        elif op in (SUM64, SUM32):
            for t in (range(4) if op == SUM32 else [None]):
                count, cyc = _sum_cycle(row, t)
                assert 1 <= count <= (FR29_ACC_MAX if op == SUM64 else 1 << 10) and cyc, kind
                assert all(max(v[:8]) <= MASK and val(v) < OUT_MAX * R for v in cyc), kind
        elif op == CARRY:
            x = slot(row, 0)
            assert x[8] + (x[7] >> 29) < 1 << 32, kind
        elif op == ACC9:
            assert meta["s"] < ACC9_MAX and meta["t"] < ACC9_MAX and meta["v"] < R and meta["w"] < R, kind


# ---- the checker
def _eq(got, want, what, kind, i):
    assert list(got) == list(want), f"record {i} ({kind}): {what}: got {[hex(x) for x in got]}, want {[hex(x) for x in want]}"


def check(op, items, out):
    """asserts every record's outputs; returns {name: the largest value / r seen} (and the widest column accumulator, in bits)"""
    assert out.shape == (len(items), OUT_WORDS)
    assert_in_class(op, items)
    mx = defaultdict(float)

    def seen(name, v):
        mx[name] = max(mx[name], float(Fraction(v, R)))

    for i, ((kind, row, meta), o) in enumerate(zip(items, out)):
        status, aux = int(o[144]), int(o[145])
        if op in (MUL, MUL_SHORT5, MUL_SHORT3):
            nb = 9 if op == MUL else meta["nb"]
            a, b = slot(row, 0), slot(row, 1)
            av, bv = val(a), val(b[:nb])
            t, widest = mont_columns(a, b, nb)
            assert widest <= 64, (kind, widest)  # the column accumulators are u64
            want = mont_exact(av, bv, nb)
            assert val(t) == want and max(t[:8]) <= MASK  # the model against the closed form
            got = slot(o, 0)
            _eq(got, t, "raw product", kind, i)
            assert max(got[:8]) <= MASK, (kind, "output limbs are exact")
            bound = mul_bound(meta["a_cls"], meta["b_cls"]) if op == MUL else OUT_MAX * R
            assert val(got) < bound and val(got) * (1 << (29 * nb)) % R == av * bv % R, (kind, "bound / residue")
            _eq(slot(o, 1, 8), words(av * bv * pow(1 << (29 * nb), -1, R) % R), "fr29_out", kind, i)
            seen(f"mul {float(meta['a_cls']):g} x {float(meta['b_cls']):g}" if op == MUL else OP_NAMES[op], val(got))
            mx["column bits"] = max(mx["column bits"], widest)
            assert status == 0 and aux == 0 and not o[18:144].any(), kind
        elif op == CANON:
            x, y, u = meta["x"], meta["y"], meta["u"]
            prod = words(x * y * pow(ABI, -1, R) % R)
            for k, name in ((CANON_MUL29, "fr_mul29(prescale)"), (CANON_MUL29V, "fr_mul29v"), (CANON_FRMUL, "frmul_apply"), (CANON_FE_MUL, "fe_mul")):
                _eq(slot(o, k, 8), prod, name, kind, i)
            narrow = y % (1 << 128) == 0
            assert aux == (1 if narrow else 0), f"record {i} ({kind}): narrow bit {aux}"
            _eq(slot(o, 8), limbs((y >> 128) << 17) if narrow else in_shift(y), "the prepared factor", kind, i)
            sh = slot(o, CANON_IN_SHIFT)
            _eq(sh, in_shift(y), "fr29_in_shift", kind, i)
            assert max(sh[:8]) <= MASK and sh[8] < 1 << 27 and val(sh) < SHIFT_B * R, kind
            _eq(slot(o, CANON_FROM_U64, 8), words(u * ABI % R), "fr_from_u64_29", kind, i)
            _eq(slot(o, CANON_FROM_MONT, 8), words(x * pow(ABI, -1, R) % R), "fr_from_mont29", kind, i)
            _eq(slot(o, CANON_TO_MONT, 8), words(x * ABI % R), "fr_mul29(x, R2PRE)", kind, i)
            # the lazy values behind those canonical outputs, from the model: all below 2 r with 64-bit columns
            for name, (t, widest) in (("fr_mul29", mont_columns(limbs(x), in_shift(y))),
                                      ("narrow", mont_columns(limbs(x), limbs((y >> 128) << 17), 5) if narrow else ([0] * 9, 0)),
                                      ("from_u64", mont_columns(K343, limbs(u), 3)), ("to_mont", mont_columns(limbs(x), R2PRE))):
                assert val(t) < OUT_MAX * R and widest <= 64, (kind, name)
                seen(name, val(t))
            assert status == 0 and all(o[9 * k + 8] == 0 for k in (0, 1, 2, 4, 5, 6, 7)) and not o[81:144].any(), kind
        elif op == SUM64:
            count, cyc = _sum_cycle(row)
            total = sum(val(cyc[j % len(cyc)]) for j in range(count))
            assert total < SUM_MAX * R
            _eq(slot(o, 0, 8), words(total % R), "acc29_reduce", kind, i)
            assert aux == FR29_ACC_MAX and status == 0, (kind, "FR29_ACC_MAX", aux)
            t, widest = mont_columns(limbs(total), C261)  # what acc29_reduce hands fr29_out
            assert val(t) < OUT_MAX * R and widest <= 64
            seen("sum64 in", total)
            seen("sum64 out", val(t))
        elif op == SUM32:
            for t in range(4):
                count, cyc = _sum_cycle(row, t)
                total = sum(val(cyc[j % len(cyc)]) for j in range(count))
                _eq(slot(o, t, 8), words(total % R), f"ChainAcc4 e[{t}]", kind, i)
                # the largest sum the reduction saw: the first FR29_ACC_MAX values, or what followed them
                for part in (range(min(count, FR29_ACC_MAX)), range(FR29_ACC_MAX, count)):
                    s = sum(val(cyc[j % len(cyc)]) for j in part)
                    assert s < SUM_MAX * R
                    seen("sum32 in", s)
            assert aux == FR29_ACC_MAX, (kind, "FR29_ACC_MAX", aux)
            assert status == (count if count < FR29_ACC_MAX else count - FR29_ACC_MAX), f"record {i} ({kind}): {status} values were pending at the last flush"
        elif op == CARRY:
            x = slot(row, 0)
            got = slot(o, 0)
            _eq(got, carry_step(x), "f29_carry", kind, i)
            assert val(got) == val(x) and got[0] <= MASK and max(got[1:8]) < NEAR, kind
        elif op == ACC9:
            s, v, w, t = meta["s"], meta["v"], meta["w"], meta["t"]
            assert acc9_reduce_model(s) == s % R
            _eq(slot(o, 0, 8), words(s % R), "acc9_reduce", kind, i)
            assert o[8] == 0
            for k, want, name in ((1, s + v, "acc9_add"), (2, s + w, "acc9_add_if(true)"), (3, s, "acc9_add_if(false)"), (4, s + t, "acc9_add_acc")):
                assert want < 1 << 288
                _eq(slot(o, k), words(want, 9), name, kind, i)
            mx["acc9 bits"] = max(mx["acc9 bits"], s.bit_length())
    return dict(mx)


# ---- what both test files run: the record counts, the kinds that must be present
SEED = 20261
N = {MUL: 2048, MUL_SHORT5: 1024, MUL_SHORT3: 1024, CANON: 2048, SUM64: 1024, SUM32: 1024, CARRY: 1024, ACC9: 2048}
NEED = {
    MUL: ["rand", "top-A1", "top-A2", "top-A4", "raised-a-A1", "raised-a-A2", "raised-a-A4", "raised-both-A4", "top-A4-largest-quotient", "top-A4-largest-quotient-raised", "kr-0", "kr-1", "kr-2", "kr-3", "kr-4",
             "single-limb-0", "single-limb-7", "top-limb", "spartan-W-top", "spartan-W", "pair-sum-top", "pair-sum"],
    MUL_SHORT5: ["rand", "H-0", "H-1", "H-0xffffffffffffffff", f"H-{hex(H_MAX)}", f"H-{hex(H_MAX - 1)}", "b-top", "b-top-raised-a", "junk-high"],
    MUL_SHORT3: ["rand", "b-top", "junk-high"] + [f"k343-u-{hex(u)}" for u in U64_EDGES],
    CANON: ["rand", "rand-narrow", "narrow-H-0", "narrow-H-1", "narrow-H-0xffffffffffffffff", f"narrow-H-{hex(H_MAX)}", f"narrow-H-{hex(H_MAX - 1)}",
               "one-low-word-0", "one-low-word-1", "one-low-word-2", "one-low-word-3", "y-zero", "y-one-mont", "xy-top"] + [f"u-{hex(u)}" for u in U64_EDGES],
    SUM64: [f"{k}-{c}" for k in ("max", "zero", "ones", "rand") for c in (1, 2, 3, 4, 5, 63, 64)],
    SUM32: [f"{k}-{c}" for k in ("max", "zero", "ones", "rand", "mixed") for c in (1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68)],
    CARRY: ["all-max", "zero", "four-additions", "rand"],
    ACC9: ["kr-2^10-1", "kr-2^10+0", "kr-2^10+1", "kr-2^10+r-1", "kr-2^20-1", "kr-2^20+r-1", "kr-2^30-1", "kr-2^30+0", "kr-2^30+1", "kr-2^30+r-1", "kr-max-1",
              "kr-max+0", "top", "carry-through", "zero", "rand"],
}


def family(run, op, n=None):
    """one op's records through `run` (the host harness or the device hook), every named kind present, checked; prints the largest values"""
    n = n or N[op]
    items = records_for(op, SEED + op, n)
    assert len(items) == n
    kinds = {it[0] for it in items}
    missing = [w for w in NEED[op] if w not in kinds]
    assert not missing, (missing, sorted(kinds))
    out = run(op, items)
    mx = check(op, items, out)
    print(f"{OP_NAMES[op]}: {n} records, largest values / r (and widths in bits): " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(mx.items())))
    return items, out, mx



# ---- the block reduction (device only): one workgroup per case, every thread its own raw pair
def blocksum_cases(threads, seed):
    """[(kind, (threads, 18) uint32)]: totals below 2^284 (acc9_reduce's bound); g0 and g1 always differ"""
    g = Gen(seed * 4099 + threads)
    per = ACC9_MAX // threads  # any `threads` values below this add up to less than 2^284
    cases = []

    def case(kind, fn):
        a = np.zeros((threads, PAIR_WORDS), dtype=np.uint32)
        for t in range(threads):
            p = fn(t)
            if p is not None:
                a[t, :9], a[t, 9:] = words(p[0], 9), words(p[1], 9)
        cases.append((kind, a))

    top = (per >> 256) - 1
    case("all-ones-low", lambda t: ((top << 256) | (ABI - 1), ((top - 1) << 256) | (ABI - 1)))  # every addition carries across all nine limbs
    case("all-ones-low-rand-top", lambda t: ((g.below(top) << 256) | (ABI - 1), (g.below(top) << 256) | (ABI - 1)))
    for lane in (0, 15, 16, 31, 32, 63):
        v = (g.below(ACC9_MAX), g.below(ACC9_MAX))
        case(f"single-lane-{lane}", lambda t, lane=lane, v=v: v if t == lane else None)
    for name, at in (("last-wave-first", threads - 64), ("last-wave-last", threads - 1), ("last-wave-31", threads - 33)):
        v = (ACC9_MAX - 1, g.below(ACC9_MAX))
        case(name, lambda t, at=at, v=v: v if t == at else None)
    case("zero", lambda t: None)
    case("canonical-max", lambda t: (R - 1, R - 2))
    case("rand", lambda t: (g.below(per), g.below(per)))
    case("rand-g1-only", lambda t: (0, g.below(per)))
    case("thread-index", lambda t: (t + 1, (threads - t) << 255))
    return cases


def check_blocksum(cases, out):
    assert out.shape == (len(cases), 16)
    for (kind, a), o in zip(cases, out):
        for half, name in ((0, "g0"), (1, "g1")):
            total = sum(wval(row[9 * half:9 * half + 9]) for row in a)
            assert total < ACC9_MAX, kind
            got = [int(x) for x in o[8 * half:8 * half + 8]]
            assert got == words(total % R), f"{kind} ({a.shape[0]} threads): {name}: got {hex(wval(got))}, want {hex(total % R)}"
