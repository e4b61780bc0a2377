"""Column headroom of the mixed addition's ten products with P, R and 4p - Y1 UN-CARRIED (zolt_amd/csrc/g1_29.hip.h: xyzz29_madd_nz;
fp29.hip.h: f29_sub7_raw, f29_pmsub45_raw, f29_neg4_raw). No GPU and no compiler: exact Python integers.

The multiplier (fp29.hip.h: f29t_mulsum / f29_sqr and the asm column statements) adds, per column k, the carry out of column k - 1,
the product terms a_i * b_(k-i) (two sets in the two-product form) and the reduction terms m_i * P_(k-i) with quotient digits
m_i < 2^29, into ONE unsigned 64-bit word, then shifts it right by 29 (logically). The results are right exactly as long as no
column reaches 2^64. This file

  * parses the raised bias tables RAW4P / RAW5P / RAW7P from the source text, derives them from p and checks the decomposition
    (b0 = L0 + 2^r, bi = Li + 2^r - 2^(r-29), b8 = L8 - 2^(r-29); sum k*p) and the limb condition (every Li, i = 0..7, >= 8: a
    near-normalised subtrahend, limbs <= 2^29 + 7, never underflows a limb; 5p's 2^30 covers an exact and a near-normalised one);
  * propagates PER-LIMB MAXIMA through the ten products for both signs of the digit. Each limb of each operand is taken at its
    largest independently of the others, which no single input reaches: the figures are upper bounds, not attained values. Operand
    classes (g1_29.hip.h, top of file): table rows and mul outputs have exact limbs (<= 2^29 - 1); acc.x is a carry output
    (<= 2^29 + 7, limb 0 exact); acc.y is a mul output or, at a run start, a negated affine y <= 2p (a carry output) — taken
    near-normalised in ALL limbs 0..7 here, and so are acc.zz and acc.zzz, because the self-test records force such limbs
    (tests/lazy_model.py: Gen.forced); top limbs are those of the class bounds;
  * asserts every column, reduction terms and carry-in included, is below 2^64. The reduction terms are counted as 2^29 * 2^29
    each (COARSE_P), the accounting the design's bounds are written in; the figures with the limbs of p as they are (TIGHT_P, about
    5 * 2^58 lower per full column) are printed beside them;
  * asserts that with Q + 7p - X3 un-carried as well the bound is NOT below 2^64 in that accounting (64.6 * 2^58; 59.6 with the
    limbs of p as they are): that form keeps its carry pass, and whoever wants to "finish the job" has to come through here and
    redo the accounting for every product on the tighter basis first.

    python -m pytest tests/test_lazy_g1_headroom.py -q -s       # prints the largest column of each product in units of 2^58"""
import os
import re
from fractions import Fraction

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MASK = (1 << 29) - 1
NEAR_MAX = (1 << 29) + 7
LIMIT = 1 << 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zolt_amd", "csrc", "fp29.hip.h")


def limbs(v):
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def kp(k):
    return int(Fraction(k) * P)


def table(name):
    with open(SRC) as f:
        text = f.read()
    m = re.search(r"static constexpr u32 %s\[9\] = \{([^}]*)\}" % name, text)
    assert m, name
    out = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert len(out) == 9
    return out


def raised(k, r):
    """k*p with limbs 0..7 raised by 2^r and the excess borrowed from the next limb"""
    L, e = limbs(k * P), 1 << (r - 29)
    return [L[0] + (1 << r)] + [L[i] + (1 << r) - e for i in range(1, 8)] + [L[8] - e]


P_LIMBS = limbs(P)
RAW4P, RAW5P, RAW7P = table("RAW4P"), table("RAW5P"), table("RAW7P")


def test_bias_tables():
    assert table("P") == P_LIMBS
    for name, got, k, r in (("RAW4P", RAW4P, 4, 29), ("RAW5P", RAW5P, 5, 30), ("RAW7P", RAW7P, 7, 29)):
        assert got == raised(k, r), name
        assert val(got) == k * P, name
        L = limbs(k * P)
        assert min(L[:8]) >= 8, (name, min(L[:8]))
        print(f"{name}: smallest limb 0..7 of {k}p = {min(L[:8])}, smallest middle limb = {min(L[1:8])}")
        # no limb underflows: one near-normalised subtrahend under 2^29 (limb 0: b0 has the whole raise), an exact one more under 2^30
        sub = NEAR_MAX + (MASK if r == 30 else 0)
        assert all(b >= sub for b in got[:8]), name
    # the carried forms' tables, for comparison: the same multiples of p
    for name, k in (("BIAS4P", 4), ("BIAS5P", 5), ("BIAS7P", 7)):
        assert val(table(name)) == k * P


# ---- per-limb maxima of the operand classes
def exact(bound):
    return [MASK] * 8 + [(kp(bound) - 1) >> 232]


def near(bound, keep0):
    return [MASK if keep0 else NEAR_MAX] + [NEAR_MAX] * 7 + [(kp(bound) - 1) >> 232]


def carried(raw):
    """f29_carry of limbs < 2^32: limbs 1..7 < 2^29 + 8, limb 0 exact, the top limb takes limb 7's carry"""
    assert all(x < 1 << 32 for x in raw)
    return [MASK] + [MASK + (raw[i - 1] >> 29) for i in range(1, 8)] + [raw[8] + (raw[7] >> 29)]


def plus(a, bias):
    """a + bias - (a subtrahend >= 0), limb-wise maxima"""
    out = [x + b for x, b in zip(a, bias)]
    assert all(x < 1 << 32 for x in out)
    return out


ROW, MUL, ACC_X = "1.1", "1.6", "6.6"
# the reduction terms m_i * P_j, two accountings. TIGHT: the limbs of p as they are (several are small: the terms of a full column add
# up to 3.0 * 2^58). COARSE: every term < 2^29 * 2^29, the accounting of the design tables (docs/design/04_kernels.md), 8 to 9 * 2^58
# per column. Every assertion below is made under COARSE, which implies TIGHT; both figures are printed.
TIGHT_P, COARSE_P = P_LIMBS, [MASK] * 9


def columns(pairs, p_limbs):
    """the largest value each of the 17 column accumulators can hold, for sum of a*b over `pairs` of per-limb maxima: carry-in,
    product terms, reduction terms m_i * P_(k-i) with quotient digits m_i <= 2^29 - 1"""
    worst, carry = [], 0
    for k in range(17):
        acc = carry
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(max(0, k - 8), min(k, 8) + 1))
        acc += sum(MASK * p_limbs[k - i] for i in range(max(0, k - 8), min(k, 8) + 1))
        worst.append(acc)
        carry = acc >> 29
    return worst


def addition(neg, p_limbs, carry_q_minus_x3=True):
    """{product: its 17 column maxima} for one mixed addition. acc.y (a mul output, or a negated affine y <= 2p at a run start) is a
    subtrahend only: it enters through the no-underflow condition of test_bias_tables, and the maxima below take it as 0."""
    px, py = exact(ROW), exact(ROW)
    x1, zz, zzz = near(ACC_X, True), near(MUL, False), near(MUL, False)
    m = exact(MUL)  # every mul output: U2, S2, PP, R^2, PPP, Q
    Pp = plus(m, RAW7P)                         # U2 + 7p - X1
    R = list(RAW5P) if neg else plus(m, RAW4P)  # 5p - S2 - Y1 (RAW5P + 1 + ~S2 - Y1 = RAW5P - S2 - Y1), or S2 + 4p - Y1
    ny = list(RAW4P)                            # 4p - Y1
    assert all(2 * x < 1 << 32 for x in Pp + R)  # f29_twice of the squares' operands fits 32 bits
    if carry_q_minus_x3:
        qx = carried(plus(m, table("BIAS7P")))  # Q + 7p - X3 as the code has it: f29_sub7
    else:
        qx = plus(m, RAW7P)                     # ... and as f29_sub7_raw would leave it
    prods = {"U2": [(px, zz)], "S2": [(py, zzz)], "PP": [(Pp, Pp)], "RR": [(R, R)], "PPP": [(Pp, m)], "Q": [(x1, m)], "ZZ3": [(zz, m)],
             "Y3": [(R, qx), (ny, m)], "ZZZ3": [(zzz, m)]}
    return {name: columns(pairs, p_limbs) for name, pairs in prods.items()}


def _largest(p_limbs, **kw):
    out = {}
    for neg in (False, True):
        for name, cols in addition(neg, p_limbs, **kw).items():
            k = max(range(17), key=lambda i: cols[i])
            if cols[k] > out.get(name, (0, 0, ""))[0]:
                out[name] = (cols[k], k, "-" if neg else "+")
    return out


def test_every_column_is_below_2_64():
    coarse, tight = _largest(COARSE_P), _largest(TIGHT_P)
    for name, (v, k, sign) in coarse.items():
        print(f"{name}: largest column {v / 2 ** 58:.1f} * 2^58 (column {k}, sign {sign}); with the limbs of p as they are "
              f"{tight[name][0] / 2 ** 58:.1f}; limit 64")
        assert tight[name][0] <= v < LIMIT, (name, k, sign, v / 2 ** 58)
    # the products of near-normalised operands keep the old bound (< 2^63)
    assert all(coarse[n][0] < 1 << 63 for n in ("U2", "S2", "Q", "ZZ3", "ZZZ3"))


def test_q_minus_x3_has_to_stay_carried():
    """Un-carried, Q + 7p - X3 takes a column of Y3 past 2^64 in the accounting every bound of this design is written in (COARSE). With
    the limbs of p as they are the same column is bounded lower (printed): whoever drops that carry pass has to redo the accounting
    for ALL products on that basis first, and change this test with it."""
    coarse = _largest(COARSE_P, carry_q_minus_x3=False)["Y3"]
    tight = _largest(TIGHT_P, carry_q_minus_x3=False)["Y3"]
    print(f"Y3 with Q + 7p - X3 un-carried: {coarse[0] / 2 ** 58:.1f} * 2^58 (column {coarse[1]}, sign {coarse[2]}); with the limbs of p "
          f"as they are {tight[0] / 2 ** 58:.1f}; limit 64")
    assert coarse[0] >= LIMIT, coarse[0] / 2 ** 58


def test_the_model_reproduces_the_carried_bound():
    """the checker on the forms as they were (every operand near-normalised): fp29.hip.h counts at most 9 + 9 terms of < 2^58 in a
    column, 27 in the two-product form, < 2^63. The widest columns with eight full-size limbs hold 8 + 8 and 8 + 8 + 8 of them."""
    a = near("8.6", False)
    one, two = max(columns([(a, a)], COARSE_P)), max(columns([(a, a), (a, a)], COARSE_P))
    assert 16 << 58 < one < 18 << 58 and 24 << 58 < two < 27 << 58 and two < 1 << 63, (one / 2 ** 58, two / 2 ** 58)
