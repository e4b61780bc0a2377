"""The DoryVerifierSetup the reference itself wrote (tests/golden/dory_verifier_setup_captured.bin, cut by
tests/golden/make_dory_vsetup_fixture.py from the reference's captured prove run) parsed for the tests: DoryVerifierSetup.serialize's
layout (src/zkvm/preprocessing.zig:977-1025) walked field by field, the GT values as tests/pairing_model.py tuples and as the ABI's
48-word arrays, the four points decompressed.

Decompression is written from the reference's own flag rules (serializeG1 :1061-1090, serializeG2 :1092-1127, lexicographicallyLess
:1129-1139, lexicographicallyLessFp2 :1141-1166) and the curve equations, not by inverting this repository's serialisers: bit 63 of the
last limb is set exactly when y is NOT lexicographically less than -y, bit 62 alone is the identity. Plain module: no fixtures, no
pytest hooks."""
import os

import numpy as np

from tests import g2_model as g2m
from tests import pairing_model as pm

P = g2m.P
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dory_verifier_setup_captured.bin")
SHA256 = "9137300bccf4ca64796a08be5742f88bc4d7b941a556aac406c1a06629f8d16a"
LENGTH, K, GT_BYTES = 17904, 8, 384
VECTORS = ("delta_1l", "delta_1r", "delta_2l", "delta_2r", "chi")
POINTS_AT = 5 * (8 + (K + 1) * GT_BYTES)  # 17 320: g1_0, g2_0, h1, h2, ht, max_log_n follow
SIGN, INFINITY = 1 << 255, 1 << 254       # bits 63 and 62 of the last limb of a little-endian 32-byte value


def read():
    return open(PATH, "rb").read()


# ---- square roots (p = 3 mod 4)
def fp_sqrt(a):
    """a root of a in Fp, or None"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def f2_sqrt(a):
    """a root of a = a0 + a1 u in Fp2 = Fp[u] / (u^2 + 1), or None: x0^2 - x1^2 = a0, 2 x0 x1 = a1, so x0^2 = (a0 +- |a|) / 2 with
    |a|^2 = a0^2 + a1^2 the norm; whichever half is a square in Fp gives x0"""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        y = fp_sqrt(a0)
        if y is not None:
            return (y, 0)
        y = fp_sqrt(-a0 % P)  # -1 is no square: exactly one of a0, -a0 is
        return (0, y)
    alpha = fp_sqrt((a0 * a0 + a1 * a1) % P)
    if alpha is None:
        return None
    half = pow(2, -1, P)
    x0 = fp_sqrt((a0 + alpha) * half % P)
    if x0 is None:
        x0 = fp_sqrt((a0 - alpha) * half % P)
    if x0 is None or x0 == 0:
        return None
    y = (x0, a1 * pow(2 * x0, -1, P) % P)
    return y if g2m.f2_sqr(y) == (a0, a1) else None


# ---- the reference's orderings (:1129-1166), on canonical integers
def lexicographically_less(a, b):
    return a < b


def lexicographically_less_fp2(a, b):
    if a[1] != b[1]:  # c1 is the more significant
        return a[1] < b[1]
    return a[0] < b[0]


# ---- points
def decompress_g1(b, flip=False):
    """32 bytes of serializeG1 -> (x, y) or None for the identity; flip=True gives the OTHER root (for the sign-sensitivity tests)"""
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    if v & INFINITY:
        assert v == INFINITY, "the identity is bit 62 alone"
        return None
    x = v & ~SIGN
    assert x < P, "non-canonical x"
    y = fp_sqrt((x * x * x + 3) % P)
    assert y is not None, "x is not on y^2 = x^3 + 3"
    flag = bool(v & SIGN)
    if (not lexicographically_less(y, -y % P)) != flag:
        y = -y % P
    assert (not lexicographically_less(y, -y % P)) == flag
    return (x, -y % P if flip else y)


def decompress_g2(b, flip=False):
    """64 bytes of serializeG2 -> ((x0, x1), (y0, y1)) or None; the flags sit in the last limb of x.c1"""
    assert len(b) == 64
    x0, v = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
    if v & INFINITY:
        assert v == INFINITY and x0 == 0, "the identity is bit 62 alone"
        return None
    x = (x0, v & ~SIGN)
    assert x[0] < P and x[1] < P, "non-canonical x"
    y = f2_sqrt(g2m.f2_add(g2m.f2_mul(g2m.f2_sqr(x), x), g2m.B_TWIST))
    assert y is not None, "x is not on y^2 = x^3 + 3 / xi"
    flag = bool(v & SIGN)
    if (not lexicographically_less_fp2(y, g2m.f2_neg(y))) != flag:
        y = g2m.f2_neg(y)
    assert (not lexicographically_less_fp2(y, g2m.f2_neg(y))) == flag
    return (x, g2m.f2_neg(y) if flip else y)


# ---- the whole setup
class Captured:
    """raw: the bytes; delta_1l .. chi: lists of nine model Fp12 tuples, and <name>_words their (9, 48) Montgomery arrays; g1_0, g2_0,
    h1, h2: model points, <name>_bytes their compressed bytes; ht / ht_words; max_log_n"""


def parse(data=None):
    from zolt_amd import api
    data = read() if data is None else data
    assert len(data) == LENGTH
    out = Captured()
    out.raw = data
    pos = 0
    for name in VECTORS:
        count = int.from_bytes(data[pos:pos + 8], "little")
        assert count == K + 1, (name, count)
        pos += 8
        chunks = [data[pos + GT_BYTES * i:pos + GT_BYTES * (i + 1)] for i in range(count)]
        pos += GT_BYTES * count
        setattr(out, name + "_bytes", chunks)
        setattr(out, name, [pm.from_bytes(c) for c in chunks])
        setattr(out, name + "_words", np.stack([api.gt_from_bytes(c) for c in chunks]))
    assert pos == POINTS_AT
    for name, size, fn in (("g1_0", 32, decompress_g1), ("g2_0", 64, decompress_g2), ("h1", 32, decompress_g1), ("h2", 64, decompress_g2)):
        setattr(out, name + "_bytes", data[pos:pos + size])
        setattr(out, name, fn(data[pos:pos + size]))
        pos += size
    out.ht_bytes = data[pos:pos + GT_BYTES]
    out.ht, out.ht_words = pm.from_bytes(out.ht_bytes), api.gt_from_bytes(out.ht_bytes)
    pos += GT_BYTES
    out.max_log_n = int.from_bytes(data[pos:pos + 8], "little")
    assert pos + 8 == LENGTH
    return out


def gt_values(cap):
    """the entries of the five vectors other than one, in file order: 5 * 9 - 4 = 41 of them, 25 distinct (delta_1l and delta_2l repeat
    chi[0..7]; ht repeats chi[0] and is left out) -> (model tuples, (41, 48) words)"""
    one = pm.to_bytes(pm.ONE)
    vals, words = [], []
    for name in VECTORS:
        for b, v, w in zip(getattr(cap, name + "_bytes"), getattr(cap, name), getattr(cap, name + "_words")):
            if b != one:
                vals.append(v)
                words.append(w)
    return vals, np.stack(words)
