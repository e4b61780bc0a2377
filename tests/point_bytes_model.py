"""The byte formats of include/zolt_gpu.h, "Points from bytes", restated on Python integers from the reference's own parsers — the model
the device kernels (zolt_amd/csrc/point_bytes.hip), their lane functions compiled for the host and the mirrors are held to:
  BE              parseG1Uncompressed / parseG2Uncompressed   src/poly/commitment/srs.zig:65-99, :165-203
  LE              parseG1LE / parseG2LE                       srs.zig:616-712
  ARK             DoryCommitmentScheme.parseG1Uncompressed / parseG2Uncompressed   src/poly/commitment/dory.zig:828-924
  ARK_COMPRESSED  decompressG1 / decompressG2, tonelliShanks, fp2Sqrt, yIsPositive, fp2IsPositive   dory.zig:81-344
A G1 point is (x, y), a G2 point ((x0, x1), (y0, y1)), canonical integers; None is the identity. Plain module: no fixtures, no pytest
hooks."""
import numpy as np

from tests import g2_model as G2
from tests import pairing_model as PM

P = G2.P
BE, LE, ARK, ARK_COMPRESSED = 0, 1, 2, 3
CHECK = 1
G1, G2_ = 1, 2
COORDS = {G1: 2, G2_: 4}
OK, NOT_ON_CURVE, NO_ROOT = 0, 1, 2
REASON = {NOT_ON_CURVE: "PointNotOnCurve", NO_ROOT: "DecompressionFailed"}


def record_bytes(group, encoding):
    return COORDS[group] * (16 if encoding == ARK_COMPRESSED else 32)


# ---------------------------------------------------------------- square roots and signs (dory.zig:124-175, :265-344)
def fp_sqrt(n):
    """tonelliShanks (:124-158): n^((p+1)/4), accepted only if its square is n; sqrt(0) = 0"""
    n %= P
    r = pow(n, (P + 1) // 4, P)
    return r if r * r % P == n else None


def fp2_sqrt(n):
    """fp2Sqrt (:265-316), branch for branch, and the case it leaves out: (a + |n|) / 2 and (|n| - a) / 2 multiply to (b / 2)^2, so they
    are squares together or not at all, and when neither is the reference returns null for a square n (about every second one; half of
    the G2 points of its own captured proof among them). Then (a - |n|) / 2 = -(|n| - a) / 2 is a square and gives the root."""
    a, b = n[0] % P, n[1] % P
    if a == 0 and b == 0:
        return (0, 0)
    if b == 0:
        s = fp_sqrt(a)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a % P)
        return None if s is None else (0, s)
    norm_sqrt = fp_sqrt((a * a + b * b) % P)
    if norm_sqrt is None:
        return None
    two_inv = pow(2, -1, P)
    c = fp_sqrt((a + norm_sqrt) * two_inv % P)
    if c is not None:
        return (c, b * pow(2 * c, -1, P) % P)
    d = fp_sqrt(-((a - norm_sqrt) * two_inv) % P)
    if d is not None:
        return (b * pow(2 * d, -1, P) % P, d)
    c = fp_sqrt((a - norm_sqrt) * two_inv % P)
    return None if c is None else (c, b * pow(2 * c, -1, P) % P)


def fp2_sqrt_branch(n):
    """which case of the device's Fp2 root (point_bytes.hip.h) n takes: 'zero', 'a1=0,+' / 'a1=0,-' (c^2 = +-delta with delta = a0),
    '+' / '-' (c^2 = +-delta with delta = (a0 + alpha) / 2), or 'none'"""
    a, b = n[0] % P, n[1] % P
    if a == 0 and b == 0:
        return "zero"
    alpha = fp_sqrt((a * a + b * b) % P)
    if alpha is None:
        return "none"
    delta = a if b == 0 else (a + alpha) * pow(2, -1, P) % P
    c = pow(delta, (P + 1) // 4, P)
    return ("a1=0," if b == 0 else "") + ("+" if c * c % P == delta else "-")


def y_is_positive(y):
    """yIsPositive (:162-175): y <= -y as integers"""
    return y <= -y % P


def fp2_is_positive(y):
    """fp2IsPositive (:320-344): c1 first, then c0"""
    n = G2.f2_neg(y)
    return (y[1], y[0]) <= (n[1], n[0])


def g1_rhs(x):
    return (x * x * x + 3) % P


def g2_rhs(x):
    return G2.f2_add(G2.f2_mul(G2.f2_sqr(x), x), G2.B_TWIST)


def on_curve(group, p):
    if group == G1:
        return p[1] * p[1] % P == g1_rhs(p[0])
    return G2.f2_sqr(p[1]) == g2_rhs(p[0])


# ---------------------------------------------------------------- one record
def decode(group, encoding, rec, flags=0):
    """-> (status, point): status OK with the point (None = identity), or NOT_ON_CURVE / NO_ROOT with None"""
    rec = bytes(rec)
    assert len(rec) == record_bytes(group, encoding)
    nc = COORDS[group]
    if encoding == ARK_COMPRESSED:
        flag = rec[-1] & 0xC0
        if flag == 0x40:  # :84, :217 — the other bytes are not looked at
            return OK, None
        rec = rec[:-1] + bytes([rec[-1] & 0x3F])
        c = [int.from_bytes(rec[32 * k:32 * k + 32], "little") % P for k in range(nc // 2)]
        if group == G1:
            x = c[0]
            y = fp_sqrt(g1_rhs(x))
            if y is None:
                return NO_ROOT, None
            if (flag == 0) != y_is_positive(y):
                y = -y % P
        else:
            x = (c[0], c[1])
            y = fp2_sqrt(g2_rhs(x))
            if y is None:
                return NO_ROOT, None
            if (flag == 0) != fp2_is_positive(y):
                y = G2.f2_neg(y)
        return OK, (x, y)
    if encoding == ARK:
        rec = rec[:-1] + bytes([rec[-1] & 0x3F])
    if not any(rec):
        return OK, None  # for ARK G2 a deviation from the reference, which has no identity rule there (include/zolt_gpu.h)
    c = [int.from_bytes(rec[32 * k:32 * k + 32], "big" if encoding == BE else "little") % P for k in range(nc)]
    if group == G1:
        p = (c[0], c[1])
    elif encoding == BE:
        p = ((c[1], c[0]), (c[3], c[2]))  # x.c1, x.c0, y.c1, y.c0
    else:
        p = ((c[0], c[1]), (c[2], c[3]))
    if flags & CHECK and not on_curve(group, p):
        return NOT_ON_CURVE, None
    return OK, p


def decode_all(group, encoding, data, flags=0):
    """-> (points, first_bad, reason): first_bad = n and reason None when every record is good"""
    size = record_bytes(group, encoding)
    n = len(data) // size
    pts = []
    for i in range(n):
        st, p = decode(group, encoding, data[size * i:size * i + size], flags)
        if st != OK:
            return None, i, REASON[st]
        pts.append(p)
    return pts, n, None


def pack(group, points):
    """the ABI's arrays of a list of points: (xy (n, 8 | 16) uint64 Montgomery, inf (n,) uint8)"""
    if group == G1:
        return PM.g1_pack(points)
    if not points:
        return np.zeros((0, 16), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    return G2.pack(points)


# ---------------------------------------------------------------- the other direction, to build vectors
def encode(group, encoding, p, top_bits=0, sign=None):
    """a record of p (None = identity). top_bits: ORed into the record's last byte (ARK's ignored flag bits); sign (compressed only):
    override the flag bits (0x00 / 0x80 / 0xC0) instead of deriving them from y"""
    nc = COORDS[group]
    if encoding == ARK_COMPRESSED:
        if p is None:
            return bytes(16 * nc - 1) + bytes([0x40])
        xs = [p[0]] if group == G1 else list(p[0])
        out = bytearray(b"".join(int(v).to_bytes(32, "little") for v in xs))
        positive = y_is_positive(p[1]) if group == G1 else fp2_is_positive(p[1])
        out[-1] |= (0 if positive else 0x80) if sign is None else sign
        return bytes(out)
    if p is None:
        out = bytearray(32 * nc)
    elif group == G1:
        out = bytearray(b"".join(int(v).to_bytes(32, "big" if encoding == BE else "little") for v in p))
    elif encoding == BE:
        out = bytearray(b"".join(int(v).to_bytes(32, "big") for v in (p[0][1], p[0][0], p[1][1], p[1][0])))
    else:
        out = bytearray(b"".join(int(v).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1])))
    out[-1] |= top_bits
    return bytes(out)


def g1_multiples(n, start=1):
    """start * G, (start + 1) * G, ... on y^2 = x^3 + 3"""
    out, p = [], PM.g1_mul(PM.G1_GEN, start)
    for _ in range(n):
        out.append(p)
        p = PM.g1_add(p, PM.G1_GEN)
    return out


def g2_multiples(n, start=1):
    out, p = [], G2.scalar_mul(G2.G, start)
    for _ in range(n):
        out.append(p)
        p = G2.add(p, G2.G)
    return out


# ---------------------------------------------------------------- the compressed points of the two captured files
def captured_open_points(data):
    """every compressed point of tests/golden/dory_open_captured.bin (DoryProof.toBytes, dory.zig:481-535) -> [(group, name, bytes)]:
    the VMV e1, each round's e1_beta and e2_beta, each round's e1_+, e1_-, e2_+, e2_-, the final pair"""
    rounds = int.from_bytes(data[800:804], "little")
    out = [(G1, "vmv.e1", data[768:800])]
    pos = 804
    for t in range(rounds):
        out += [(G1, f"first[{t}].e1_beta", data[pos + 1536:pos + 1568]), (G2_, f"first[{t}].e2_beta", data[pos + 1568:pos + 1632])]
        pos += 1632
    for t in range(rounds):
        out += [(G1, f"second[{t}].e1_plus", data[pos + 768:pos + 800]), (G1, f"second[{t}].e1_minus", data[pos + 800:pos + 832]),
                (G2_, f"second[{t}].e2_plus", data[pos + 832:pos + 896]), (G2_, f"second[{t}].e2_minus", data[pos + 896:pos + 960])]
        pos += 960
    out += [(G1, "final.e1", data[pos:pos + 32]), (G2_, "final.e2", data[pos + 32:pos + 96])]
    assert pos + 96 + 8 == len(data)
    return out
