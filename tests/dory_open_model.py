"""A straight restatement of DoryCommitmentScheme.openWithTranscript (src/poly/commitment/dory.zig:1404-1669) — the model the device
session (zg_dory_open_*) and the host mirrors are held to. GT and G2 are the big-integer models of tests/pairing_model.py and
tests/g2_model.py, G1 the oracle's restatements of MSM.compute / MSM.scalarMul / AffinePoint.add (oracle.binding), the transcript the
Blake2b one of src/transcripts/blake2b.zig with its three Dory appenders (:496-546), the bytes DoryProof.toBytes (:481-535) over
compressG1 (:51-78) and compressG2 (:179-210). Nothing here touches the device.

Messages come out as the flat uint64 records of include/zolt_gpu.h ("Dory opening (session)"): GT = 48 words, a G1 point xy[8] + flag
word (identity written x = y = 0), a G2 point xy[16] + flag word (identity written as G2Point.identity())."""
import hashlib

import numpy as np

from oracle import binding as ob
from tests import g2_model as G2
from tests import pairing_model as PM

P, R = G2.P, G2.R
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------- compressG1 / decompressG1 (dory.zig:51-120, yIsPositive :162-175)
def compress_g1(p):
    """p = (x, y) canonical integers, or None for the identity -> 32 bytes"""
    if p is None:
        return bytes(31) + bytes([0x40])
    out = bytearray(p[0].to_bytes(32, "little"))
    positive = p[1] <= (-p[1]) % P  # y <= -y as integers; equal counts as positive
    out[31] = (out[31] & 0x3F) | (0 if positive else 0x80)
    return bytes(out)


def decompress_g1(b):
    flag = b[31] & 0xC0
    if flag == 0x40:
        return None
    x = int.from_bytes(bytes(b[:31]) + bytes([b[31] & 0x3F]), "little") % P
    y2 = (x * x * x + 3) % P
    y = pow(y2, (P + 1) // 4, P)  # p = 3 mod 4
    if y * y % P != y2:
        raise ValueError("not an x-coordinate of the curve")
    if (flag == 0) != (y <= (-y) % P):
        y = (-y) % P
    return (x, y)


# ---------------------------------------------------------------- the transcript (blake2b.zig:25-93, 123-156, 215-266, 496-546)
class Transcript:
    def __init__(self, label=b"Jolt"):
        self.state = hashlib.blake2b(bytes(label).ljust(32, b"\0"), digest_size=32).digest()
        self.n_rounds = 0

    def _hash_with(self, payload):
        self.state = hashlib.blake2b(self.state + bytes(28) + self.n_rounds.to_bytes(4, "big") + bytes(payload), digest_size=32).digest()
        self.n_rounds += 1
        return self.state

    def appendBytes(self, data):
        self._hash_with(data)

    def appendGT(self, f):  # Fp12.toBytes, all 384 bytes reversed
        self.appendBytes(PM.to_bytes(f)[::-1])

    def appendG1Compressed(self, p):
        self.appendBytes(compress_g1(p))

    def appendG2Compressed(self, q):
        self.appendBytes(G2.compress(q))

    def challengeScalar(self):  # 16 bytes, reversed, 125-bit mask, RAW limbs [0, 0, low, high]
        v = int.from_bytes(self._hash_with(b"")[:16][::-1], "big") & ((1 << 125) - 1)
        return np.array([0, 0, v & _M64, v >> 64], dtype=np.uint64)


class FixedChallenges:
    """the transcript replaced by a list of challenges (integers; handed out as Montgomery limbs): what the benches and the
    session-against-composition test drive both routes with"""

    def __init__(self, values):
        self.values = list(values)

    def appendGT(self, f):
        pass

    appendG1Compressed = appendG2Compressed = appendGT

    def challengeScalar(self):
        return G2.fr_pack([self.values.pop(0)])[0]


# ---------------------------------------------------------------- records
def g1_rec(xy, inf):
    out = np.zeros(9, dtype=np.uint64)
    if inf:
        out[8] = 1
    else:
        out[:8] = xy
    return out


def g2_rec(q):
    xy, inf = G2.pack([q])
    return np.concatenate([xy[0], np.array([inf[0]], dtype=np.uint64)])


def g1_point(rec):
    """a 9-word record -> (x, y) or None"""
    return PM.g1_unpack(rec[:8], [int(rec[8]) & 1])[0]


def g2_point(rec):
    return G2.unpack(rec[:16], [int(rec[16]) & 1])[0]


def proof_bytes(vmv, firsts, seconds, final, nu, sigma):
    """DoryProof.toBytes (:481-535) from the message records"""
    gt = lambda w: PM.to_bytes(PM.gt_unpack(w)[0])  # noqa: E731
    out = gt(vmv[0:48]) + gt(vmv[48:96]) + compress_g1(g1_point(vmv[96:105])) + len(firsts).to_bytes(4, "little")
    for m in firsts:
        out += b"".join(gt(m[48 * k:48 * k + 48]) for k in range(4)) + compress_g1(g1_point(m[192:201])) + G2.compress(g2_point(m[201:218]))
    for m in seconds:
        out += gt(m[0:48]) + gt(m[48:96]) + compress_g1(g1_point(m[96:105])) + compress_g1(g1_point(m[105:114]))
        out += G2.compress(g2_point(m[114:131])) + G2.compress(g2_point(m[131:148]))
    out += compress_g1(g1_point(final[0:9])) + G2.compress(g2_point(final[9:26]))
    return out + int(nu).to_bytes(4, "little") + int(sigma).to_bytes(4, "little")


# ---------------------------------------------------------------- G1 vectors on the oracle: (xy (n, 8), inf (n,)), identity rows zero
def _g1_msm(v, scalars):
    n = min(v[0].shape[0], scalars.shape[0])
    if n == 0:
        return g1_rec(None, 1)
    xy, inf = ob.msm_g1(v[0][:n], v[1][:n], scalars[:n])
    return g1_rec(xy, inf)


def _g1_axpy(a, b, s):
    """out[i] = AffinePoint.add(MSM.scalarMul(a[i], s).toAffine(), b[i])"""
    out = (np.zeros_like(b[0]), np.zeros_like(b[1]))
    for i in range(b[0].shape[0]):
        sx, si = ob.g1_scalar_mul(a[0][i], int(a[1][i]), s)
        xy, inf = ob.g1_add_affine(sx, si, b[0][i], int(b[1][i]))
        out[1][i] = inf
        if not inf:
            out[0][i] = xy
    return out


def _g1_points(v):
    return PM.g1_unpack(v[0], v[1])


def _inverse_or_one(c):
    """(challenge limbs) -> (integer, integer of `inverse() orelse one`, limbs of the latter)"""
    x = G2.fr_unpack(c)[0]
    xi = pow(x, -1, R) if x else 1
    return x, xi, G2.fr_pack([xi])[0]


def open_model(g1_vec, g2_vec, rows, v_vec, right_vec, left_vec, nu, sigma, transcript):
    """g1_vec / rows: (xy, inf) arrays; g2_vec: [point or None]; the scalar vectors: integer lists (v_vec at most 2^sigma, right_vec
    2^sigma, left_vec 2^nu entries). Returns a dict: vmv, first[], second[], final (records), states[] = (v1, v2, s1, s2) after every fold
    (v1 as (xy, inf), v2 a point list, s1 / s2 integer lists), challenges[] = (beta, beta_inv, alpha, alpha_inv) limbs per round, gamma,
    gamma_inv, proof (bytes), first_round (d1_left, d1_right as Fp12 values, and the v1 / g2 points they pair)."""
    assert nu <= sigma
    n, n_left = 1 << sigma, 1 << nu
    g1 = (np.asarray(g1_vec[0], dtype=np.uint64).reshape(-1, 8)[:n], np.zeros(n, dtype=np.uint8) if g1_vec[1] is None else np.asarray(g1_vec[1], dtype=np.uint8)[:n])
    g2 = list(g2_vec[:n])
    g1_pts = _g1_points(g1)
    rows_xy = np.asarray(rows[0], dtype=np.uint64).reshape(-1, 8)
    rows_inf = np.zeros(rows_xy.shape[0], dtype=np.uint8) if rows[1] is None else np.asarray(rows[1], dtype=np.uint8)
    k = min(rows_xy.shape[0], n)
    v1 = (np.zeros((n, 8), dtype=np.uint64), np.ones(n, dtype=np.uint8))  # :1438-1453: truncated or padded with identities
    v1[0][:k], v1[1][:k] = rows_xy[:k], rows_inf[:k]
    v1[0][v1[1] != 0] = 0
    v_sc, right_sc, left_sc = G2.fr_pack(v_vec), G2.fr_pack(right_vec), G2.fr_pack(left_vec)
    assert len(v_vec) <= n and len(right_vec) == n and len(left_vec) == n_left
    # the VMV message (:1456-1495)
    t_rec = _g1_msm(v1, v_sc)
    gamma_rec = _g1_msm(g1, v_sc)
    c = PM.pairing(g1_point(t_rec), g2[0])
    d2 = PM.pairing(g1_point(gamma_rec), g2[0])
    e1 = _g1_msm((v1[0][:n_left], v1[1][:n_left]), left_sc)
    vmv = np.concatenate([PM.gt_pack([c, d2]).reshape(-1), e1])
    transcript.appendGT(c)
    transcript.appendGT(d2)
    transcript.appendG1Compressed(g1_point(e1))
    # the working arrays (:1502-1533)
    v2 = [G2.scalar_mul(g2[0], s) for s in v_vec] + [None] * (n - len(v_vec))
    s1 = [int(x) % R for x in right_vec]
    s2 = [int(x) % R for x in left_vec] + [0] * (n - n_left)
    out = {"vmv": vmv, "first": [], "second": [], "states": [], "challenges": [], "first_round": None}
    cur = n
    for _ in range(sigma):  # max(nu, sigma) rounds
        n2 = cur // 2
        v1_pts = _g1_points((v1[0][:cur], v1[1][:cur]))
        d1_left = PM.multi_pairing(v1_pts[:n2], g2[:n2])
        d1_right = PM.multi_pairing(v1_pts[n2:cur], g2[:n2])
        d2_left = PM.multi_pairing(g1_pts[:n2], v2[:n2])
        d2_right = PM.multi_pairing(g1_pts[:n2], v2[n2:cur])
        e1_beta = _g1_msm((g1[0][:cur], g1[1][:cur]), G2.fr_pack(s2[:cur]))
        e2_beta = G2.msm(g2[:cur], s1[:cur])
        if out["first_round"] is None:
            out["first_round"] = (d1_left, d1_right, v1_pts, g2[:cur])
        out["first"].append(np.concatenate([PM.gt_pack([d1_left, d1_right, d2_left, d2_right]).reshape(-1), e1_beta, g2_rec(e2_beta)]))
        for f in (d1_left, d1_right, d2_left, d2_right):
            transcript.appendGT(f)
        transcript.appendG1Compressed(g1_point(e1_beta))
        transcript.appendG2Compressed(e2_beta)
        beta_l = transcript.challengeScalar()
        _, beta_inv, beta_inv_l = _inverse_or_one(beta_l)
        # apply the first challenge (:1578-1584)
        v1 = _g1_axpy((g1[0][:cur], g1[1][:cur]), (v1[0][:cur], v1[1][:cur]), beta_l)
        v2 = [G2.add(v2[i], G2.scalar_mul(g2[i], beta_inv)) for i in range(cur)]
        v1_pts = _g1_points(v1)
        c_plus = PM.multi_pairing(v1_pts[:n2], v2[n2:cur])
        c_minus = PM.multi_pairing(v1_pts[n2:cur], v2[:n2])
        e1_plus = _g1_msm((v1[0][:n2], v1[1][:n2]), G2.fr_pack(s2[n2:cur]))
        e1_minus = _g1_msm((v1[0][n2:cur], v1[1][n2:cur]), G2.fr_pack(s2[:n2]))
        e2_plus = G2.msm(v2[n2:cur], s1[:n2])
        e2_minus = G2.msm(v2[:n2], s1[n2:cur])
        out["second"].append(np.concatenate([PM.gt_pack([c_plus, c_minus]).reshape(-1), e1_plus, e1_minus, g2_rec(e2_plus), g2_rec(e2_minus)]))
        transcript.appendGT(c_plus)
        transcript.appendGT(c_minus)
        transcript.appendG1Compressed(g1_point(e1_plus))
        transcript.appendG1Compressed(g1_point(e1_minus))
        transcript.appendG2Compressed(e2_plus)
        transcript.appendG2Compressed(e2_minus)
        alpha_l = transcript.challengeScalar()
        alpha, alpha_inv, alpha_inv_l = _inverse_or_one(alpha_l)
        # fold (:1615-1634)
        v1 = _g1_axpy((v1[0][:n2], v1[1][:n2]), (v1[0][n2:cur], v1[1][n2:cur]), alpha_l)
        v2 = [G2.add(G2.scalar_mul(v2[i], alpha_inv), v2[i + n2]) for i in range(n2)]
        s1 = [(alpha * s1[i] + s1[i + n2]) % R for i in range(n2)]
        s2 = [(alpha_inv * s2[i] + s2[i + n2]) % R for i in range(n2)]
        cur = n2
        out["challenges"].append((beta_l, beta_inv_l, alpha_l, alpha_inv_l))
        out["states"].append(((v1[0].copy(), v1[1].copy()), list(v2), list(s1), list(s2)))
    gamma_l = transcript.challengeScalar()
    gamma, gamma_inv, gamma_inv_l = _inverse_or_one(gamma_l)
    # the final message (:1641-1655)
    gen = PM.g1_pack([PM.G1_GEN])[0][0]
    sx, si = ob.g1_scalar_mul(gen, 0, G2.fr_pack([gamma * s1[0] % R])[0])
    fx, fi = ob.g1_add_affine(v1[0][0], int(v1[1][0]), sx, si)
    final_e2 = G2.add(v2[0], G2.scalar_mul(G2.G, gamma_inv * s2[0] % R))
    out["final"] = np.concatenate([g1_rec(fx, fi), g2_rec(final_e2)])
    transcript.challengeScalar()  # the final d challenge keeps the transcript in sync (:1658)
    out["gamma"], out["gamma_inv"] = gamma_l, gamma_inv_l
    out["proof"] = proof_bytes(vmv, out["first"], out["second"], out["final"], nu, sigma)
    return out


def make_inputs(nu, sigma, seed, n_rows=None, n_v=None, zero_v=(), left_zero_tail=0):
    """Seeded inputs of an opening: g1_vec[i] = (i + 1) G, row commitment i = (2^sigma + i + 1) G (n_rows of them, default 2^nu),
    g2_vec[i] = h_i H for random h_i, random scalars — v_vec with zeros at `zero_v`, left_vec with `left_zero_tail` zeros at its end.
    -> dict(g1_vec, g2_vec (xy, inf), g2_pts, rows, row_ks, v_vec, right_vec, left_vec (integer lists), nu, sigma)"""
    import random
    rng = random.Random(seed)
    n, n_left = 1 << sigma, 1 << nu
    n_rows = n_left if n_rows is None else n_rows
    gm = ob.g1_gen_multiples(n + max(n_rows, 1))
    g2_pts = [G2.scalar_mul(G2.G, rng.randrange(1, R)) for _ in range(n)]
    v_vec = [rng.randrange(R) for _ in range(n if n_v is None else n_v)]
    for i in zero_v:
        v_vec[i] = 0
    left_vec = [rng.randrange(R) for _ in range(n_left)]
    for i in range(left_zero_tail):
        left_vec[n_left - 1 - i] = 0
    return {"g1_vec": (gm[:n].copy(), np.zeros(n, dtype=np.uint8)), "g2_vec": G2.pack(g2_pts), "g2_pts": g2_pts,
            "rows": (gm[n:n + n_rows].copy(), np.zeros(n_rows, dtype=np.uint8)), "row_ks": [n + i + 1 for i in range(n_rows)],
            "v_vec": v_vec, "right_vec": [rng.randrange(R) for _ in range(n)], "left_vec": left_vec, "nu": nu, "sigma": sigma}


def run_model(inp, transcript):
    return open_model(inp["g1_vec"], inp["g2_pts"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"], transcript)
