"""Two restatements of DoryCommitmentScheme.open -> openWithRowCommitments (src/poly/commitment/dory.zig:1052-1378) — the opening the
prover calls, with 2^sigma G1 and 2^nu G2 generators and its constant challenges — that the device session begun over a key
(zg_dory_open_key_begin, zg_dory_open_run) and the host mirrors are held to. Nothing here touches the device.

(a) open_exponents: the whole of open over scalars mod r. Every G1 point is a known multiple of G = (1, 2), every G2 point a known
    multiple of H, and every GT value e(G, H)^x: a message is a handful of integers, rendered with one pairing and powers of it. An
    identity is the multiple 0. Fast at any size; it knows nothing of how a group law treats its special cases.
(b) open_points: the same lines over points, in the style of dory_open_model.open_model — GT and G2 from tests/pairing_model.py and
    tests/g2_model.py, G1 from the oracle — including identities and short rows / v_vec.

Messages are the flat uint64 records of include/zolt_gpu.h; ark_bytes is writeDoryProof (src/zkvm/jolt_serialization.zig:148-185)."""
import numpy as np

from tests import dory_open_model as D
from tests import g2_model as G2
from tests import pairing_model as PM

P, R = G2.P, G2.R


# ---------------------------------------------------------------- the schedule (:1211-1214, :1236-1252, :1291-1304, :1343-1344)
def schedule(nu, sigma):
    """[(cur, n2, row, h)] per round, as the reference's loop leaves them: two lengths that halve, the row length staying at 1"""
    assert nu <= sigma
    col, row, out = 1 << sigma, 1 << nu, []
    for _ in range(max(nu, sigma)):
        cur = max(col, row)
        n2 = cur // 2
        out.append((cur, n2, row, min(n2, row)))
        col = col // 2 if col > 1 else col
        row = row // 2 if row > 1 else row
    return out


def open_challenges(sigma):
    """beta = round + 1, alpha = round + 100 per round, gamma = 999 (:1274, :1316, :1349) -> integers [beta_0, alpha_0, ..., gamma]"""
    return [c for t in range(sigma) for c in (t + 1, t + 100)] + [999]


def inverse_or_one(x):
    return pow(x, -1, R) if x % R else 1


def challenge_words(values):
    """[beta_0, alpha_0, ..., gamma] -> what zg_dory_open_run takes: (beta, beta_inv, alpha, alpha_inv) per round, (gamma, gamma_inv)"""
    return G2.fr_pack([w for c in values for w in (c, inverse_or_one(c))]).reshape(-1)


# ---------------------------------------------------------------- open's inputs from evaluations and a point, as integers (:544-670)
def lagrange_basis(point, out_len):
    out = [0] * out_len
    if not point or not out_len:
        if out_len:
            out[0] = 1
        return out
    out[0] = (1 - point[0]) % R
    if out_len > 1:
        out[1] = point[0] % R
    for level in range(1, len(point)):
        p, mid = point[level], 1 << level
        if mid >= out_len:
            out = [v * (1 - p) % R for v in out]
        else:
            for i in reversed(range(min(mid, out_len - mid))):
                l = out[i]
                if i + mid < out_len:
                    out[i + mid] = l * p % R
                out[i] = l * (1 - p) % R
    return out


def evaluation_vectors(point, nu, sigma):
    left, right = [0] * (1 << nu), [0] * (1 << sigma)
    d = len(point)
    if d == 0:
        left[0] = right[0] = 1
    elif d <= sigma:
        right[:1 << d] = lagrange_basis(point, 1 << d)
        left[0] = 1
    elif d <= nu + sigma:
        right = lagrange_basis(point[:sigma], 1 << sigma)
        left[:1 << (d - sigma)] = lagrange_basis(point[sigma:], 1 << (d - sigma))
    else:
        right = lagrange_basis(point[:sigma], 1 << sigma)
        left = lagrange_basis(point[sigma:], 1 << nu)
    return left, right


def vector_matrix_product(evals, left, nu, sigma):
    cols = 1 << sigma
    out = [0] * cols
    for row in range(min(1 << nu, len(left))):
        for col in range(cols):
            if row * cols + col < len(evals):
                out[col] = (out[col] + left[row] * evals[row * cols + col]) % R
    return out


def row_scalars(a, evals, cols):
    """computeRowCommitments in the exponent: row r = sum_c a[c] evals[r cols + c] (a short last row over its own length)"""
    return [sum(a[c] * e for c, e in enumerate(evals[s:s + cols])) % R for s in range(0, len(evals), cols)]


# ---------------------------------------------------------------- (a) over scalars
def open_exponents(a, b, row_ks, v_vec, right_vec, left_vec, nu, sigma, challenges=None):
    """a: 2^sigma G1 generator scalars, b: 2^nu G2 generator scalars, row_ks: the row commitments' scalars (any number; 0 = identity).
    -> dict(vmv = (c, d2, e1), first = [(d1l, d1r, d2l, d2r, e1_beta, e2_beta)], second = [(c+, c-, e1+, e1-, e2+, e2-)],
    final = (e1, e2)): GT exponents, G1 multiples of G, G2 multiples of H"""
    n, nl = 1 << sigma, 1 << nu
    assert nu <= sigma and len(a) >= n and len(b) >= nl and len(v_vec) <= n and len(right_vec) == n and len(left_vec) == nl
    ch = list(open_challenges(sigma) if challenges is None else challenges)
    dot = lambda x, y: sum(p * q for p, q in zip(x, y)) % R  # noqa: E731  (zip: the shorter slice)
    v1 = ([k % R for k in row_ks[:n]] + [0] * n)[:n]
    out = {"vmv": (dot(v1, v_vec) * b[0] % R, dot(a[:len(v_vec)], v_vec) * b[0] % R, dot(v1[:nl], left_vec)), "first": [], "second": []}
    v2 = ([b[0] * v % R for v in v_vec] + [0] * n)[:n]
    s1, s2 = [x % R for x in right_vec], ([x % R for x in left_vec] + [0] * n)[:n]
    for cur, n2, row, h in schedule(nu, sigma):
        out["first"].append((dot(v1[:h], b[:h]), dot(v1[n2:n2 + h], b[:h]), dot(a[:n2], v2[:n2]), dot(a[:n2], v2[n2:cur]),
                             dot(a[:cur], s2[:cur]), dot(b[:row], s1[:row])))
        beta = ch.pop(0) % R
        beta_inv = inverse_or_one(beta)
        for i in range(cur):
            v1[i] = (v1[i] + beta * a[i]) % R
        for i in range(row):
            v2[i] = (v2[i] + beta_inv * b[i]) % R
        out["second"].append((dot(v1[:h], v2[n2:n2 + h]), dot(v1[n2:n2 + h], v2[:h]), dot(v1[:n2], s2[n2:cur]), dot(v1[n2:cur], s2[:n2]),
                              dot(v2[n2:n2 + h], s1[:h]), dot(v2[:h], s1[n2:n2 + h])))
        alpha = ch.pop(0) % R
        alpha_inv = inverse_or_one(alpha)
        for i in range(n2):
            v1[i] = (alpha * v1[i] + v1[i + n2]) % R
            s2[i] = (alpha_inv * s2[i] + s2[i + n2]) % R
        for i in range(h):
            v2[i] = (alpha_inv * v2[i] + v2[i + n2]) % R
            s1[i] = (alpha * s1[i] + s1[i + n2]) % R
    gamma = ch.pop(0) % R
    out["final"] = ((v1[0] + gamma * s1[0]) % R, (v2[0] + inverse_or_one(gamma) * s2[0]) % R)
    return out


_E = []


def gt_of(x):
    """e(G, H)^x"""
    if not _E:
        _E.append(PM.pairing(PM.G1_GEN, G2.G))
    return PM.power(_E[0], x % R) if x % R else PM.ONE


def g1_of(k):
    return PM.g1_mul(PM.G1_GEN, k % R)


def g2_of(k):
    return G2.scalar_mul(G2.G, k % R)


def _g1_rec(k):
    xy, inf = PM.g1_pack([g1_of(k)])
    return D.g1_rec(xy[0], int(inf[0]))


def render(sym):
    """open_exponents' integers -> the message records: dict(vmv (105,), first [(218,)], second [(148,)], final (26,))"""
    gts = lambda xs: PM.gt_pack([gt_of(x) for x in xs]).reshape(-1)  # noqa: E731
    c, d2, e1 = sym["vmv"]
    out = {"vmv": np.concatenate([gts((c, d2)), _g1_rec(e1)]), "first": [], "second": []}
    for m in sym["first"]:
        out["first"].append(np.concatenate([gts(m[:4]), _g1_rec(m[4]), D.g2_rec(g2_of(m[5]))]))
    for m in sym["second"]:
        out["second"].append(np.concatenate([gts(m[:2]), _g1_rec(m[2]), _g1_rec(m[3]), D.g2_rec(g2_of(m[4])), D.g2_rec(g2_of(m[5]))]))
    out["final"] = np.concatenate([_g1_rec(sym["final"][0]), D.g2_rec(g2_of(sym["final"][1]))])
    return out


def ark_bytes(rec, nu, sigma):
    """writeDoryProof (jolt_serialization.zig:148-185) of message records: DoryProof.toBytes' values in the same order — the round count
    as a u32 after the VMV message, nu and sigma as u32 at the end"""
    return D.proof_bytes(rec["vmv"], rec["first"], rec["second"], rec["final"], nu, sigma)


def ark_bytes_of_exponents(sym, nu, sigma):
    """the same straight from the integers, without the detour through limbs"""
    gt = lambda x: PM.to_bytes(gt_of(x))  # noqa: E731
    g1 = lambda k: D.compress_g1(g1_of(k))  # noqa: E731
    g2 = lambda k: G2.compress(g2_of(k))  # noqa: E731
    c, d2, e1 = sym["vmv"]
    out = gt(c) + gt(d2) + g1(e1) + len(sym["first"]).to_bytes(4, "little")
    for m in sym["first"]:
        out += b"".join(gt(x) for x in m[:4]) + g1(m[4]) + g2(m[5])
    for m in sym["second"]:
        out += gt(m[0]) + gt(m[1]) + g1(m[2]) + g1(m[3]) + g2(m[4]) + g2(m[5])
    return out + g1(sym["final"][0]) + g2(sym["final"][1]) + int(nu).to_bytes(4, "little") + int(sigma).to_bytes(4, "little")


# ---------------------------------------------------------------- (b) over points (:1062-1378)
def open_points(g1_vec, g2_pts, rows, v_vec, right_vec, left_vec, nu, sigma, challenges=None):
    """g1_vec / rows: (xy, inf) arrays (inf may be None); g2_pts: [point or None], 2^nu of them; scalars: integer lists (v_vec at most
    2^sigma entries — the reference's own v_vec has exactly 2^sigma —, right_vec 2^sigma, left_vec 2^nu) -> the message records"""
    from oracle import binding as ob
    n, nl = 1 << sigma, 1 << nu
    assert nu <= sigma and len(g2_pts) >= nl and len(v_vec) <= n and len(right_vec) == n and len(left_vec) == nl
    ch = list(open_challenges(sigma) if challenges is None else challenges)
    g1 = (np.asarray(g1_vec[0], dtype=np.uint64).reshape(-1, 8)[:n], np.zeros(n, dtype=np.uint8) if g1_vec[1] is None else np.asarray(g1_vec[1], dtype=np.uint8)[:n])
    g2 = list(g2_pts[:nl])
    g1_pts = D._g1_points(g1)
    rows_xy = np.asarray(rows[0], dtype=np.uint64).reshape(-1, 8)
    rows_inf = np.zeros(rows_xy.shape[0], dtype=np.uint8) if rows[1] is None else np.asarray(rows[1], dtype=np.uint8)
    k = min(rows_xy.shape[0], n)
    v1 = (np.zeros((n, 8), dtype=np.uint64), np.ones(n, dtype=np.uint8))  # :1095-1114: truncated, or padded with identities
    v1[0][:k], v1[1][:k] = rows_xy[:k], rows_inf[:k]
    v1[0][v1[1] != 0] = 0
    v_sc, left_sc = G2.fr_pack(v_vec), G2.fr_pack(left_vec)
    # the VMV message (:1116-1162)
    t_rec = D._g1_msm(v1, v_sc)
    gamma_rec = D._g1_msm(g1, v_sc)
    c, d2 = PM.pairing(D.g1_point(t_rec), g2[0]), PM.pairing(D.g1_point(gamma_rec), g2[0])
    e1 = D._g1_msm((v1[0][:nl], v1[1][:nl]), left_sc)
    out = {"vmv": np.concatenate([PM.gt_pack([c, d2]).reshape(-1), e1]), "first": [], "second": []}
    v2 = [G2.scalar_mul(g2[0], s % R) for s in v_vec] + [None] * (n - len(v_vec))  # :1179-1187
    s1, s2 = [int(x) % R for x in right_vec], [int(x) % R for x in left_vec] + [0] * (n - nl)
    sub = lambda v, lo, hi: (v[0][lo:hi], v[1][lo:hi])  # noqa: E731
    for cur, n2, row, h in schedule(nu, sigma):
        v1_pts = D._g1_points(sub(v1, 0, cur))
        gts = [PM.multi_pairing(v1_pts[:h], g2[:h]), PM.multi_pairing(v1_pts[n2:n2 + h], g2[:h]),
               PM.multi_pairing(g1_pts[:n2], v2[:n2]), PM.multi_pairing(g1_pts[:n2], v2[n2:cur])]
        e1_beta = D._g1_msm(sub(g1, 0, cur), G2.fr_pack(s2[:cur]))
        e2_beta = G2.msm(g2[:row], s1[:row])
        out["first"].append(np.concatenate([PM.gt_pack(gts).reshape(-1), e1_beta, D.g2_rec(e2_beta)]))
        beta = ch.pop(0) % R
        beta_inv = inverse_or_one(beta)
        upd = D._g1_axpy(sub(g1, 0, cur), sub(v1, 0, cur), G2.fr_pack([beta])[0])  # :1279-1286
        v1[0][:cur], v1[1][:cur] = upd
        for i in range(row):
            v2[i] = G2.add(v2[i], G2.scalar_mul(g2[i], beta_inv))
        v1_pts = D._g1_points(sub(v1, 0, cur))
        gts = [PM.multi_pairing(v1_pts[:h], v2[n2:n2 + h]), PM.multi_pairing(v1_pts[n2:n2 + h], v2[:h])]
        e1_plus = D._g1_msm(sub(v1, 0, n2), G2.fr_pack(s2[n2:cur]))
        e1_minus = D._g1_msm(sub(v1, n2, cur), G2.fr_pack(s2[:n2]))
        e2_plus, e2_minus = G2.msm(v2[n2:n2 + h], s1[:h]), G2.msm(v2[:h], s1[n2:n2 + h])
        out["second"].append(np.concatenate([PM.gt_pack(gts).reshape(-1), e1_plus, e1_minus, D.g2_rec(e2_plus), D.g2_rec(e2_minus)]))
        alpha = ch.pop(0) % R
        alpha_inv = inverse_or_one(alpha)
        fold = D._g1_axpy(sub(v1, 0, n2), sub(v1, n2, cur), G2.fr_pack([alpha])[0])  # :1321-1340
        v1[0][:n2], v1[1][:n2] = fold
        for i in range(n2):
            s2[i] = (alpha_inv * s2[i] + s2[i + n2]) % R
        for i in range(h):
            v2[i] = G2.add(G2.scalar_mul(v2[i], alpha_inv), v2[i + n2])
            s1[i] = (alpha * s1[i] + s1[i + n2]) % R
    gamma = ch.pop(0) % R
    gen = PM.g1_pack([PM.G1_GEN])[0][0]
    sx, si = ob.g1_scalar_mul(gen, 0, G2.fr_pack([gamma * s1[0] % R])[0])
    fx, fi = ob.g1_add_affine(v1[0][0], int(v1[1][0]), sx, si)
    final_e2 = G2.add(v2[0], G2.scalar_mul(G2.G, inverse_or_one(gamma) * s2[0] % R))
    out["final"] = np.concatenate([D.g1_rec(fx, fi), D.g2_rec(final_e2)])
    return out


# ---------------------------------------------------------------- inputs as known multiples of the generators
def make_inputs(nu, sigma, seed, n_rows=None, n_v=None, identity_rows=(), left_zero_tail=0, identity_g1=(), identity_g2=()):
    """Seeded inputs whose every point is a known multiple: dict(a, b, row_ks, v_vec, right_vec, left_vec (integers), g1_vec, rows
    ((xy, inf) arrays), g2_pts, g2_vec ((xy, inf)), nu, sigma). An identity is the multiple 0."""
    import random
    rng = random.Random(seed)
    n, nl = 1 << sigma, 1 << nu
    n_rows = nl if n_rows is None else n_rows
    a = [0 if i in identity_g1 else rng.randrange(1, 1 << 20) for i in range(n)]
    b = [0 if i in identity_g2 else rng.randrange(1, R) for i in range(nl)]
    row_ks = [0 if i in identity_rows else rng.randrange(1, 1 << 20) for i in range(n_rows)]
    v_vec = [rng.randrange(R) for _ in range(n if n_v is None else n_v)]
    left = [rng.randrange(R) for _ in range(nl)]
    for i in range(left_zero_tail):
        left[nl - 1 - i] = 0
    g2_pts = [g2_of(x) for x in b]
    return {"a": a, "b": b, "row_ks": row_ks, "v_vec": v_vec, "right_vec": [rng.randrange(R) for _ in range(n)], "left_vec": left,
            "g1_vec": PM.g1_pack([g1_of(x) for x in a]), "rows": PM.g1_pack([g1_of(x) for x in row_ks]), "g2_pts": g2_pts, "g2_vec": G2.pack(g2_pts),
            "nu": nu, "sigma": sigma}


def exponents_of(inp, challenges=None):
    return open_exponents(inp["a"], inp["b"], inp["row_ks"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"], challenges)


def points_of(inp, challenges=None):
    return open_points(inp["g1_vec"], inp["g2_pts"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"], challenges)


def same_records(x, y):
    return (np.array_equal(x["vmv"], y["vmv"]) and len(x["first"]) == len(y["first"]) and len(x["second"]) == len(y["second"])
            and all(np.array_equal(p, q) for p, q in zip(x["first"], y["first"])) and all(np.array_equal(p, q) for p, q in zip(x["second"], y["second"]))
            and np.array_equal(x["final"], y["final"]))


# ---------------------------------------------------------------- the captured run: open(setup(9), bytecode_evals, point)
def captured_inputs(elf_bytes, setup_scalars):
    """serializeJoltProofWithDory's call (src/zkvm/mod.zig:1471-1490): evals = fromU64 of the 104 program bytes at 0x1000, zero-padded
    to 128 (:848, :868-875); point[i] = (i + 1) * 12345; setup_scalars = api.Dory.setupScalars(9) = (sigma, nu, a, b)"""
    sigma, nu, a, b = setup_scalars
    evals = list(elf_bytes[0x1000:0x1000 + 104]) + [0] * 24
    point = [(i + 1) * 12345 % R for i in range(9)]
    left, right = evaluation_vectors(point, nu, sigma)
    return {"a": a, "b": b, "row_ks": row_scalars(a, evals, 1 << sigma), "v_vec": vector_matrix_product(evals, left, nu, sigma), "right_vec": right,
            "left_vec": left, "nu": nu, "sigma": sigma, "evals": evals, "point": point}


def setup_scalars(max_num_vars):
    """setup's generator scalars (:931-979, generateG1Point / generateG2Point :1675-1712): Fr.fromBytes(SHA3-256(seed || u64le(index) ||
    "G1" | "G2")), seed = SHA3-256("Jolt Dory URS seed"), the G2 indices offset by the number of columns -> (sigma, nu, a, b)"""
    import hashlib
    sigma = (int(max_num_vars) + 1) // 2
    nu = int(max_num_vars) - sigma
    seed = hashlib.sha3_256(b"Jolt Dory URS seed").digest()
    scalar = lambda index, tag: int.from_bytes(hashlib.sha3_256(seed + int(index).to_bytes(8, "little") + tag).digest(), "little") % R  # noqa: E731
    cols = 1 << sigma
    return sigma, nu, [scalar(i, b"G1") for i in range(cols)], [scalar(i + cols, b"G2") for i in range(1 << nu)]
