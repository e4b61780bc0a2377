"""G2 on the device (zg_g2_*, zg_msm_g2*, zg_g1_axpy_batch) and the group side of Dory's reduce-and-fold rounds, against the
big-integer model of tests/g2_model.py (pinned by tests/test_g2_model.py), closed forms, and second device paths.

Where outputs are sampled (scalar multiplications, axpy) the sample is at most 64 indices drawn by a seeded generator, always with the
first and the last element; every other output is still covered by an all-n equality against another device path."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import g2_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = M.R, M.P


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


def _sample(seed, n, k=64):
    if n <= k:
        return list(range(n))
    rng = random.Random(seed)
    return sorted({0, n - 1} | set(rng.sample(range(1, n - 1), k - 2)))


def _gen_xy():
    return M.pack([M.G])[0][0]


def _multiples(zl, ks):
    """k_i * G on the device (fixed base) -> (xy, inf)"""
    return zl.g2_fixed_base_mul_batch(_gen_xy(), M.fr_pack(ks))


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1]).reshape(-1), np.asarray(want[1]).reshape(-1))


# ---------------------------------------------------------------- 1. Fp2
def test_fp2_mul_square_inverse(zl):
    rng = random.Random(1)
    x = rng.randrange(1, P)
    edge = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (P - 1, P - 1), (0, x), (x, 0), (1, 1), (x, P - x)]
    a = edge + [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]
    b = [(rng.randrange(P), rng.randrange(P)) for _ in edge] + edge * 2 + [(rng.randrange(P), rng.randrange(P)) for _ in range(200 - 2 * len(edge))]
    assert len(a) == len(b)
    pa, pb = M.f2_pack(a).reshape(-1, 4), M.f2_pack(b).reshape(-1, 4)
    assert M.f2_unpack(zl.field_op(zl.FP, zl.OP_FP2_MUL, pa, pb)) == [M.f2_mul(u, v) for u, v in zip(a, b)]
    assert M.f2_unpack(zl.field_op(zl.FP, zl.OP_FP2_SQR, pa)) == [M.f2_sqr(u) for u in a]
    inv = M.f2_unpack(zl.field_op(zl.FP, zl.OP_FP2_INV, pa))
    assert inv == [M.f2_inv(u) for u in a] and inv[0] == (0, 0)
    with pytest.raises(zl.ZgError):  # an odd number of Fp elements is not a vector of Fp2 elements
        zl.field_op(zl.FP, zl.OP_FP2_SQR, pa[:3])
    with pytest.raises(zl.ZgError):
        zl.field_op(zl.FR, zl.OP_FP2_SQR, pa)


# ---------------------------------------------------------------- 2. affine add, on-curve
def test_affine_add_and_on_curve(zl):
    rng = random.Random(2)
    ks = [rng.randrange(1, R) for _ in range(40)]
    pts = [M.scalar_mul(M.G, k) for k in ks]
    a = pts[:20] + [pts[0], None, None, pts[1], pts[2], pts[3], M.G, M.neg(M.G)]
    b = pts[20:] + [None, pts[0], None, pts[1], M.neg(pts[2]), pts[3], M.G, M.G]
    # P + identity, identity + P, identity + identity, P + P, P + (-P), equal x by construction (twice), -G + G
    (axy, ainf), (bxy, binf) = M.pack(a), M.pack(b)
    want = M.pack([M.add(p, q) for p, q in zip(a, b)])
    got = zl.g2_affine_add_batch(axy, ainf, bxy, binf)
    assert _same(got, want)
    assert list(got[1][20:]) == [0, 0, 1, 0, 1, 0, 0, 1]
    # on input only the flag counts: garbage coordinates under a set flag change nothing
    axy2 = axy.copy()
    axy2[21] = 0xdeadbeef
    assert _same(zl.g2_affine_add_batch(axy2, ainf, bxy, binf), want)
    # flags may be NULL when there are no identities
    assert _same(zl.g2_affine_add_batch(axy[:20], None, bxy[:20], None), (want[0][:20], want[1][:20]))
    on = zl.g2_is_on_curve_batch(axy, ainf)
    assert list(on) == [1] * len(a)
    bad = axy.copy()
    bad[0, 8] ^= np.uint64(1)
    bad[21] = 0
    assert list(zl.g2_is_on_curve_batch(bad, ainf)[:3]) == [0, 1, 1]
    assert zl.g2_is_on_curve_batch(bad[21:22])[0] == 0  # (0, 0) without the flag is not on the twist


def test_affine_add_equal_x_unrelated_y_doubles_the_first_operand(zl):
    """Inputs the ABI cannot rule out: Q = (P.x, P.y + 1) is on no curve, and G2Point.add (pairing.zig:839-859) has no case for it — equal
    x that is not P + (-P) goes to self.double(). Every pair equals the model's add, which is double(P); a point with y = 0 added to
    itself is P + (-P), the identity, written (0, (1, 0))."""
    rng = random.Random(21)
    pts = [M.scalar_mul(M.G, rng.randrange(1, R)) for _ in range(8)]
    a = pts + [((5, 7), (0, 0))]
    b = [(p[0], M.f2_add(p[1], (1, 0))) for p in pts] + [((5, 7), (0, 0))]
    (axy, ainf), (bxy, binf) = M.pack(a), M.pack(b)
    want = [M.add(p, q) for p, q in zip(a, b)]
    assert want[:8] == [M.double(p) for p in pts] and want[8] is None
    got = zl.g2_affine_add_batch(axy, ainf, bxy, binf)
    assert _same(got, M.pack(want))
    assert list(got[1]) == [0] * 8 + [1] and list(got[0][8]) == M.IDENTITY_WORDS


# ---------------------------------------------------------------- 3. scalar multiplication, per pair and fixed base
SPECIAL = [0, 1, 2, R - 1, R - 2, 1 << 64, (1 << 64) - 1, 1 << 128, (1 << 200) - 1, 1 << 253, 255, 256, (1 << 32) - 1, 1 << 32]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_scalar_mul_batch_and_fixed_base(zl, n):
    rng = random.Random(30 + n)
    sc = [(SPECIAL[i] if i < len(SPECIAL) and n > 1 else rng.randrange(R)) for i in range(n)]
    if n > 20:
        sc[-1] = R - 1
    base = M.scalar_mul(M.G, 0xC0FFEE)
    bxy, _ = M.pack([base])
    fx = zl.g2_fixed_base_mul_batch(bxy[0], M.fr_pack(sc))
    sm = zl.g2_scalar_mul_batch(np.repeat(bxy, n, axis=0), np.zeros(n, dtype=np.uint8), M.fr_pack(sc))
    assert _same(fx, sm)  # the two entry points agree on all n outputs
    idx = _sample(300 + n, n)
    assert M.unpack(fx[0][idx], fx[1][idx]) == [M.scalar_mul(base, sc[i]) for i in idx]
    assert bool(fx[1][0]) == (sc[0] == 0)
    # per-pair bases k_i * G with identity entries: all n against the fixed-base path on the products, a sample against the model
    ks = [rng.randrange(1, R) for _ in range(n)]
    kxy, kinf = _multiples(zl, ks)
    kinf = kinf.copy()
    kinf[::7] = 1
    got = zl.g2_scalar_mul_batch(kxy, kinf, M.fr_pack(sc))
    prod = [0 if kinf[i] else ks[i] * sc[i] % R for i in range(n)]
    assert _same(got, _multiples(zl, prod))
    kp = M.unpack(kxy[idx], kinf[idx])
    assert M.unpack(got[0][idx], got[1][idx]) == [M.scalar_mul(p, sc[i]) for p, i in zip(kp, idx)]
    # identity base: every output is G2Point.identity(), written as the reference writes it
    ident = zl.g2_fixed_base_mul_batch(bxy[0], M.fr_pack(sc), base_inf=1)
    assert _same(ident, M.pack([None] * n))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_g1_scalar_mul_batch_on_the_special_scalars(zl, ob, n):
    """The G1 twin of the test above (the two per-pair kernels share one double-and-add), at the edge of the 256-thread workgroup: all n
    outputs against zg_g1_fixed_base_mul_batch, at most 16 of them against the CPU restatement of MSM.scalarMul."""
    rng = random.Random(70 + n)
    sc = [(SPECIAL[i] if i < len(SPECIAL) and n > 1 else rng.randrange(R)) for i in range(n)]
    if n > 20:
        sc[-1] = R - 1
    gm = ob.g1_gen_multiples(n + 12)  # gm[k - 1] = k * G
    base = gm[11]
    scm = M.fr_pack(sc)
    fx = zl.g1_fixed_base_mul_batch(base, scm)
    sm = zl.g1_scalar_mul_batch(np.repeat(base[None, :], n, axis=0), np.zeros(n, dtype=np.uint8), scm)
    assert _same(fx, sm)  # the two entry points agree on all n outputs
    assert bool(fx[1][0]) == (sc[0] == 0)
    idx = _sample(700 + n, n, 16)
    for i in idx:
        w, wi = ob.g1_scalar_mul(base, 0, scm[i])
        assert fx[1][i] == wi and np.array_equal(fx[0][i], w if not wi else np.zeros(8, dtype=np.uint64)), i
    # per-pair bases (i + 1) * G with identity entries on every 7th: all n against the fixed-base path on the products
    kxy, kinf = gm[:n].copy(), np.zeros(n, dtype=np.uint8)
    kinf[::7] = 1
    got = zl.g1_scalar_mul_batch(kxy, kinf, scm)
    prod = [0 if kinf[i] else (i + 1) * sc[i] % R for i in range(n)]
    assert _same(got, zl.g1_fixed_base_mul_batch(gm[0], M.fr_pack(prod)))
    for i in idx:
        w, wi = ob.g1_scalar_mul(kxy[i], int(kinf[i]), scm[i])
        assert got[1][i] == wi and np.array_equal(got[0][i], w if not wi else np.zeros(8, dtype=np.uint64)), i


# ---------------------------------------------------------------- 4. msmG2
def _msm_family(name, n, rng, ks):
    if name == "uniform":
        return [rng.randrange(R) for _ in range(n)]
    if name == "equal":
        return [rng.randrange(1, R)] * n
    if name == "bits":
        return [rng.randrange(2) for _ in range(n)]
    if name == "bytes":
        return [rng.randrange(256) for _ in range(n)]
    if name == "rm1":
        return [R - 1] * n
    if name == "single":
        s = [0] * n
        if n:
            s[rng.randrange(n)] = rng.randrange(1, R)
        return s
    if name == "cancel":  # sum s_i k_i == 0 mod r: the last scalar balances the others
        s = [rng.randrange(R) for _ in range(n)]
        if n:
            s[-1] = -sum(a * b for a, b in zip(s[:-1], ks[:-1])) * pow(ks[-1], -1, R) % R
        return s
    raise AssertionError(name)


@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33, 255, 1024, 4096, 8192])
def test_msm_g2_closed_form(zl, n):
    rng = random.Random(400 + n)
    ks = [rng.randrange(1, R) for _ in range(n)]
    xy, inf = _multiples(zl, ks) if n else (np.zeros((0, 16), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    assert not inf.any()
    pts = M.unpack(xy, inf) if n <= 64 else None
    d_xy = zl.DeviceBuffer.from_host(xy) if n else None
    d_out = zl.DeviceBuffer(17 * 8)
    for fam in ("uniform", "equal", "bits", "bytes", "rm1", "single", "cancel"):
        s = _msm_family(fam, n, rng, ks)
        want = M.scalar_mul(M.G, sum(a * b for a, b in zip(s, ks)) % R)
        got = zl.msm_g2(xy, None, M.fr_pack(s), n=n)
        assert M.unpack(got[0], [got[1]]) == [want], (n, fam)
        if want is None:
            assert list(got[0]) == M.IDENTITY_WORDS and got[1] == 1
        if fam == "cancel" and n:
            assert want is None
        if pts is not None:
            assert M.msm(pts, s) == want  # the reference's literal loop
        # the device-pointer entry point writes the same 17 words
        d_sc = zl.DeviceBuffer.from_host(M.fr_pack(s)) if n else None
        zl.msm_g2_dev(d_xy.ptr if n else 0, 0, d_sc.ptr if n else 0, n, d_out.ptr)
        rec = d_out.to_host()
        assert np.array_equal(rec[:16], got[0]) and int(rec[16]) == got[1], (n, fam)
        if d_sc is not None:
            d_sc.free()
    if d_xy is not None:
        d_xy.free()
    d_out.free()


def test_msm_g2_identity_flags_duplicates_and_opposite_points(zl):
    rng = random.Random(44)
    n = 300
    ks = [rng.randrange(1, R) for _ in range(n)]
    s = [rng.randrange(R) for _ in range(n)]
    xy, inf = _multiples(zl, ks)
    inf = inf.copy()
    inf[::5] = 1  # flagged bases contribute nothing, whatever their coordinates say
    xy2 = xy.copy()
    xy2[5] = 0
    want = M.scalar_mul(M.G, sum(a * b for i, (a, b) in enumerate(zip(s, ks)) if not inf[i]) % R)
    got = zl.msm_g2(xy2, inf, M.fr_pack(s))
    assert M.unpack(got[0], [got[1]]) == [want]
    # duplicate bases (the same point under many scalars, equal digits included)
    dup = np.repeat(xy[3:4], n, axis=0)
    got = zl.msm_g2(dup, None, M.fr_pack(s))
    assert M.unpack(got[0], [got[1]]) == [M.scalar_mul(M.G, ks[3] * sum(s) % R)]
    got = zl.msm_g2(dup, None, M.fr_pack([s[0]] * n))
    assert M.unpack(got[0], [got[1]]) == [M.scalar_mul(M.G, ks[3] * s[0] * n % R)]
    # P, -P, P, -P under one scalar: the identity; under scalars (a, b, a, b): 2 (a - b) P
    p = M.scalar_mul(M.G, ks[0])
    alt, _ = M.pack([p, M.neg(p)] * 8)
    got = zl.msm_g2(alt, None, M.fr_pack([s[1]] * 16))
    assert got[1] == 1 and list(got[0]) == M.IDENTITY_WORDS
    got = zl.msm_g2(alt, None, M.fr_pack([s[1], s[2]] * 8))
    assert M.unpack(got[0], [got[1]]) == [M.scalar_mul(p, 8 * (s[1] - s[2]) % R)]
    # the scalar vector shorter than the bases: msmG2 takes min(len) (dory.zig:694)
    from zolt_amd import api
    got = api.Dory.msmG2((xy, None), M.fr_pack(s[:10]))
    assert M.unpack(got[0], [got[1]]) == [M.scalar_mul(M.G, sum(a * b for a, b in zip(s[:10], ks[:10])) % R)]


# ---------------------------------------------------------------- 5. axpy, both groups
def test_axpy_g2(zl):
    rng = random.Random(5)
    n = 200
    ka = [rng.randrange(1, R) for _ in range(n)]
    kb = [rng.randrange(1, R) for _ in range(n)]
    for case, s in enumerate((0, 1, R - 1, rng.randrange(R))):
        kb2 = list(kb)
        for i in range(0, n, 9):
            kb2[i] = ka[i]  # a[i] == b[i]
        for i in range(1, n, 9):
            kb2[i] = -s * ka[i] % R  # s * a[i] == -b[i]  (b = identity when s == 0)
        a_xy, a_inf = _multiples(zl, ka)
        b_xy, b_inf = _multiples(zl, kb2)
        a_inf, b_inf = a_inf.copy(), b_inf.copy()
        a_inf[2::9] = 1
        b_inf[3::9] = 1
        a_inf[4::9] = 1
        b_inf[4::9] = 1
        sm = M.fr_pack([s])[0]
        got = zl.g2_axpy_batch(a_xy, a_inf, b_xy, b_inf, sm)
        scaled = zl.g2_scalar_mul_batch(a_xy, a_inf, np.repeat(sm.reshape(1, 4), n, axis=0))
        assert _same(got, zl.g2_affine_add_batch(scaled[0], scaled[1], b_xy, b_inf)), case  # all n, second device path
        idx = _sample(50 + case, n)
        pa, pb = M.unpack(a_xy[idx], a_inf[idx]), M.unpack(b_xy[idx], b_inf[idx])
        assert M.unpack(got[0][idx], got[1][idx]) == [M.add(M.scalar_mul(x, s), y) for x, y in zip(pa, pb)], case
        assert got[1][1] == 1 and got[1][4] == 1  # s * a == -b (both the identity when s == 0); identity + identity
        if s not in (0, R - 1):
            assert got[1][0] == 0


def test_axpy_g1_equals_scalar_mul_then_add(zl, ob):
    rng = random.Random(6)
    n = 333
    gm = ob.g1_gen_multiples(2 * n)
    a_xy, b_xy0 = gm[:n].copy(), gm[n:].copy()
    for case, s in enumerate((0, 1, R - 1, rng.randrange(R))):
        sm = M.fr_pack([s])[0]
        rep = np.repeat(sm.reshape(1, 4), n, axis=0)
        b_xy = b_xy0.copy()
        b_inf, a_inf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        b_xy[0::9] = a_xy[0::9]  # a[i] == b[i]
        neg, neg_inf = zl.g1_scalar_mul_batch(a_xy, a_inf, np.repeat(M.fr_pack([-s % R]).reshape(1, 4), n, axis=0))
        b_xy[1::9], b_inf[1::9] = neg[1::9], neg_inf[1::9]  # s * a[i] == -b[i]
        a_inf[2::9] = 1
        b_inf[3::9] = 1
        a_inf[4::9] = 1
        b_inf[4::9] = 1
        got = zl.g1_axpy_batch(a_xy, a_inf, b_xy, b_inf, sm)
        scaled = zl.g1_scalar_mul_batch(a_xy, a_inf, rep)
        want = zl.g1_affine_add_batch(scaled[0], scaled[1], b_xy, b_inf)
        assert _same(got, want), case
        assert got[1][1] == 1 and got[1][4] == 1
        for i in (0, 1, 2, 3, 5, n - 1):  # and the CPU restatement on a few
            sx, si = ob.g1_scalar_mul(a_xy[i], int(a_inf[i]), sm)
            wx, wi = ob.g1_add_affine(sx, si, b_xy[i], int(b_inf[i]))
            assert wi == got[1][i] and (wi or np.array_equal(wx, got[0][i])), (case, i)


# ---------------------------------------------------------------- 6. a whole reduce-and-fold run of the group side
@pytest.mark.parametrize("m", [4, 6])
def test_reduce_and_fold_rounds(zl, ob, m):
    """dory.zig:1503-1635 without the transcript and the pairings: nu = sigma = m, challenges are fixed pseudo-random Fr values. After every
    round v1, v2, s1, s2 and the six group messages equal a straight restatement over the model (G1 side: the CPU restatement of MSM,
    scalarMul and AffinePoint.add)."""
    from zolt_amd import api
    rng = random.Random(600 + m)
    vec_len = 1 << m
    hs = [rng.randrange(1, R) for _ in range(vec_len)]
    g2_vec = api.Dory.generateG2Points(M.fr_pack(hs))
    g2_pts = M.unpack(*g2_vec)
    assert g2_pts[:3] == [M.scalar_mul(M.G, h) for h in hs[:3]]
    g1_all = ob.g1_gen_multiples(3 * vec_len)
    g1_vec = (g1_all[:vec_len].copy(), np.zeros(vec_len, dtype=np.uint8))
    n_rows = vec_len - vec_len // 4  # fewer row commitments than the vector holds: identity padding (:1506-1509)
    v1 = (np.zeros((vec_len, 8), dtype=np.uint64), np.ones(vec_len, dtype=np.uint8))
    v1[0][:n_rows], v1[1][:n_rows] = g1_all[vec_len:vec_len + n_rows], 0
    v_vec = [rng.randrange(R) for _ in range(vec_len - 3)]  # shorter than vec_len: v2 padded with identities (:1513-1519)
    v_vec[1] = 0
    v2 = api.Dory.initV2(g2_vec[0][0], M.fr_pack(v_vec), vec_len)
    s1_i = [rng.randrange(R) for _ in range(vec_len)]
    s2_i = [rng.randrange(R) for _ in range(vec_len - 5)] + [0] * 5  # left_vec zero-padded (:1528-1533)
    s1, s2 = M.fr_pack(s1_i), M.fr_pack(s2_i)
    # the model's state
    w2 = [M.scalar_mul(g2_pts[0], v) for v in v_vec] + [None] * 3
    assert M.unpack(*v2) == w2 and list(v2[1][-3:]) == [1, 1, 1] and v2[1][1] == 1
    w1 = (v1[0].copy(), v1[1].copy())

    def g1_msm(xy, inf, sc):
        return ob.msm_g1(xy, inf, sc)

    def g1_axpy(a, b, s):
        out = (np.zeros_like(b[0]), np.zeros_like(b[1]))
        for i in range(b[0].shape[0]):
            sx, si = ob.g1_scalar_mul(a[0][i], int(a[1][i]), s)
            out[0][i], out[1][i] = ob.g1_add_affine(sx, si, b[0][i], int(b[1][i]))
        return out

    def dev_g1_msm(xy, inf, sc):
        h = zl.Bases.upload(xy, inf, expected_uses=1)
        try:
            return h.msm(sc)
        finally:
            h.free()

    def eq_g1(a, b):
        return a[1] == b[1] and (a[1] or np.array_equal(a[0], b[0]))

    def eq_g1v(a, b):
        return np.array_equal(a[1], b[1]) and np.array_equal(a[0][np.asarray(a[1]) == 0], b[0][np.asarray(b[1]) == 0])

    cur = vec_len
    for rnd in range(m):
        n2 = cur // 2
        beta, alpha = rng.randrange(1, R), rng.randrange(1, R)
        beta_inv, alpha_inv = pow(beta, -1, R), pow(alpha, -1, R)
        fb, fbi, fa, fai = (M.fr_pack([x])[0] for x in (beta, beta_inv, alpha, alpha_inv))
        # first reduce message (:1553-1554)
        assert eq_g1(dev_g1_msm(g1_vec[0][:cur], g1_vec[1][:cur], s2[:cur]), g1_msm(g1_vec[0][:cur], g1_vec[1][:cur], s2[:cur])), rnd
        e2_beta = api.Dory.msmG2((g2_vec[0][:cur], g2_vec[1][:cur]), s1[:cur])
        assert M.unpack(e2_beta[0], [e2_beta[1]]) == [M.msm(g2_pts[:cur], s1_i[:cur])], rnd
        # apply the first challenge (:1578-1584)
        v1, v2 = api.Dory.applyFirstChallenge((v1[0][:cur], v1[1][:cur]), (v2[0][:cur], v2[1][:cur]), g1_vec, g2_vec, fb, fbi)
        w1 = g1_axpy((g1_vec[0][:cur], g1_vec[1][:cur]), (w1[0][:cur], w1[1][:cur]), fb)
        w2 = [M.add(w2[i], M.scalar_mul(g2_pts[i], beta_inv)) for i in range(cur)]
        assert eq_g1v(v1, w1) and M.unpack(*v2) == w2, rnd
        # second reduce message (:1589-1592)
        assert eq_g1(dev_g1_msm(v1[0][:n2], v1[1][:n2], s2[n2:cur]), g1_msm(w1[0][:n2], w1[1][:n2], s2[n2:cur])), rnd
        assert eq_g1(dev_g1_msm(v1[0][n2:cur], v1[1][n2:cur], s2[:n2]), g1_msm(w1[0][n2:cur], w1[1][n2:cur], s2[:n2])), rnd
        e2_plus = api.Dory.msmG2((v2[0][n2:cur], v2[1][n2:cur]), s1[:n2])
        e2_minus = api.Dory.msmG2((v2[0][:n2], v2[1][:n2]), s1[n2:cur])
        assert M.unpack(e2_plus[0], [e2_plus[1]]) == [M.msm(w2[n2:cur], s1_i[:n2])], rnd
        assert M.unpack(e2_minus[0], [e2_minus[1]]) == [M.msm(w2[:n2], s1_i[n2:cur])], rnd
        # fold (:1615-1632)
        v1, v2, s1, s2 = api.Dory.foldVectors(v1, v2, s1[:cur], s2[:cur], fa, fai)
        w1 = g1_axpy((w1[0][:n2], w1[1][:n2]), (w1[0][n2:cur], w1[1][n2:cur]), fa)
        w2 = [M.add(M.scalar_mul(w2[i], alpha_inv), w2[i + n2]) for i in range(n2)]
        s1_i = [(alpha * s1_i[i] + s1_i[i + n2]) % R for i in range(n2)]
        s2_i = [(alpha_inv * s2_i[i] + s2_i[i + n2]) % R for i in range(n2)]
        assert eq_g1v(v1, w1) and M.unpack(*v2) == w2, rnd
        assert M.fr_unpack(s1) == s1_i and M.fr_unpack(s2) == s2_i, rnd
        cur = n2
    assert cur == 1 and len(w2) == 1


# ---------------------------------------------------------------- 7. the C++ mirror
def test_cpp_g2_mirror(tmp_path):
    exe = str(tmp_path / "test_g2_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_g2_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout
