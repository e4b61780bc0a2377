"""Pairings on the device (zg_miller_loop_batch, zg_final_exponentiation_batch, zg_pairing_batch, zg_multi_pairing[_dev], the
ZG_OP_FP12_* hooks of zg_field_op and api.Dory's multiPairG1G2 / multiPairBatch / commit) against the big-integer model of
tests/pairing_model.py (pinned by tests/test_pairing_model.py) and against second device paths. Bit-exact: no tolerances.

Operands are k_i * G1 and k_i * G2 built on the device by the fixed-base entry points. Where outputs are sampled against the model the
sample is at most 16 indices, always with the first and the last; every output is still covered by an all-n equality between two device
paths. The model's Miller values are computed once per pair and shared by the tests."""
import random

import numpy as np
import pytest

from tests import g2_model as G2
from tests import pairing_model as M

pytestmark = pytest.mark.gpu
R, P = M.R, M.P
N_POOL = 130
ONE_WORDS = M.gt_pack([M.ONE])[0]


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


class Pool:
    """N_POOL pairs (k1_i * G1, k2_i * G2) from the device's fixed-base paths, their model points, and the model's Miller values (lazy)"""

    def __init__(self, zl):
        rng = random.Random(0xD0C1)
        self.k1 = [rng.randrange(1, R) for _ in range(N_POOL)]
        self.k2 = [rng.randrange(1, R) for _ in range(N_POOL)]
        self.g1, i1 = zl.g1_fixed_base_mul_batch(M.g1_pack([M.G1_GEN])[0][0], G2.fr_pack(self.k1))
        self.g2, i2 = zl.g2_fixed_base_mul_batch(G2.pack([G2.G])[0][0], G2.fr_pack(self.k2))
        assert not i1.any() and not i2.any()
        self.p = M.g1_unpack(self.g1, i1)
        self.q = G2.unpack(self.g2, i2)
        assert self.p[0] == M.g1_mul(M.G1_GEN, self.k1[0]) and self.q[0] == G2.scalar_mul(G2.G, self.k2[0])
        self._miller = {}

    def miller(self, i):
        if i not in self._miller:
            self._miller[i] = M.miller_loop(self.p[i], self.q[i])
        return self._miller[i]


@pytest.fixture(scope="module")
def pool(zl):
    return Pool(zl)


@pytest.fixture(scope="module")
def dev65(zl, pool):
    """the device's Miller values and pairings of the first 65 pairs, no identities: what the smaller batches are compared with"""
    return zl.miller_loop_batch(pool.g1[:65], None, pool.g2[:65], None), zl.pairing_batch(pool.g1[:65], None, pool.g2[:65], None)


def _sample(seed, n, k=16):
    if n <= k:
        return list(range(n))
    rng = random.Random(seed)
    return sorted({0, n - 1} | set(rng.sample(range(1, n - 1), k - 2)))


def _prod(elems):
    acc = M.ONE
    for e in elems:
        acc = M.mul(acc, e)
    return acc


def _dev_product(zl, gts):
    """the product of (m, 48) GT elements through ZG_OP_FP12_MUL: a tree of elementwise products -> (48,)"""
    cur = np.ascontiguousarray(gts, dtype=np.uint64).reshape(-1, 48)
    if cur.shape[0] == 0:
        return ONE_WORDS.copy()
    while cur.shape[0] > 1:
        h = cur.shape[0] // 2
        nxt = zl.field_op(zl.FP, zl.OP_FP12_MUL, cur[:h].reshape(-1, 4), cur[h:2 * h].reshape(-1, 4)).reshape(-1, 48)
        cur = np.concatenate([nxt, cur[2 * h:]]) if cur.shape[0] & 1 else nxt
    return cur[0]


# ---------------------------------------------------------------- 1. the tower
def _tower_inputs():
    rng = random.Random(12)
    edge = [M.ZERO, M.ONE, tuple([(P - 1, P - 1)] * 6)]
    for k in range(6):
        for c in ((1, 0), (0, 1), (rng.randrange(P), rng.randrange(P))):
            f = [(0, 0)] * 6
            f[k] = c
            edge.append(tuple(f))
    rand = lambda: tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))  # noqa: E731
    a = edge + [rand() for _ in range(200)]
    b = [rand() for _ in edge] + edge + [rand() for _ in range(200 - len(edge))]
    assert len(a) == len(b)
    return a, b


def test_fp12_tower_ops(zl):
    a, b = _tower_inputs()
    pa, pb = M.gt_pack(a).reshape(-1, 4), M.gt_pack(b).reshape(-1, 4)

    def run(op, y=None):
        return M.gt_unpack(zl.field_op(zl.FP, op, pa, y))

    assert run(zl.OP_FP12_MUL, pb) == [M.mul(u, v) for u, v in zip(a, b)]
    assert run(zl.OP_FP12_SQR) == [M.sqr(u) for u in a]
    inv = run(zl.OP_FP12_INV)
    assert inv == [M.inv(u) for u in a] and inv[0] == M.ZERO and inv[1] == M.ONE
    assert all(M.mul(u, v) == M.ONE for u, v in zip(a[1:], inv[1:]))
    assert run(zl.OP_FP12_CONJ) == [M.conj(u) for u in a]
    for n, op in ((1, zl.OP_FP12_FROB1), (2, zl.OP_FP12_FROB2), (3, zl.OP_FP12_FROB3)):
        assert run(op) == [M.frobenius(u, n) for u in a], n
    # an output may alias nothing here, but the operands may be equal: a * a through MUL is SQR
    assert np.array_equal(zl.field_op(zl.FP, zl.OP_FP12_MUL, pa, pa), zl.field_op(zl.FP, zl.OP_FP12_SQR, pa))


def test_fp12_exp_by_x_on_8_elements(zl):
    a, _ = _tower_inputs()
    pick = [a[0], a[1], a[2], a[5]] + a[-4:]
    got = M.gt_unpack(zl.field_op(zl.FP, zl.OP_FP12_EXP_X, M.gt_pack(pick).reshape(-1, 4)))
    assert got == [M.exp_by_x(u) for u in pick] and got[0] == M.ZERO and got[1] == M.ONE


def test_fp12_hooks_refuse_other_shapes_and_fields(zl):
    pa = M.gt_pack([M.ONE, M.ONE]).reshape(-1, 4)
    for op in range(zl.OP_FP12_MUL, zl.OP_FP12_EXP_X + 1):
        with pytest.raises(zl.ZgError):  # 13 Fp elements are not a vector of Fp12 elements
            zl.field_op(zl.FP, op, pa[:13], pa[:13])
        with pytest.raises(zl.ZgError):
            zl.field_op(zl.FR, op, pa, pa)
    with pytest.raises(zl.ZgError):  # the product needs its second operand
        zl.field_op(zl.FP, zl.OP_FP12_MUL, pa, None)
    with pytest.raises(zl.ZgError):  # one past the last code
        zl.field_op(zl.FP, zl.OP_FP12_EXP_X + 1, pa, pa)


# ---------------------------------------------------------------- 2. the Miller loop
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_miller_loop_batch(zl, pool, dev65, n):
    """The header promises millerLoopArkworks' value, so the UNREDUCED equality with the model is this entry point's contract (the kernel
    follows the reference's step formulas and digits); the equality after the model's final exponentiation is what every pairing built
    on it depends on, and is asserted on its own."""
    got = zl.miller_loop_batch(pool.g1[:n], None, pool.g2[:n], None)
    assert got.shape == (n, 48) and np.array_equal(got, dev65[0][:n])  # all n: the same lanes of a longer launch
    dev = M.gt_unpack(got)
    for i in _sample(200 + n, n):
        assert M.final_exponentiation(dev[i]) == M.pairing(pool.p[i], pool.q[i]), i
        assert dev[i] == pool.miller(i), i


# ---------------------------------------------------------------- 3. the final exponentiation
def test_final_exponentiation_batch(zl, pool, dev65):
    ms = [pool.miller(i) for i in range(65)]
    got = zl.final_exponentiation_batch(M.gt_pack(ms + [M.ZERO, M.ONE]))
    assert np.array_equal(got[:65], dev65[1])  # all 65: the device's own pairings of the same pairs
    assert np.array_equal(got[65], ONE_WORDS) and np.array_equal(got[66], ONE_WORDS)  # zero -> one, one -> one
    dev = M.gt_unpack(got)
    for i in _sample(31, 65):
        assert dev[i] == M.final_exponentiation(ms[i]), i
    one = zl.final_exponentiation_batch(M.gt_pack(ms[:1]))  # n = 1
    assert one.shape == (1, 48) and np.array_equal(one[0], got[0])
    f = tuple((3 * k + 1, 5 * k + 2) for k in range(6))  # not a Miller value: any non-zero element goes through the same power
    assert M.gt_unpack(zl.final_exponentiation_batch(M.gt_pack([f]))) == [M.final_exponentiation(f)]
    assert zl.final_exponentiation_batch(np.zeros((0, 48), dtype=np.uint64)).shape == (0, 48)


# ---------------------------------------------------------------- 4. pairings
def test_pairing_batch(zl, pool, dev65):
    n = 65
    mil, pair = dev65
    assert np.array_equal(pair, zl.final_exponentiation_batch(mil))  # all n
    dev = M.gt_unpack(pair)
    for i in _sample(41, n):
        assert dev[i] == M.final_exponentiation(pool.miller(i)), i
    # an identity on either side gives one: G1 at 0, G2 at 63, both at 64 = n - 1; only the flags count, the coordinates under them do not
    i1, i2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    i1[[0, 64]] = 1
    i2[[63, 64]] = 1
    g1, g2 = pool.g1[:n].copy(), pool.g2[:n].copy()
    g1[0], g2[63], g2[64] = 0, 0xdeadbeef, 0
    for fn, clean in ((zl.pairing_batch, pair), (zl.miller_loop_batch, mil)):
        got = fn(g1, i1, g2, i2)
        ones = np.array([0, 63, 64])
        assert np.array_equal(got[ones], np.tile(ONE_WORDS, (3, 1)))
        keep = np.setdiff1d(np.arange(n), ones)
        assert np.array_equal(got[keep], clean[keep])
    assert zl.pairing_batch(np.zeros((0, 8), dtype=np.uint64), None, np.zeros((0, 16), dtype=np.uint64), None).shape == (0, 48)


def test_generator_pairing_has_the_recorded_bytes(zl):
    import json
    import os
    from zolt_amd import api
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairing_generator_jolt.json")))
    got = zl.pairing_batch(api.generator().reshape(1, 8), None, api.g2_generator().reshape(1, 16), None)
    assert api.gt_to_bytes(got[0])[:16].hex() == fx["pairing_to_bytes_first_16_hex"]
    assert api.gt_to_bytes(got[0]) == M.to_bytes(M.pairing(M.G1_GEN, G2.G))


# ---------------------------------------------------------------- 5. multi-pairings
def _multi_dev(zl, g1, i1, g2, i2, seg, stream):
    n, k = g1.shape[0], len(seg) - 1
    bufs = [zl.DeviceBuffer.from_host(x) for x in (g1, i1, g2, i2, np.asarray(seg, dtype=np.uint64))]
    d_out = zl.DeviceBuffer(max(k, 1) * 48 * 8)
    zl.multi_pairing_dev(bufs[0].ptr if n else 0, bufs[1].ptr if n else 0, bufs[2].ptr if n else 0, bufs[3].ptr if n else 0, n, bufs[4].ptr, k, d_out.ptr,
                         stream=stream)
    out = d_out.to_host()[:k * 48].reshape(k, 48)
    for b in bufs + [d_out]:
        b.free()
    return out


def _check_multi(zl, pool, g1, i1, g2, i2, seg, millers):
    """every output against the model's product of Miller values and one final exponentiation, against the device's own product of
    zg_pairing_batch outputs, and against the device-pointer entry point on a stream of its own"""
    import torch
    k = len(seg) - 1
    got = zl.multi_pairing(g1, i1, g2, i2, seg)
    assert got.shape == (k, 48)
    pairs = zl.pairing_batch(g1, i1, g2, i2)
    for j in range(k):
        lo, hi = seg[j], seg[j + 1]
        assert M.gt_unpack(got[j])[0] == M.final_exponentiation(_prod(millers[lo:hi])), j
        assert np.array_equal(got[j], _dev_product(zl, pairs[lo:hi])), j
    work = torch.cuda.Stream()
    assert np.array_equal(_multi_dev(zl, g1, i1, g2, i2, seg, work.cuda_stream), got)
    return got


def test_multi_pairing_shape_a_segments_0_1_64_65(zl, pool):
    """n = 130, k = 4: an empty segment (-> one), a single pair, a full wave, a wave and one more — a tree that is no power of two"""
    n, seg = 130, [0, 0, 1, 65, 130]
    none = np.zeros(n, dtype=np.uint8)
    got = _check_multi(zl, pool, pool.g1, none, pool.g2, none, seg, [pool.miller(i) for i in range(n)])
    assert np.array_equal(got[0], ONE_WORDS)
    assert np.array_equal(got[1], zl.pairing_batch(pool.g1[:1], None, pool.g2[:1], None)[0])
    assert np.array_equal(zl.multi_pairing(pool.g1, None, pool.g2, None, seg), got)  # NULL flags = no identities
    # closed form: prod e(k1 G1, k2 G2) = e(G1, G2)^(sum k1 k2)
    e = M.pairing(M.G1_GEN, G2.G)
    assert M.gt_unpack(got[3])[0] == M.power(e, sum(a * b for a, b in zip(pool.k1[65:], pool.k2[65:])) % R)


def test_multi_pairing_shape_b_one_product_of_128(zl, pool):
    """n = 128, k = 1, with a (P, Q), (-P, Q) pair whose contributions cancel and an identity that is skipped; a permutation of the
    pairs gives the same bits"""
    n = 128
    g1, g2 = pool.g1[:n].copy(), pool.g2[:n].copy()
    neg_p0 = M.g1_neg(pool.p[0])
    g1[1], g2[1] = M.g1_pack([neg_p0])[0][0], pool.g2[0]
    i1, i2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    i2[77] = 1
    millers = [pool.miller(i) for i in range(n)]
    millers[1] = M.miller_loop(neg_p0, pool.q[0])
    millers[77] = M.ONE
    got = _check_multi(zl, pool, g1, i1, g2, i2, [0, n], millers)
    rest = [i for i in range(2, n) if i != 77]
    assert np.array_equal(got, zl.multi_pairing(g1[rest], None, g2[rest], None))  # the cancelling pair and the identity contribute one
    perm = list(range(n))
    random.Random(5).shuffle(perm)
    assert np.array_equal(zl.multi_pairing(g1[perm], i1[perm], g2[perm], i2[perm]), got)
    assert np.array_equal(zl.multi_pairing(g1[:2], None, g2[:2], None)[0], ONE_WORDS)


def test_multi_pairing_of_nothing(zl, pool):
    e1, e2 = np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 16), dtype=np.uint64)
    assert zl.multi_pairing(pool.g1[:4], None, pool.g2[:4], None, [0]).shape == (0, 48)  # k = 0
    assert zl.multi_pairing(e1, None, e2, None, [0]).shape == (0, 48)  # k = 0 and n = 0
    got = zl.multi_pairing(e1, None, e2, None, [0, 0, 0])  # n = 0: every product is empty
    assert np.array_equal(got, np.tile(ONE_WORDS, (2, 1)))
    none = np.zeros(0, dtype=np.uint8)
    assert np.array_equal(_multi_dev(zl, e1, none, e2, none, [0, 0, 0], 0), got)
    assert _multi_dev(zl, e1, none, e2, none, [0], 0).shape == (0, 48)
    for bad in ([0, 5], [3, 2, 4], [0, 2, 1]):  # past n, descending
        with pytest.raises(zl.ZgError):
            zl.multi_pairing(pool.g1[:4], None, pool.g2[:4], None, bad)


# ---------------------------------------------------------------- 6. Dory's shapes
def test_dory_multi_pair_batch_is_six_multi_pairs(zl, pool):
    from zolt_amd import api
    inf = np.zeros(8, dtype=np.uint8)
    vecs = []
    for j in range(6):
        s = slice(8 * j, 8 * j + 8)
        i2 = inf.copy()
        i2[j] = j & 1  # an identity in every other vector
        vecs.append(((pool.g1[s], None if j == 2 else inf), (pool.g2[s], i2)))
    got = api.Dory.multiPairBatch(vecs)
    assert got.shape == (6, 48)
    for j, (a, b) in enumerate(vecs):
        assert np.array_equal(got[j], api.Dory.multiPairG1G2(a, b)), j
    j = 3
    want = _prod([pool.miller(8 * j + t) for t in range(8) if t != j])
    assert M.gt_unpack(got[j])[0] == M.final_exponentiation(want)
    # min(len): a longer G2 vector is cut
    assert np.array_equal(api.Dory.multiPairG1G2((pool.g1[:8], inf), (pool.g2[:12], None)), got[0])
    assert api.Dory.multiPairBatch([]).shape == (0, 48)


def test_dory_commit_4_by_8(zl, pool):
    from zolt_amd import api
    rng = random.Random(66)
    rows, cols = 4, 8
    ev = [rng.randrange(R) for _ in range(rows * cols)]
    bases = zl.Bases.upload(pool.g1[:cols], np.zeros(cols, dtype=np.uint8))
    g2_vec = (pool.g2[:rows], np.zeros(rows, dtype=np.uint8))
    got = api.Dory.commit(bases, g2_vec, G2.fr_pack(ev), cols)
    rc = api.Dory.computeRowCommitments(bases, G2.fr_pack(ev), cols)
    bases.free()
    dev_rows = M.g1_unpack(*rc)
    assert M.gt_unpack(got)[0] == M.multi_pairing(dev_rows, pool.q[:rows])  # the model over the device's row commitments
    model_rows = []
    for r in range(rows):
        acc = None
        for c in range(cols):
            acc = M.g1_add(acc, M.g1_mul(pool.p[c], ev[r * cols + c]))
        model_rows.append(acc)
    assert model_rows == dev_rows  # and with the rows from the model too
    assert M.gt_unpack(got)[0] == M.multi_pairing(model_rows, pool.q[:rows])


def test_bilinearity_through_the_fold_steps(zl, pool):
    """e(alpha P, alpha^-1 Q) = e(P, Q) on 4 pairs, the scalings done by the axpy entry points of the fold steps with identity addends.
    (That multiPair(v1', v2') after foldVectors equals the D-terms is protocol algebra — the verifier's business, not asserted.)"""
    rng = random.Random(77)
    alpha = rng.randrange(2, R)
    n = 4
    ident = np.ones(n, dtype=np.uint8)
    a1 = zl.g1_axpy_batch(pool.g1[:n], None, np.zeros((n, 8), dtype=np.uint64), ident, G2.fr_pack([alpha])[0])
    a2 = zl.g2_axpy_batch(pool.g2[:n], None, np.tile(np.array(G2.IDENTITY_WORDS, dtype=np.uint64), (n, 1)), ident, G2.fr_pack([pow(alpha, -1, R)])[0])
    assert not a1[1].any() and not a2[1].any()
    assert np.array_equal(zl.pairing_batch(a1[0], a1[1], a2[0], a2[1]), zl.pairing_batch(pool.g1[:n], None, pool.g2[:n], None))
    assert not np.array_equal(a1[0], pool.g1[:n])
