"""The wave pairing engine (include/zolt_gpu.h, "Pairings (engine)": a wavefront per Miller loop and per final exponentiation) through
every consumer, against the lane engine in the same process — every value is a canonical field element, so the two must agree word for
word — and against the big-integer models of tests/pairing_model.py and tests/dory_open_model.py.

The engine is process-wide and the suite shares one process: it is only ever set inside `with lib.pairing_engine(...)`, which restores
what was set before, and no test asserts what the default is (the suite also runs under ZG_PAIRING_ENGINE=wave)."""
import random
import threading

import numpy as np
import pytest

from tests import dory_open_model as D
from tests import g2_model as G2
from tests import pairing_model as M
from tests import test_gpu_pairing as TP

pytestmark = pytest.mark.gpu
R, P = M.R, M.P
ONE_WORDS = TP.ONE_WORDS


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def pool(zl):
    return TP.Pool(zl)


def lane(zl):
    return zl.pairing_engine(zl.PAIRING_ENGINE_LANE)


def wave(zl):
    return zl.pairing_engine(zl.PAIRING_ENGINE_WAVE)


@pytest.fixture(scope="module")
def lane65(zl, pool):
    """the lane engine's Miller values and pairings of the first 65 pairs"""
    with lane(zl):
        return zl.miller_loop_batch(pool.g1[:65], None, pool.g2[:65], None), zl.pairing_batch(pool.g1[:65], None, pool.g2[:65], None)


# ---------------------------------------------------------------- 1. the tower hooks
@pytest.fixture(scope="module")
def tower():
    a, b = TP._tower_inputs()
    return a, b, M.gt_pack(a).reshape(-1, 4), M.gt_pack(b).reshape(-1, 4)


def test_wave_tower_ops_equal_the_model_and_the_lane_tower(zl, tower):
    a, b, pa, pb = tower

    def both(wop, lop, y=None):
        got = zl.field_op(zl.FP, wop, pa, y)
        assert np.array_equal(got, zl.field_op(zl.FP, lop, pa, y)), wop
        return M.gt_unpack(got)

    assert both(zl.OP_FP12W_MUL, zl.OP_FP12_MUL, pb) == [M.mul(u, v) for u, v in zip(a, b)]
    assert both(zl.OP_FP12W_SQR, zl.OP_FP12_SQR) == [M.sqr(u) for u in a]
    inv = both(zl.OP_FP12W_INV, zl.OP_FP12_INV)
    assert inv == [M.inv(u) for u in a] and inv[0] == M.ZERO and inv[1] == M.ONE
    assert both(zl.OP_FP12W_CONJ, zl.OP_FP12_CONJ) == [M.conj(u) for u in a]
    for n, wop, lop in ((1, zl.OP_FP12W_FROB1, zl.OP_FP12_FROB1), (2, zl.OP_FP12W_FROB2, zl.OP_FP12_FROB2), (3, zl.OP_FP12W_FROB3, zl.OP_FP12_FROB3)):
        assert both(wop, lop) == [M.frobenius(u, n) for u in a], n
    assert np.array_equal(zl.field_op(zl.FP, zl.OP_FP12W_MUL, pa, pa), zl.field_op(zl.FP, zl.OP_FP12W_SQR, pa))


@pytest.mark.parametrize("count", [1, 2, 3, 5, 65])
def test_wave_tower_element_counts(zl, tower, count):
    """a launch of one wave, of a few, and of more than a workgroup of any size could hold, on the random tail of the inputs"""
    a, b, pa, pb = tower
    lo = len(a) - count
    sa, sb = pa[12 * lo:], pb[12 * lo:]
    assert M.gt_unpack(zl.field_op(zl.FP, zl.OP_FP12W_MUL, sa, sb)) == [M.mul(u, v) for u, v in zip(a[lo:], b[lo:])]
    assert np.array_equal(zl.field_op(zl.FP, zl.OP_FP12W_INV, sa), zl.field_op(zl.FP, zl.OP_FP12_INV, sa))


def test_wave_exp_by_x_on_8_elements(zl, tower):
    a = tower[0]
    pick = [a[0], a[1], a[2], a[5]] + a[-4:]
    pp = M.gt_pack(pick).reshape(-1, 4)
    got = zl.field_op(zl.FP, zl.OP_FP12W_EXP_X, pp)
    assert np.array_equal(got, zl.field_op(zl.FP, zl.OP_FP12_EXP_X, pp))
    got = M.gt_unpack(got)
    assert got == [M.exp_by_x(u) for u in pick] and got[0] == M.ZERO and got[1] == M.ONE


def test_wave_mul_by_034(zl, tower):
    a = tower[0]
    rng = random.Random(34)
    r2 = lambda: (rng.randrange(P), rng.randrange(P))  # noqa: E731
    sparse = [(r2(), r2(), r2()) for _ in a]
    # sparse coefficients that are zero, one at a time and all three
    sparse[3], sparse[4], sparse[5], sparse[6] = ((0, 0), r2(), r2()), (r2(), (0, 0), r2()), (r2(), r2(), (0, 0)), ((0, 0), (0, 0), (0, 0))
    z = (0, 0)
    b = [(c0, z, c3, z, c4, z) for c0, c3, c4 in sparse]  # memory order is w^0, w^2, w^4, ...: the first three Fp2 of the 12 words
    got = M.gt_unpack(zl.field_op(zl.FP, zl.OP_FP12W_MUL_034, tower[2], M.gt_pack(b).reshape(-1, 4)))
    assert got == [M.mul_by_034(u, *s) for u, s in zip(a, sparse)]


def test_wave_hooks_refuse_other_shapes_and_fields(zl):
    pa = M.gt_pack([M.ONE, M.ONE]).reshape(-1, 4)
    for op in range(zl.OP_FP12W_MUL, zl.OP_FP12W_MUL_034 + 1):
        with pytest.raises(zl.ZgError):  # 13 Fp elements are not a vector of Fp12 elements
            zl.field_op(zl.FP, op, pa[:13], pa[:13])
        with pytest.raises(zl.ZgError):
            zl.field_op(zl.FR, op, pa, pa)
    for op in (zl.OP_FP12W_MUL, zl.OP_FP12W_MUL_034):
        with pytest.raises(zl.ZgError):  # a product needs its second operand
            zl.field_op(zl.FP, op, pa, None)
    for op in (zl.OP_FP12W_MUL - 1, zl.OP_FP12W_MUL_034 + 1):  # 37..39 stay invalid; one past the last code
        with pytest.raises(zl.ZgError):
            zl.field_op(zl.FP, op, pa, pa)


# ---------------------------------------------------------------- 2. the Miller loop
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_wave_miller_loop(zl, pool, lane65, n):
    with wave(zl):
        got = zl.miller_loop_batch(pool.g1[:n], None, pool.g2[:n], None)
    assert got.shape == (n, 48) and np.array_equal(got, lane65[0][:n])  # all n words against the lane engine
    dev = M.gt_unpack(got)
    for i in TP._sample(900 + n, n, 4):  # the UNREDUCED value is millerLoopArkworks'
        assert dev[i] == pool.miller(i), i


def test_wave_miller_identity_flags(zl, pool, lane65):
    """G1 at 0, G2 at 63, both at 64 of 65; only the flags count, the coordinates under them are garbage"""
    n = 65
    i1, i2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    i1[[0, 64]] = 1
    i2[[63, 64]] = 1
    g1, g2 = pool.g1[:n].copy(), pool.g2[:n].copy()
    g1[0], g2[63], g2[64], g1[64] = 0xdeadbeef, 0xdeadbeef, 0, 0xfeedface
    ones = np.array([0, 63, 64])
    keep = np.setdiff1d(np.arange(n), ones)
    for fn, clean in ((zl.miller_loop_batch, lane65[0]), (zl.pairing_batch, lane65[1])):
        with wave(zl):
            got = fn(g1, i1, g2, i2)
        assert np.array_equal(got[ones], np.tile(ONE_WORDS, (3, 1)))
        assert np.array_equal(got[keep], clean[keep])


# ---------------------------------------------------------------- 3. the final exponentiation
def test_wave_final_exponentiation(zl, pool, lane65):
    ins = np.concatenate([lane65[0], M.gt_pack([M.ZERO, M.ONE])])  # 65 Miller values, zero, one
    with wave(zl):
        got = zl.final_exponentiation_batch(ins)
        one = zl.final_exponentiation_batch(ins[:1])
        none = zl.final_exponentiation_batch(np.zeros((0, 48), dtype=np.uint64))
        f = tuple((3 * k + 1, 5 * k + 2) for k in range(6))  # not a Miller value
        other = zl.final_exponentiation_batch(M.gt_pack([f]))
    with lane(zl):
        assert np.array_equal(got, zl.final_exponentiation_batch(ins))
    assert np.array_equal(got[:65], lane65[1])
    assert np.array_equal(got[65], ONE_WORDS) and np.array_equal(got[66], ONE_WORDS)
    assert one.shape == (1, 48) and np.array_equal(one[0], got[0]) and none.shape == (0, 48)
    assert M.gt_unpack(other) == [M.final_exponentiation(f)]
    assert M.gt_unpack(got[:1])[0] == M.final_exponentiation(pool.miller(0))


# ---------------------------------------------------------------- 4. the generator pairing
def test_wave_generator_pairing_has_the_recorded_bytes(zl):
    import json
    import os
    from zolt_amd import api
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairing_generator_jolt.json")))
    with wave(zl):
        got = zl.pairing_batch(api.generator().reshape(1, 8), None, api.g2_generator().reshape(1, 16), None)
    assert api.gt_to_bytes(got[0])[:16].hex() == fx["pairing_to_bytes_first_16_hex"]


# ---------------------------------------------------------------- 5. multi-pairings
def test_wave_multi_pairing(zl, pool):
    import torch
    n, seg = 130, [0, 0, 1, 65, 130]
    none = np.zeros(n, dtype=np.uint8)
    e1, e2 = np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 16), dtype=np.uint64)
    work = torch.cuda.Stream()
    with wave(zl):
        got = zl.multi_pairing(pool.g1, none, pool.g2, none, seg)
        got128 = zl.multi_pairing(pool.g1[:128], None, pool.g2[:128], None)
        empty = zl.multi_pairing(e1, None, e2, None, [0, 0, 0])  # k > 0 and n = 0
        dev = TP._multi_dev(zl, pool.g1, none, pool.g2, none, seg, work.cuda_stream)
    with lane(zl):
        assert np.array_equal(got, zl.multi_pairing(pool.g1, none, pool.g2, none, seg))
        assert np.array_equal(got128, zl.multi_pairing(pool.g1[:128], None, pool.g2[:128], None))
    assert np.array_equal(dev, got)
    assert np.array_equal(empty, np.tile(ONE_WORDS, (2, 1))) and np.array_equal(got[0], ONE_WORDS)
    assert M.gt_unpack(got[1])[0] == M.final_exponentiation(pool.miller(0))  # the model product on the small ones
    e = M.pairing(M.G1_GEN, G2.G)  # closed form for the long ones: prod e(k1 G1, k2 G2) = e(G1, G2)^(sum k1 k2)
    assert M.gt_unpack(got[3])[0] == M.power(e, sum(a * b for a, b in zip(pool.k1[65:], pool.k2[65:])) % R)
    assert M.gt_unpack(got128)[0] == M.power(e, sum(a * b for a, b in zip(pool.k1[:128], pool.k2[:128])) % R)


# ---------------------------------------------------------------- 6. Dory's consumers
def _open(zl, inp, after_begin=None):
    """one opening with the Blake2b transcript -> the proof's bytes; `after_begin` runs once the session exists"""
    from zolt_amd import api
    tr = api.Blake2bTranscript(b"Jolt")
    ses = zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]),
                                   G2.fr_pack(inp["left_vec"]), inp["nu"], inp["sigma"])
    if after_begin:
        after_begin()
    vmv = ses.vmv
    tr.appendGT(vmv[0:48])
    tr.appendGT(vmv[48:96])
    tr.appendG1Compressed((vmv[96:104], int(vmv[104])))
    firsts, seconds = [], []
    for _ in range(inp["sigma"]):
        m = ses.first_message()
        firsts.append(m)
        for k in range(4):
            tr.appendGT(m[48 * k:48 * k + 48])
        tr.appendG1Compressed((m[192:200], int(m[200])))
        tr.appendG2Compressed((m[201:217], int(m[217])))
        beta = tr.challengeScalar()
        m = ses.second_message(beta, api.Dory.inverseOrOne(beta))
        seconds.append(m)
        tr.appendGT(m[0:48])
        tr.appendGT(m[48:96])
        tr.appendG1Compressed((m[96:104], int(m[104])))
        tr.appendG1Compressed((m[105:113], int(m[113])))
        tr.appendG2Compressed((m[114:130], int(m[130])))
        tr.appendG2Compressed((m[131:147], int(m[147])))
        alpha = tr.challengeScalar()
        ses.fold(alpha, api.Dory.inverseOrOne(alpha))
    gamma = tr.challengeScalar()
    final = ses.final(gamma, api.Dory.inverseOrOne(gamma))
    ses.close()
    return api.DoryProof(vmv, firsts, seconds, final, inp["nu"], inp["sigma"]).toBytes()


@pytest.mark.parametrize("nu,sigma", [(2, 2), (2, 3)])  # (the session requires nu <= sigma)
def test_wave_opening_session(zl, nu, sigma):
    from tests.test_gpu_dory_open import CASES
    inp = D.make_inputs(nu, sigma, seed=1000 + 16 * nu + sigma, **CASES[(nu, sigma)])
    want = D.run_model(inp, D.Transcript(b"Jolt"))["proof"]
    with lane(zl):
        assert _open(zl, inp) == want
    with wave(zl):
        assert _open(zl, inp) == want
        # a session begun under WAVE keeps WAVE when the engine goes back to LANE mid-session; the bytes say nothing about which engine
        # ran, so the test is that the proof is still right with the setting changed under it
        assert _open(zl, inp, after_begin=lambda: zl.pairing_engine_set(zl.PAIRING_ENGINE_LANE)) == want
        assert zl.pairing_engine_get() == zl.PAIRING_ENGINE_LANE


def test_wave_commit_batch_4_by_8(zl, pool):
    from zolt_amd import api
    rng = random.Random(66)
    rows, cols = 4, 8
    key = zl.DoryKey.create((pool.g1[:cols], None), (pool.g2[:rows], None))
    ev = [rng.randrange(R) for _ in range(rows * cols)]
    polys = [("fr", G2.fr_pack(ev)), ("u64", np.arange(1, rows * cols + 1, dtype=np.uint64))]
    with lane(zl):
        a = api.Dory.batchCommit(key, polys, want_rows=True)
    with wave(zl):
        b = api.Dory.batchCommit(key, polys, want_rows=True)
    key.free()
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[1], b[1]))
    dev_rows = M.g1_unpack(*b[1][0])
    assert M.gt_unpack(b[0][:1])[0] == M.multi_pairing(dev_rows, pool.q[:rows])


def test_wave_verifier_setup_key_and_points(zl, pool):
    g1, g2 = (pool.g1[:4].copy(), np.zeros(4, dtype=np.uint8)), (pool.g2[:4].copy(), np.zeros(4, dtype=np.uint8))  # K = 2
    key = zl.DoryKey.create(g1, g2)
    with lane(zl):
        want = zl.dory_verifier_setup(key)
    with wave(zl):
        by_key = zl.dory_verifier_setup(key)
        by_points = zl.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1])
    key.free()
    for got in (by_key, by_points):
        assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
    assert M.gt_unpack(want[0][:1])[0] == M.final_exponentiation(pool.miller(0))  # chi[0] = e(g1[0], g2[0])


# ---------------------------------------------------------------- 7. the setter
def test_engine_context_manager_restores_and_refuses(zl):
    start = zl.pairing_engine_get()
    other = zl.PAIRING_ENGINE_WAVE if start == zl.PAIRING_ENGINE_LANE else zl.PAIRING_ENGINE_LANE
    with zl.pairing_engine(other):
        assert zl.pairing_engine_get() == other
        with zl.pairing_engine(start):
            assert zl.pairing_engine_get() == start
        assert zl.pairing_engine_get() == other
    assert zl.pairing_engine_get() == start
    with pytest.raises(KeyError):
        with zl.pairing_engine(other):
            raise KeyError("inside")
    assert zl.pairing_engine_get() == start
    for bad in (2, 7, -1):
        with pytest.raises(zl.ZgError) as ei:
            zl.pairing_engine_set(bad)
        assert ei.value.code == zl.ERR_INVALID and zl.pairing_engine_get() == start
    with pytest.raises(zl.ZgError):  # the context manager refuses before it changes anything
        with zl.pairing_engine(9):
            pass
    assert zl.pairing_engine_get() == start
    assert zl.abi_features() & 256


def test_two_threads_one_toggling_the_engine(zl, pool):
    """a call reads the engine once, so whichever engine each call meets, its bits are the expected ones"""
    n = 8
    with lane(zl):
        want = zl.multi_pairing(pool.g1[:n], None, pool.g2[:n], None)
        start = zl.pairing_engine_get()
        results, stop = [], threading.Event()

        def toggler():
            e = zl.PAIRING_ENGINE_WAVE
            while not stop.is_set():
                zl.pairing_engine_set(e)
                e ^= 1

        t = threading.Thread(target=toggler)
        t.start()
        try:
            for _ in range(6):
                results.append(zl.multi_pairing(pool.g1[:n], None, pool.g2[:n], None))
        finally:
            stop.set()
            t.join()
            zl.pairing_engine_set(start)
    assert all(np.array_equal(r, want) for r in results)
