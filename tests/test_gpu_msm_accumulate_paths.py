"""The accumulate loop's sign and run-start paths, driven hard through the public MSM entry point and checked against the closed form.

The loop folds a digit's sign into R = +-S2 - Y1 of the mixed addition (a subtracted point never has its y negated first), applies
the sign where a bucket run starts (the point is copied into the accumulator), walks the run ends by rank and finishes the
exceptional additions (acc == +-P) from the point alone. The scalar vectors below are built from their signed digits, so that a
whole vector takes one of those paths: every digit negative, digits alternating in sign, a 0/1 column, and one entry per bucket
(every addition is a run start, with either sign). Bases are (i+1)G, so the MSM is (sum s_i (i+1) mod r) G: one scalar
multiplication on an independent kernel. Each vector runs through the lane-per-chunk kernel and the quad-per-chunk kernel
(ZG_MSM_QUAD_ACC_MAX_CHUNKS) and with long chunks (ZG_MSM_CHUNK_THREADS), under an explicit window size and the automatic plan.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


@pytest.fixture(scope="module")
def gm(ob):
    return ob.g1_gen_multiples(1 << 16)  # P_i = (i+1)G


def _value(digits, c):
    """the integer whose signed c-bit digits (|d| < 2^(c-1), lowest window first) are `digits`"""
    return sum(int(d) << (c * j) for j, d in enumerate(digits))


def _vectors(c, n, rng):
    """name -> list of n non-negative integers below 2^253 < r"""
    top = 253 // c  # the window that takes the final carry: digit +1 there keeps the value positive
    half = 1 << (c - 1)
    out = {}
    # every digit below the top one negative
    mags = rng.integers(1, half, size=(n, top))
    out["all_negative"] = [(1 << (c * top)) - _value(m, c) for m in mags]
    # digits alternating in sign along the scalar and from one scalar to the next (a bucket run mixes both signs)
    mags = rng.integers(1, half, size=(n, top))
    alt = []
    for i, m in enumerate(mags):
        d = [int(v) if (i + j) % 2 else -int(v) for j, v in enumerate(m)]
        alt.append((1 << (c * top)) + _value(d, c))
    out["alternating"] = alt
    # a 0/1 column: one bucket holds half of the points
    out["zero_one"] = [int(v) for v in rng.integers(0, 2, size=n)]
    # one entry per bucket in windows 0 and 1: digit -(i+1) below, perm(i)+1 above (m <= 2^(c-1) - 1 points use every magnitude once)
    m = min(n, half - 1)
    perm = rng.permutation(m)
    one = [((int(perm[i]) + 1) << c) - (i + 1) for i in range(m)] + [0] * (n - m)
    out["one_per_bucket"] = one
    # the same with positive digits only
    out["one_per_bucket_positive"] = [((int(perm[i]) + 1) << c) + (i + 1) for i in range(m)] + [0] * (n - m)
    return out


def _mont(zl, vals):
    raw = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)
    return zl.field_op(zl.FR, zl.OP_TO_MONT, raw)


ENVS = [{}, {"ZG_MSM_QUAD_ACC_MAX_CHUNKS": "0"}, {"ZG_MSM_QUAD_ACC_MAX_CHUNKS": "1000000"},
        {"ZG_MSM_QUAD_ACC_MAX_CHUNKS": "0", "ZG_MSM_CHUNK_THREADS": "1000"}]


@pytest.mark.parametrize("cfg", [dict(window_bits=13, precompute_levels=0), dict(window_bits=8, precompute_levels=1), dict()])
def test_sign_and_run_start_paths_against_closed_form(zl, ob, gm, cfg, monkeypatch):
    from zolt_amd import api
    n = 1 << 16
    g = api.generator()
    rng = np.random.default_rng(2917)
    cases = None
    for env in ENVS:
        for k in ("ZG_MSM_QUAD_ACC_MAX_CHUNKS", "ZG_MSM_CHUNK_THREADS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        b = zl.Bases.upload(gm[:n], **cfg)  # the plan reads ZG_MSM_CHUNK_THREADS at upload
        try:
            c = b.plan()[0]
            if cases is None:  # the window size does not depend on the switches above
                cases = []
                for name, vals in _vectors(c, n, rng).items():
                    assert all(0 <= v < (1 << 253) for v in vals), name
                    want_k = sum(v * (i + 1) for i, v in enumerate(vals)) % api.R_MOD
                    cases.append((name, _mont(zl, vals), api.MSM.scalarMul(g, api.fr_from_int(want_k))))
            for name, sc, want in cases:
                got = b.msm(sc)
                assert got[1] == want[1] and np.array_equal(got[0], want[0]), (name, cfg, env, c)
        finally:
            b.free()


def test_repeated_and_opposite_points_finish_from_the_point_alone(zl, ob, gm, monkeypatch):
    """acc == P (the sum is 2P) and acc == -P (the sum is infinity) inside the lane-per-chunk loop, with both signs of the digit:
    the same base many times, and a base beside its negative."""
    from zolt_amd import api
    monkeypatch.setenv("ZG_MSM_QUAD_ACC_MAX_CHUNKS", "0")
    n = 4096
    g = api.generator()
    rng = np.random.default_rng(77)
    neg = gm[:n].copy()
    neg[:, 4:] = ob.f_neg(ob.FP, gm[:n, 4:])
    same = np.repeat(gm[6:7], n, axis=0)  # 7G, n times
    for c in (8, 13):
        top = 253 // c
        half = 1 << (c - 1)
        d0 = int(rng.integers(1, half))
        for sign in (1, -1):
            # every scalar has the same digits, so a bucket's run is the same point again and again: P + P first, then kP + P
            v = (1 << (c * top)) + sign * _value([d0] * top, c)
            b = zl.Bases.upload(same, window_bits=c, precompute_levels=1)
            try:
                got = b.msm(_mont(zl, [v] * n))
            finally:
                b.free()
            want = api.MSM.scalarMul(g, api.fr_from_int(7 * n * v % api.R_MOD))
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (c, sign)
            # P_i and -P_i with the same scalar, next to each other in a bucket's run: every pair cancels
            xy = np.empty((2 * n, 8), dtype=np.uint64)
            xy[0::2], xy[1::2] = gm[:n], neg
            b = zl.Bases.upload(xy, window_bits=c, precompute_levels=1)
            try:
                got = b.msm(_mont(zl, [v] * (2 * n)))
            finally:
                b.free()
            assert got[1] == 1 and not got[0].any(), (c, sign)
