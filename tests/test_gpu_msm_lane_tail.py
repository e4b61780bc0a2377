"""The LANE form of the MSM bucket tail (msm_bucket_combine_lane_kernel, msm_rowcol_lane_kernel; msm_plan.h: plan_tail) against the QUAD
form and the closed form. Every case runs twice over the same handle settings, with ZG_MSM_LANE_TAIL=1 and with =0 (the planner reads
the switch for every plan, i.e. at every upload, so one process serves both), and the two results must agree byte for byte with each
other and with (sum s_i k_i)·G for bases k_i·G.

Shapes: the smallest that reach every branch of the lane kernels — ZG_MSM_WINDOW_BITS=13 (6 x 6 buckets: rows and columns of 64, one
lane stage and two quad stages) at n = 4096 and ZG_MSM_WINDOW_BITS=15 (split 6 x 8 under the switch: rows of 64, columns of 256 with
two lane stages) at n = 2^15.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import util as U

pytestmark = pytest.mark.gpu

SHAPES = [(13, 1 << 12), (15, 1 << 15)]  # (window bits, points)


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
    return ob.g1_gen_multiples(1 << 17)  # P_i = (i+1)G


@contextlib.contextmanager
def _switches(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _msm(zl, xy, sc, **switches):
    with _switches(**switches):
        b = zl.Bases.upload(xy)
        got, ginf = b.msm(sc)
        b.free()
    return got, ginf


def _both_forms(zl, xy, sc, want, **switches):
    """want: the affine point (x, y) as canonical ints, or None for the identity"""
    lane = _msm(zl, xy, sc, ZG_MSM_LANE_TAIL=1, **switches)
    quad = _msm(zl, xy, sc, ZG_MSM_LANE_TAIL=0, **switches)
    assert lane[1] == quad[1] and np.array_equal(lane[0], quad[0]), (lane, quad)
    assert U.point_from_xy(*lane) == want
    if want is None:
        assert not lane[0].any()


def _closed_form(ks, ints):
    from oracle import pymodel as pm
    return pm.msm_generator_multiples(ks, ints)


def _fr(ob, ints):
    from oracle import pymodel as pm
    return np.array([pm.limbs(pm.to_mont(v, pm.R_MOD)) for v in ints], dtype=np.uint64).reshape(-1, 4)


def _scalar_ints(kind, n):
    from oracle import pymodel as pm
    if kind == "uniform":
        return [pm.from_limbs(r) % pm.R_MOD for r in U.random_raw256(900 + n, n)]
    if kind == "zero":
        return [0] * n
    if kind == "equal":
        return [pm.from_limbs(U.random_raw256(17, 1)[0]) % pm.R_MOD] * n
    assert kind == "bits"  # 0 / 1: one bucket takes half the points — the heavy path runs beside the lane path
    return [int(v) for v in np.random.default_rng(n).integers(0, 2, size=n)]


@pytest.mark.parametrize("c,n", SHAPES)
@pytest.mark.parametrize("kind", ["uniform", "zero", "equal", "bits"])
def test_lane_equals_quad_and_closed_form(zl, ob, gm, c, n, kind):
    ints = _scalar_ints(kind, n)
    _both_forms(zl, gm[:n], _fr(ob, ints), _closed_form(range(1, n + 1), ints), ZG_MSM_WINDOW_BITS=c)


@pytest.mark.parametrize("c,n", SHAPES)
def test_cancelling_pairs(zl, ob, gm, c, n):
    """Bases P_0, -P_0, P_1, -P_1, ...; both points of a pair carry the same scalar, +1 and -1 alternating from pair to pair: every
    bucket's total — and the MSM — is the identity, met by the additions of both forms as P + (-P)."""
    from oracle import pymodel as pm
    xy = np.repeat(gm[:n // 2], 2, axis=0)
    xy[1::2, 4:] = ob.f_neg(ob.FP, xy[1::2, 4:])
    ints = [1 if (i // 2) % 2 == 0 else pm.R_MOD - 1 for i in range(n)]
    _both_forms(zl, xy, _fr(ob, ints), None, ZG_MSM_WINDOW_BITS=c)


@pytest.mark.parametrize("c", [13, 15])
def test_single_point(zl, ob, gm, c):
    from oracle import pymodel as pm
    ints = [pm.from_limbs(U.random_raw256(23, 1)[0]) % pm.R_MOD]
    _both_forms(zl, gm[:1], _fr(ob, ints), _closed_form([1], ints), ZG_MSM_WINDOW_BITS=c)


def test_light_heavy_boundary(zl, ob, gm):
    """Both sides of the light / heavy boundary (8 partials). 4096 scalars below 2^12 have one non-zero digit each (window 0, the digit
    is the scalar), so the sorted list has 4096 entries; ZG_MSM_CHUNK_THREADS=256 cuts it into chunks of 16. Digit 1 takes entries
    [0, 128): chunks 0 .. 7, exactly 8 partials — the lane kernel sums it. Digit 2 takes [128, 272): chunks 8 .. 16, 9 partials — queued
    for msm_heavy_kernel. The rest spread over digits 3 .. 1002."""
    n = 4096
    ints = [1] * 128 + [2] * 144 + [3 + i % 1000 for i in range(n - 272)]
    _both_forms(zl, gm[:n], _fr(ob, ints), _closed_form(range(1, n + 1), ints), ZG_MSM_WINDOW_BITS=13, ZG_MSM_CHUNK_THREADS=256)


def test_auto_keeps_quad_at_2_17(zl, ob, gm):
    """The automatic rule leaves a 2^17-point handle (c = 16: 8 x 7 buckets) on the QUAD kernels: same bytes as with the switch off."""
    n = 1 << 17
    ints = _scalar_ints("uniform", n)
    sc = _fr(ob, ints)
    auto = _msm(zl, gm, sc, ZG_MSM_LANE_TAIL="auto")
    off = _msm(zl, gm, sc, ZG_MSM_LANE_TAIL=0)
    assert auto[1] == off[1] and np.array_equal(auto[0], off[0])
    assert U.point_from_xy(*auto) == _closed_form(range(1, n + 1), ints)
