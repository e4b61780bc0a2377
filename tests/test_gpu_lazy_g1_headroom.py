"""The un-carried linear forms of the mixed addition ON THE DEVICE (zolt_amd/csrc/g1_29.hip.h: xyzz29_madd_nz with P, R and 4p - Y1
un-carried; fp29.hip.h: f29_sub7_raw, f29_pmsub45_raw, f29_neg4_raw). The inline-assembly product groups exist on the device only, so
the records of tests/lazy_headroom_records.py — limbs at the edges the larger operands matter for, both signs, acc = +-P — go through
zg_selftest_lazy_g1 twice from one binary: as the accumulate loop has the addition, and in the carried reference form
(LAZY_MADD_CARRY_ALL). Required: limb-identical to each other and to the host run of the same records (the program of
tests/test_lazy_g1_headroom_host.py, built here too: a second and a half), and right by the big-integer model. Then one MSM through
the device entry point at the smallest size class that takes msm_accumulate_chunk_kernel<false>, with a scalar vector whose digits
are mostly negative.

    python -m pytest tests/test_gpu_lazy_g1_headroom.py -m gpu -q -s --durations=0"""
import numpy as np
import pytest

from tests import lazy_headroom_records as hr
from tests import lazy_model as lm

pytestmark = pytest.mark.gpu
SEED = 20261  # the host test's: the same records


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return hr.host_harness(str(tmp_path_factory.mktemp("lazy_g1_headroom") / "host"))


def _both(zl, op, items):
    rec = lm.pack(items)
    ref = rec.copy()
    if op == lm.LIN:
        ref[:, 90] &= np.uint32(~hr.LIN_RAW & 0xFFFFFFFF)
    else:
        ref[:, 90] |= np.uint32(hr.MADD_CARRY_ALL)
    return zl.selftest_lazy_g1(op, rec), zl.selftest_lazy_g1(op, ref)


def test_madd_uncarried_is_the_carried_addition(zl, host):
    items = hr.madd_items(SEED, 3072)
    lm.assert_in_class(lm.MADD, items)
    head = {it[0] for it in items[:64]}  # the edge records share waves with each other under both signs, regular beside exceptional
    assert any(k.startswith("x-limbs-max-double") for k in head) and any(k.startswith("x-limbs-max+") for k in head), sorted(head)
    new, ref = _both(zl, lm.MADD, items)
    mx = hr.check_madd(items, new, ref, device=True)
    assert np.array_equal(new, host(lm.MADD, items)[0]), "device and host differ"
    print(f"madd: {len(items)} records, largest outputs / p: {dict(mx)}")


def test_start_uncarried_is_the_carried_addition(zl, host):
    items = lm.start_records(SEED + 2, 256)
    new, ref = _both(zl, lm.START, items)
    assert np.array_equal(new, ref) and np.array_equal(new, host(lm.START, items)[0])
    lm.check(lm.START, items, new, device=True)


def test_raw_linear_forms_and_the_zero_test(zl, host):
    items = hr.lin_items(SEED, 2048)
    new, ref = _both(zl, lm.LIN, items)
    assert np.array_equal(new, host(lm.LIN, items)[0]), "device and host differ"
    hr.check_lin(items, new, ref)


def test_msm_on_the_lane_per_chunk_path_with_negative_digits(zl):
    """2^15 + 77 points under the automatic plan: c = 16, 16 windows, so the launch has (2^15 + 77) * 16 digits, aims at 16 per chunk and
    takes 65536 chunks — above the 32768 up to which the quad-per-chunk kernel runs (msm.hip: accumulate_range), while 2^15 points
    would still take it. Every digit below the top one is negative or the digits alternate in sign, so R = 5p - S2 - Y1, the form
    whose un-carried limbs are the largest, runs in nearly every addition. Bases (i + 1) G: the sum is (sum s_i (i + 1)) G."""
    import torch
    from oracle import binding as ob
    from zolt_amd import api
    n = (1 << 15) + 77
    gm = ob.g1_gen_multiples(n)
    b = zl.Bases.upload(gm)
    try:
        c, w, levels = b.plan()
        assert (c, w) == (16, 16), (c, w, levels)
        chunks = lambda pts: max(1024, 1 << ((pts * w // 16) - 1).bit_length())  # msm_plan.h: chunk_threads
        assert chunks(n) > 32768 >= chunks(1 << 15)  # the non-quad kernel; one size class lower it is the quad kernel
        rng = np.random.default_rng(515)
        top, half = 253 // c, 1 << (c - 1)
        mags = rng.integers(1, half, size=(n, top))
        vals = []
        for i, m in enumerate(mags):
            d = [-int(v) for v in m] if i % 4 else [int(v) if j % 2 else -int(v) for j, v in enumerate(m)]
            vals.append((1 << (c * top)) + sum(x << (c * j) for j, x in enumerate(d)))
        assert all(0 < v < 1 << 254 for v in vals)
        raw = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)
        sc = zl.field_op(zl.FR, zl.OP_TO_MONT, raw)
        want = api.MSM.scalarMul(api.generator(), api.fr_from_int(sum(v * (i + 1) for i, v in enumerate(vals)) % api.R_MOD))
        d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        got = b.msm_dev(d_sc.data_ptr(), n)
    finally:
        b.free()
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
