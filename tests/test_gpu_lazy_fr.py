"""The sumcheck kernels' lazy Fr arithmetic and their lazy 288-bit sums ON THE DEVICE, function by function, on raw limbs:
zg_selftest_lazy_fr (zolt_amd/csrc/selftest.hip) runs the functions poly.hip, psc.hip, rrw.hip, rwc.hip and ingest.hip call — f29t_mul<Fr29>
and its short forms, the prescaled and narrow factors, fr_from_u64_29, the 64- and 32-bit limb sums with ChainAcc4's carry passes and
in-loop flush, acc9_add / add_if / add_acc / reduce — on records that tests/lazy_fr_model.py places at the edges of the classes the
headers state: top representatives, limbs raised to 2^30 - 1, 64 values of 2 r - 1, sums up to 2^284 - 1. The same vectors run on the CPU
in tests/test_lazy_fr_host.py. The block reduction (the DPP additions, wave_sum_pair9, all three branches of block_sum_pair9's cross-wave
step) runs here only: one workgroup per case, every thread its own raw pair of sums.

    python -m pytest tests/test_gpu_lazy_fr.py -m gpu -q -s --durations=0"""
import numpy as np
import pytest

from tests import lazy_fr_model as fm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


def _run(zl):
    return lambda op, items: zl.selftest_lazy_fr(op, fm.pack(items))


def test_mul(zl):
    _, _, mx = fm.family(_run(zl), fm.MUL)
    assert max(v for k, v in mx.items() if k.startswith("mul ")) < fm.OUT_MAX


def test_mul_short(zl):
    fm.family(_run(zl), fm.MUL_SHORT5)
    fm.family(_run(zl), fm.MUL_SHORT3)


def test_canonical_entry_points(zl):
    """both paths of frmul_apply side by side in one wave, against fe_mul and x y R^-1 mod r"""
    items, out, _ = fm.family(_run(zl), fm.CANON)
    head = {(it[0], int(o[145])) for it, o in zip(items[:64], out[:64])}
    assert {a for _, a in head} == {0, 1}, head
    narrow = {it[0] for it, o in zip(items, out) if o[145]}
    assert {"y-zero", "rand-narrow", "narrow-H-1"} <= narrow and not any(k.startswith("one-low-word") or k in ("rand", "y-one-mont") for k in narrow), sorted(narrow)


def test_sum64_and_sum32(zl):
    """lanes of one wave run different counts: the in-loop flush of ChainAcc4 at 64 is taken by some lanes and not by their neighbours"""
    fm.family(_run(zl), fm.SUM64)
    items, _, _ = fm.family(_run(zl), fm.SUM32)
    assert len({int(it[1][144]) for it in items[:64]}) >= 11


def test_carry_and_acc9(zl):
    fm.family(_run(zl), fm.CARRY)
    _, _, mx = fm.family(_run(zl), fm.ACC9)
    assert mx["acc9 bits"] == 284


@pytest.mark.parametrize("threads", fm.BLOCK_SIZES)
def test_block_sum(zl, threads):
    """block_sum_pair9 over one workgroup of 1, 2, 3, 4 (totals moved from lanes 3 / 35), 5, 8 and 16 waves: all-ones low limbs (every DPP
    addition carries across all nine limbs), one non-zero thread at each lane where a row or a half-wave ends and in the last wave, zeros"""
    cases = fm.blocksum_cases(threads, fm.SEED)
    kinds = [k for k, _ in cases]
    assert all(w in kinds for w in ["all-ones-low", "zero", "rand", "last-wave-first", "last-wave-last"] + [f"single-lane-{l}" for l in (0, 15, 16, 31, 32, 63)])
    out = zl.selftest_lazy_fr(fm.BLOCKSUM, np.stack([a for _, a in cases]), threads=threads)
    fm.check_blocksum(cases, out)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_launch_edges(zl, n):
    """a last wave that is one lane, one short of full, one over: the records past n are not touched"""
    items = fm.records_for(fm.MUL, fm.SEED, 66)[:n]
    out = zl.selftest_lazy_fr(fm.MUL, fm.pack(items))
    fm.check(fm.MUL, items, out)


def test_bad_arguments_are_error_codes(zl):
    rec = np.zeros((1, fm.IN_WORDS), dtype=np.uint32)
    for op, threads in ((-1, 0), (9, 0), (1 << 20, 0), (fm.MUL, 64), (fm.BLOCKSUM, 0), (fm.BLOCKSUM, 32), (fm.BLOCKSUM, 96), (fm.BLOCKSUM, 1088)):
        out = np.zeros((1, fm.OUT_WORDS), dtype=np.uint32)
        assert zl._lib.zg_selftest_lazy_fr(op, rec.ctypes.data, 1, out.ctypes.data, threads) == zl.ERR_INVALID, (op, threads)
    out = np.zeros((1, fm.OUT_WORDS), dtype=np.uint32)
    assert zl._lib.zg_selftest_lazy_fr(0, None, 1, out.ctypes.data, 0) == zl.ERR_INVALID
    assert zl._lib.zg_selftest_lazy_fr(0, rec.ctypes.data, 1, None, 0) == zl.ERR_INVALID
    assert zl._lib.zg_selftest_lazy_fr(0, rec.ctypes.data, 0, out.ctypes.data, 0) == zl.ERR_INVALID
    assert zl._lib.zg_selftest_lazy_fr(0, rec.ctypes.data, (1 << 12) + 1, out.ctypes.data, 0) == zl.ERR_INVALID
    assert zl._lib.zg_selftest_lazy_fr(0, None, 0, None, 0) == zl.ERR_INVALID
