"""The MSM's lazy-limb group law and its interleaved products ON THE DEVICE, function by function, on raw limbs: zg_selftest_lazy_g1
(zolt_amd/csrc/selftest.hip) runs the functions msm.hip calls — xyzz29_madd_nz with the inline-assembly product groups, the exceptional
finish, xyzz29_add / dbl, jac29_dbl, the four-lane forms, every product form and every biased subtraction alone — on records that
tests/lazy_model.py builds at the edges of the classes the headers state: top representatives, limbs in [2^29, 2^29 + 8), acc == +-P under
both signs, and the branches side by side in one wave. The same vectors run on the CPU in tests/test_lazy_group_law_host.py.

    python -m pytest tests/test_gpu_lazy_group_law.py -m gpu -q -s --durations=0"""
import numpy as np
import pytest

from tests import lazy_model as lm

pytestmark = pytest.mark.gpu
SEED = 20260


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


def _family(zl, op, n, need, first=64):
    items = lm.records_for(op, SEED + op, n)
    assert len(items) == n
    lm.assert_in_class(op, items)
    head = {it[0] for it in items[:first]}  # one wave: 64 single-lane records, or the 16 adjacent quads of a four-lane op
    assert all(any(k.startswith(w) for k in head) for w in need), (sorted(head), need)
    out = zl.selftest_lazy_g1(op, lm.pack(items))
    mx = lm.check(op, items, out, device=True)
    print(f"{lm.OP_NAMES[op]}: {n} records, largest outputs / p: {dict(mx)}")
    return items, out


def test_madd(zl):
    """xyzz29_madd_nz as the accumulate loop has it (the interleaved asm products), then xyzz29_madd_except: one wave holds regular,
    doubling and infinity records under both signs, run-start accumulators and forced limb patterns side by side"""
    items, _ = _family(zl, lm.MADD, 512, ["regular+", "regular-", "double+", "double-", "infinity+", "infinity-", "run-start", "forced-"])
    kinds = {it[0] for it in items}
    assert all(any(k.startswith(w) for k in kinds) for w in ("forced-x-double", "forced-x-infinity", "forced-y", "forced-zz", "forced-zzz", "forced-y-2p"))


def test_start(zl):
    """xyzz29_start (with the first point's sign) followed by one mixed addition: the run-start accumulator whose y is <= 2p"""
    _family(zl, lm.START, 256, ["regular++", "regular+-", "regular-+", "regular--", "double", "infinity"])


def test_add(zl):
    _family(zl, lm.ADD, 512, ["regular", "double", "infinity", "identity-a", "identity-b", "forced-"])


def test_dbl_and_jdbl(zl):
    _family(zl, lm.DBL, 256, ["regular", "identity", "forced-x", "forced-y", "forced-zz", "forced-zzz"])
    _family(zl, lm.JDBL, 256, ["zero", "top", "forced-x", "forced-y", "forced-z"])


def test_quad_ops(zl):
    """xyzz29_madd4 / add4 / dbl4, one record per quad: the sixteen adjacent quads of a wave take different branches, and the four lanes
    of each return identical limbs"""
    _family(zl, lm.MADD4, 512, ["regular", "double", "infinity", "start"], first=16)
    _family(zl, lm.ADD4, 512, ["regular", "double", "infinity", "identity-a", "identity-b"], first=16)
    _family(zl, lm.DBL4, 256, ["regular", "identity", "forced-"], first=16)


def test_prod_asm_forms_are_the_compiler_forms(zl):
    """f29_mul_x2 / mul_x3 / sqr_x2 / mul2_mul against f29_mul / sqr / mul2 bit for bit, and all of them against a*b*2^-261 and the product
    bound, at the class products of the mixed addition with all low limbs at 2^29 + 7"""
    _family(zl, lm.PROD, 2048, ["worst", "forced", "top-exact", "rand"])


def test_lin(zl):
    items, out = _family(zl, lm.LIN, 2048, ["zero-", "near-", "random"])
    kinds = {it[0] for it in items}
    assert {"zero-0p", "zero-16p", "zero-17p", "near-0p-raised", "sub-extreme", "x3-extreme", "to-fp-edge"} <= kinds
    yes = {it[0] for it, o in zip(items, out) if o[144]}
    assert sorted(yes - {"to-fp-edge"}) == sorted(f"zero-{k}p" for k in range(17)), sorted(yes)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_launch_edges(zl, n):
    """a last wave that is one lane, one short of full, full, one over; more than one block: single-lane and four-lane kernels. The
    records past n are not touched: the output rows of a longer run agree with the shorter one's"""
    for op in (lm.MADD, lm.ADD4):
        items = lm.records_for(op, SEED, 258)[:n]
        out = zl.selftest_lazy_g1(op, lm.pack(items))
        assert out.shape == (n, lm.OUT_WORDS)
        lm.check(op, items, out, device=True)


def test_bad_arguments_are_error_codes(zl):
    rec = np.zeros((1, lm.IN_WORDS), dtype=np.uint32)
    for op in (-1, 10, 1 << 20):
        with pytest.raises(zl.ZgError) as err:
            zl.selftest_lazy_g1(op, rec)
        assert err.value.code == zl.ERR_INVALID
    with pytest.raises(zl.ZgError) as err:
        zl.selftest_lazy_g1(lm.MADD, np.zeros((0, lm.IN_WORDS), dtype=np.uint32))
    assert err.value.code == zl.ERR_INVALID
    out = np.zeros((1, lm.OUT_WORDS), dtype=np.uint32)
    assert zl._lib.zg_selftest_lazy_g1(0, None, 1, out.ctypes.data) == zl.ERR_INVALID
    assert zl._lib.zg_selftest_lazy_g1(0, rec.ctypes.data, 1, None) == zl.ERR_INVALID
