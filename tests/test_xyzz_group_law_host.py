"""The canonical XYZZ group law (zolt_amd/csrc/xyzz.hip.h) over Fp and over Fp2, function by function, on the CPU: tests/cpp/xyzz_host.cpp
compiles the kernels' own headers for the host (hipcc --offload-host-only) and runs the record format of zg_selftest_xyzz
(zolt_amd/csrc/xyzz_selftest.hip.h) over stdin / stdout, once as it is and once as a stand-alone program built with
-fsanitize=address,undefined. The records choose the representative of every XYZZ operand, which no entry point that takes affine points
can: the identity on either side (zz == 0 over garbage), the same point and opposite points under equal and under different
representatives, a sum feeding the next addition, the scalars at every limb boundary of xyzz_scalar_mul, every aliasing xyzz_axpy_at
allows. The vectors, the model and the checker are tests/xyzz_model.py — the ones the device test (tests/test_gpu_xyzz_group_law.py) uses.
fe_inv_safegcd (the inversion of xyzz_to_affine) runs the structured values of tests/test_gpu_field.py and 2^16 uniform ones.

    python -m pytest tests/test_xyzz_group_law_host.py -q --durations=0"""
import os

import numpy as np
import pytest

from tests import xyzz_model as xm

pytestmark = pytest.mark.skipif(not os.path.exists(xm.HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

SEED = 2027


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return xm.compile_host(str(tmp_path_factory.mktemp("xyzz_host") / "xyzz_host"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return xm.compile_host(str(tmp_path_factory.mktemp("xyzz_host_san") / "xyzz_host_san"), extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.mark.parametrize("gid", [xm.G1, xm.G2], ids=["g1", "g2"])
@pytest.mark.parametrize("op", xm.ALL_OPS, ids=[xm.OP_NAMES[op] for op in xm.ALL_OPS])
def test_op(harness, gid, op):
    """every family of the op (records_for asserts that each is there) against the big-integer model"""
    items = xm.records_for(gid, op, SEED, xm.COUNTS[op])
    xm.check(xm.GROUPS[gid], op, items, harness(gid, op, items))


@pytest.mark.parametrize("gid", [xm.G1, xm.G2], ids=["g1", "g2"])
def test_inversion(harness, gid):
    """fe_inv_safegcd on raw words: Fp, and Fp2 through its norm"""
    items = xm.records_for(gid, xm.INV, SEED, xm.inv_total(gid))
    assert sum(it[0] == "random" for it in items) == xm.INV_RANDOM
    xm.check(xm.GROUPS[gid], xm.INV, items, harness(gid, xm.INV, items))


@pytest.mark.parametrize("gid", [xm.G1, xm.G2], ids=["g1", "g2"])
def test_under_asan_and_ubsan(harness, harness_san, gid):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined: a shift past a word's width, a signed overflow
    or an index past a local array ends the run with a report instead of a result. Its outputs are the plain build's, word for word"""
    for op in xm.ALL_OPS + (xm.INV,):
        items = xm.records_for(gid, op, SEED, xm.COUNTS[op])[:96] if op != xm.INV else xm.records_for(gid, xm.INV, SEED, xm.inv_total(gid))[:2048]
        out = harness_san(gid, op, items)
        xm.check(xm.GROUPS[gid], op, items, out)
        assert np.array_equal(out, harness(gid, op, items))


def test_the_checker_can_fail(harness):
    """one word, one flag and one record off: the checker says so (a checker that accepts everything would pass every test above)"""
    for gid in (xm.G1, xm.G2):
        grp = xm.GROUPS[gid]
        W = grp.W
        for op in (xm.ADD, xm.AXPY, xm.TO_AFFINE):
            items = xm.records_for(gid, op, SEED, xm.COUNTS[op])
            out = harness(gid, op, items).copy()
            xm.check(grp, op, items, out)
            point = next(i for i, it in enumerate(items) if it[0] in ("regular", "inf_none", "general"))
            ident = next(i for i, it in enumerate(items) if it[0] in ("opposite_other_rep", "inf_both", "identity"))
            flips = [(point, 0, 1), (point, W, 1 << 63), (point, 2 * W - 1, 1 << 40), (point, 4 * W, 1), (ident, 4 * W, 1), (point, 4 * W + 1, 1)]
            if op == xm.ADD:
                flips += [(point, 2 * W, 1), (point, 3 * W, 1), (ident, 2 * W, 1)]  # zz and zzz alone: zz^3 != zzz^2; an identity whose zz != 0
            else:
                flips += [(ident, 0, 1), (ident, 2 * W - 1, 2)]  # how the group writes an identity
            for row, word, delta in flips:
                bad = out.copy()
                bad[row, word] ^= np.uint64(delta)
                with pytest.raises(AssertionError):
                    xm.check(grp, op, items, bad)
            swapped = out.copy()
            swapped[[point, ident]] = swapped[[ident, point]]  # one record off
            with pytest.raises(AssertionError):
                xm.check(grp, op, items, swapped)
            with pytest.raises(AssertionError):
                xm.check(grp, op, items, out[:-1])


def test_the_model_is_bn254():
    """the checker's own arithmetic against closed forms: the generators' order, the affine laws against the Jacobian walk, the two G2
    scalar multiplications, associativity"""
    for grp in xm.GROUPS:
        G = grp.G
        assert grp.on_curve(G) and grp.mul(G, xm.R) is None and grp.mul(G, xm.R - 1) == grp.neg(G)
        assert grp.mul(G, xm.R + 5) == grp.mul(G, 5) and grp.mul(G, xm.ALL_BUT_BIT_255) == grp.mul(G, xm.ALL_BUT_BIT_255 % xm.R)
        acc = None
        for k in range(1, 9):
            acc = grp.add(acc, G)
            assert acc == grp.mul(G, k) and grp.on_curve(acc)
        a, b, c = grp.mul(G, 77), grp.mul(G, 1 << 100), grp.mul(G, xm.R - 3)
        assert grp.add(grp.add(a, b), c) == grp.add(a, grp.add(b, c)) and grp.add(a, a) == grp.double(a) and grp.add(a, grp.neg(a)) is None
        assert grp.add(c, grp.mul(G, 3)) is None
        F, lam = grp.F, grp.F.rand(xm.Gen(grp, 1).rng)
        x, y, zz, zzz = grp.rep(a, lam)
        assert F.mul(x, F.inv(zz)) == a[0] and F.mul(y, F.inv(zzz)) == a[1] and F.mul(F.mul(zz, zz), zz) == F.mul(zzz, zzz)
    assert xm.GROUPS[1].mul(xm.M.G, 123456789) == xm.M.scalar_mul(xm.M.G, 123456789) == xm.M.scalar_mul_affine(xm.M.G, 123456789)
