"""The canonical XYZZ group law (zolt_amd/csrc/xyzz.hip.h) ON THE DEVICE, function by function, over Fp (G1) and over Fp2 (G2):
zg_selftest_xyzz (zolt_amd/csrc/selftest.hip) runs the functions that small_msm.hip.h, g2.hip, points.hip and dory.hip call on records
whose XYZZ representatives tests/xyzz_model.py chooses — identities over garbage, the same point and opposite points under equal and under
different representatives, chained additions, the scalars at the limb boundaries of xyzz_scalar_mul, every aliasing of xyzz_axpy_at — one
record per lane, the branches side by side in one wave. Every comparison is exact: group elements against the big-integer model, affine
outputs word for word, and every output word against the same header compiled for the CPU (tests/cpp/xyzz_host.cpp).

    python -m pytest tests/test_gpu_xyzz_group_law.py -m gpu -q --durations=0"""
import os

import numpy as np
import pytest

from tests import xyzz_model as xm

pytestmark = pytest.mark.gpu
SEED = 2027  # the records of tests/test_xyzz_group_law_host.py
GROUPS = pytest.mark.parametrize("gid", [xm.G1, xm.G2], ids=["g1", "g2"])


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(xm.HIPCC):
        pytest.skip("hipcc is absent: the host harness compiles the kernels' own HIP headers")
    return xm.compile_host(str(tmp_path_factory.mktemp("xyzz_host") / "xyzz_host"))


def _device(zl, gid, op, items):
    grp = xm.GROUPS[gid]
    return np.concatenate([zl.selftest_xyzz(gid, op, xm.pack(grp, items[lo:lo + xm.MAX_RECORDS])) for lo in range(0, len(items), xm.MAX_RECORDS)])


@GROUPS
@pytest.mark.parametrize("op", xm.ALL_OPS, ids=[xm.OP_NAMES[op] for op in xm.ALL_OPS])
def test_op(zl, gid, op):
    """every family of the op against the model, the first wave holding every branch"""
    items = xm.records_for(gid, op, SEED, xm.COUNTS[op])
    assert {it[0] for it in items[:64]} >= set(xm.REQUIRED[op])
    xm.check(xm.GROUPS[gid], op, items, _device(zl, gid, op, items))


@GROUPS
def test_inversion(zl, gid):
    """fe_inv_safegcd, the inversion of xyzz_to_affine: the structured values and 2^16 uniform ones (Fp2 through its norm)"""
    items = xm.records_for(gid, xm.INV, SEED, xm.inv_total(gid))
    xm.check(xm.GROUPS[gid], xm.INV, items, _device(zl, gid, xm.INV, items))


@GROUPS
def test_the_device_writes_the_host_builds_words(zl, host, gid):
    """the same header compiled for the CPU (tests/cpp/xyzz_host.cpp), the same records: every output word of every op, the coordinates
    under zz == 0 that the checker does not read included"""
    for op in xm.ALL_OPS + (xm.INV,):
        items = xm.records_for(gid, op, SEED, xm.inv_total(gid) if op == xm.INV else xm.COUNTS[op])
        assert np.array_equal(_device(zl, gid, op, items), host(gid, op, items)), xm.OP_NAMES[op]


@GROUPS
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_launch_edges(zl, gid, n):
    """a last wave that is one lane, one short of full, full, one over: every op; the rows are those of the longer run"""
    for op in xm.ALL_OPS + (xm.INV,):
        items = xm.records_for(gid, op, SEED, xm.inv_total(gid) if op == xm.INV else xm.COUNTS[op])[:n]
        out = zl.selftest_xyzz(gid, op, xm.pack(xm.GROUPS[gid], items))
        assert out.shape == (n, xm.GROUPS[gid].OUT_WORDS)
        xm.check(xm.GROUPS[gid], op, items, out)


def test_bad_arguments_are_error_codes(zl):
    for gid in (xm.G1, xm.G2):
        rec = np.zeros((1, xm.GROUPS[gid].IN_WORDS), dtype=np.uint64)
        out = np.zeros((1, xm.GROUPS[gid].OUT_WORDS), dtype=np.uint64)
        for op in (-1, 9, 1 << 20):
            assert zl._lib.zg_selftest_xyzz(gid, op, rec.ctypes.data, 1, out.ctypes.data) == zl.ERR_INVALID
        assert zl._lib.zg_selftest_xyzz(gid, xm.ADD, rec.ctypes.data, 0, out.ctypes.data) == zl.ERR_INVALID
        assert zl._lib.zg_selftest_xyzz(gid, xm.ADD, rec.ctypes.data, (1 << 16) + 1, out.ctypes.data) == zl.ERR_INVALID
        assert zl._lib.zg_selftest_xyzz(gid, xm.ADD, None, 1, out.ctypes.data) == zl.ERR_INVALID
        assert zl._lib.zg_selftest_xyzz(gid, xm.ADD, rec.ctypes.data, 1, None) == zl.ERR_INVALID
    rec = np.zeros((1, xm.GROUPS[1].IN_WORDS), dtype=np.uint64)
    out = np.zeros((1, xm.GROUPS[1].OUT_WORDS), dtype=np.uint64)
    for group in (-1, 2):
        assert zl._lib.zg_selftest_xyzz(group, xm.ADD, rec.ctypes.data, 1, out.ctypes.data) == zl.ERR_INVALID
    with pytest.raises(zl.ZgError) as err:
        zl.selftest_xyzz(0, 9, np.zeros((1, xm.GROUPS[0].IN_WORDS), dtype=np.uint64))
    assert err.value.code == zl.ERR_INVALID
