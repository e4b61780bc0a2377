"""Pins tests/g2_model.py (the big-integer checker of the G2 GPU tests) before anything on the device is compared with it, and the
CPU-side facts of the G2 section of the ABI. No GPU needed."""
import random
import re
import os

import numpy as np

from tests import g2_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G2_EXPORTS = ["zg_g2_is_on_curve_batch", "zg_g2_affine_add_batch", "zg_g2_scalar_mul_batch", "zg_g2_fixed_base_mul_batch", "zg_g2_axpy_batch",
              "zg_g1_axpy_batch", "zg_msm_g2", "zg_msm_g2_dev"]


def test_generator_is_on_the_twist_and_has_order_r():
    assert M.B_TWIST == (27 * pow(82, -1, M.P) % M.P, -3 * pow(82, -1, M.P) % M.P)  # 3 / (9 + u) = (27 - 3u) / 82
    assert M.is_on_curve(M.G) and M.is_on_curve(None)
    assert not M.is_on_curve((M.G[0], M.f2_add(M.G[1], (1, 0))))
    assert M.scalar_mul(M.G, M.R) is None
    assert M.scalar_mul(M.G, M.R - 1) == M.neg(M.G)
    assert M.add(M.G, M.neg(M.G)) is None and M.add(None, M.G) == M.G and M.add(M.G, None) == M.G and M.add(None, None) is None
    assert M.add(M.G, M.G) == M.double(M.G) == M.scalar_mul(M.G, 2)
    assert M.double(None) is None and M.scalar_mul(None, 5) is None and M.scalar_mul(M.G, 0) is None


def test_fp2_field_laws():
    rng = random.Random(11)
    for _ in range(20):
        a, b, c = [(rng.randrange(M.P), rng.randrange(M.P)) for _ in range(3)]
        assert M.f2_mul(a, M.f2_add(b, c)) == M.f2_add(M.f2_mul(a, b), M.f2_mul(a, c))
        assert M.f2_mul(a, M.f2_inv(a)) == (1, 0)
        assert M.f2_sqr(a) == ((a[0] + a[1]) * (a[0] - a[1]) % M.P, 2 * a[0] * a[1] % M.P)
    assert M.f2_sqr((0, 1)) == (M.P - 1, 0) and M.f2_inv((0, 0)) == (0, 0)


def test_group_laws_and_the_jacobian_ladder_against_the_affine_one():
    rng = random.Random(12)
    a, b = rng.randrange(M.R), rng.randrange(M.R)
    aG, bG = M.scalar_mul(M.G, a), M.scalar_mul(M.G, b)
    assert M.is_on_curve(aG) and M.is_on_curve(bG)
    assert M.scalar_mul(aG, b) == M.scalar_mul(M.G, a * b % M.R)
    assert M.add(aG, bG) == M.scalar_mul(M.G, (a + b) % M.R)
    for s in (1, 2, 3, 5, 255, 256, (1 << 64) - 1, 1 << 200, a, b, M.R - 1, M.R - 2):
        assert M.scalar_mul(M.G, s) == M.scalar_mul_affine(M.G, s), s
    assert M.scalar_mul(aG, 7) == M.scalar_mul_affine(aG, 7)
    pts = [M.scalar_mul(M.G, k) for k in (3, 5, 9)]
    assert M.msm(pts, [2, 4, 6]) == M.scalar_mul(M.G, 3 * 2 + 5 * 4 + 9 * 6)
    assert M.msm(pts + [None], [0, 0, 0, 9]) is None


def test_compress_g2_of_small_multiples():
    """compressG2 (dory.zig:179-210): x.c0 then x.c1 as little-endian integers, the sign of y in bit 7 of the last byte (c1 compared first,
    fp2IsPositive :320-344), the identity as 0x40 there; P and -P differ in that bit only"""
    assert M.compress(None) == bytes(63) + b"\x40"
    for k in range(1, 6):
        p = M.scalar_mul(M.G, k)
        c, cn = M.compress(p), M.compress(M.neg(p))
        assert int.from_bytes(c[:32], "little") == p[0][0]
        assert int.from_bytes(c[32:63] + bytes([c[63] & 0x3F]), "little") == p[0][1]
        assert c[:63] == cn[:63] and (c[63] ^ cn[63]) == 0x80
        ny = M.f2_neg(p[1])
        assert (c[63] & 0xC0 == 0) == ((p[1][1], p[1][0]) <= (ny[1], ny[0]))
    assert M.compress(M.G)[:8] == bytes.fromhex("edf692d95cbdde46")  # the generator's x0 bytes (pairing.zig:781-786)


def test_packing_round_trips_and_identity_layout():
    pts = [M.G, None, M.scalar_mul(M.G, 77)]
    xy, inf = M.pack(pts)
    assert xy.shape == (3, 16) and list(inf) == [0, 1, 0]
    assert M.unpack(xy, inf) == pts
    one = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]  # Fp.one() in Montgomery form
    assert list(xy[1]) == [0] * 8 + one + [0] * 4  # G2Point.identity(): x = 0, y = (one, 0)
    assert M.fr_unpack(M.fr_pack([0, 1, M.R - 1, 12345])) == [0, 1, M.R - 1, 12345]
    assert M.f2_unpack(M.f2_pack([(3, M.P - 1)])) == [(3, M.P - 1)]
    from oracle import pymodel as pm  # the existing model's Montgomery convention is the same one
    assert list(M.fr_pack([987654321])[0]) == list(pm.limbs(pm.to_mont(987654321, pm.R_MOD)))


def test_abi_carries_the_g2_section():
    from zolt_amd import _abi, lib
    assert _abi.ZG_ABI_MINOR == 11 and _abi.ZG_FEATURE_G2 == 8
    for name in G2_EXPORTS:
        assert name in _abi.PROTOS, name
        assert hasattr(lib._lib, name)
    hdr = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "G2 (Dory)" in hdr and re.search(r"#define ZG_FEATURE_G2 8u", hdr)
    assert _abi.ZG_OP_FP2_MUL == 14 and _abi.ZG_OP_FP2_INV == 16 and "ZG_OP_FP2" not in hdr  # self-test hooks stay in the internal header
    for fn in ("g2_is_on_curve_batch", "g2_affine_add_batch", "g2_scalar_mul_batch", "g2_fixed_base_mul_batch", "g2_axpy_batch", "g1_axpy_batch",
               "msm_g2", "msm_g2_dev"):
        assert callable(getattr(lib, fn)), fn
    assert np.dtype(np.uint64).itemsize * 16 == 128  # one affine G2 point
