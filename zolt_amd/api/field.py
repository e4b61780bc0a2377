"""field.py — zolt.field: BatchOps (src/field/mod.zig:1164-1280) over the device.

Part of the zolt_amd.api package (the host mirror of the reference's module API over libzolt_gpu.so); import zolt_amd.api,
which re-exports every name of every part."""
import numpy as np

from .. import lib
from ._base import *  # noqa: F401,F403


def _vec(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def _same_len(a, b):
    a, b = _vec(a), _vec(b)
    assert a.shape == b.shape  # std.debug.assert(a.len == b.len)
    return a, b


class BatchOps:
    """BatchOps with the reference's names; the reference's `results` slice is the return value. Vectors are (n, 4) uint64 Montgomery limbs
    on the host; `field` is lib.FR (the reference's BN254Scalar) or lib.FP. A table that already lives in HBM goes through the _dev
    wrappers of zolt_amd.lib instead (field_op_dev, field_scale_dev, field_batch_inverse_dev, field_inner_product_dev, field_horner_dev)."""

    @staticmethod
    def batchAdd(a, b, field=lib.FR):
        """:1166-1171"""
        return lib.field_op(field, lib.OP_ADD, *_same_len(a, b))

    @staticmethod
    def batchSub(a, b, field=lib.FR):
        """:1174-1179"""
        return lib.field_op(field, lib.OP_SUB, *_same_len(a, b))

    @staticmethod
    def batchMul(a, b, field=lib.FR):
        """:1182-1187"""
        return lib.field_op(field, lib.OP_MUL, *_same_len(a, b))

    @staticmethod
    def batchMulScalar(a, scalar, field=lib.FR):
        """:1190-1195, on the device from end to end: the scalar travels with the launch"""
        a = _vec(a)
        if a.shape[0] == 0:
            return a.copy()
        buf = lib.DeviceBuffer.from_host(a)
        try:
            lib.field_scale_dev(field, buf.ptr, a.shape[0], scalar, buf.ptr)
            lib.sync()
            return buf.to_host().reshape(-1, 4)
        finally:
            buf.free()

    @staticmethod
    def batchSquare(a, field=lib.FR):
        """:1198-1203"""
        return lib.field_op(field, lib.OP_SQR, _vec(a))

    @staticmethod
    def innerProduct(a, b, field=lib.FR):
        """:1206-1213"""
        return lib.field_inner_product(field, *_same_len(a, b))

    @staticmethod
    def hornerEval(coeffs, x, field=lib.FR):
        """:1217-1227: coeffs[0] + x (coeffs[1] + x (...)); zero for no coefficients"""
        return lib.field_horner(field, _vec(coeffs), x)

    @staticmethod
    def batchInverse(a, field=lib.FR):
        """:1232-1273, Montgomery's trick. Element-wise: zero only where the input is zero — the reference zeroes EVERY output when a[0] is
        zero (its :1241 seeds the running product without the zero guard); on any other input the two agree (include/zolt_gpu.h)."""
        return lib.field_batch_inverse(field, _vec(a))

    @staticmethod
    def multiScalarMulLinear(scalars, bases, field=lib.FR):
        """:1277-1279"""
        return BatchOps.innerProduct(scalars, bases, field)


__all__ = [_k for _k in dir() if not _k.startswith("__")]  # underscore helpers are shared between the parts too
