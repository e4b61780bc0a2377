"""ctypes binding of include/zolt_gpu.h. Arrays are numpy uint64 (host) or raw device
pointers (ints, e.g. torch.Tensor.data_ptr()). No torch import here."""
import contextlib as _contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZOLT_GPU_LIB: load another build of the same library (A/B experiments on kernel variants); never a fallback
LIB_PATH = os.environ.get("ZOLT_GPU_LIB") or os.path.join(_HERE, "libzolt_gpu.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C zolt_amd/csrc` (or __graft_entry__.build()). "
        "zolt_amd has no CPU fallback."
    )
_lib = C.CDLL(LIB_PATH)

OK, ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_NO_DEVICE, ERR_VERIFY = 0, 1, 2, 3, 4, 5
FR, FP = 0, 1
OP_MUL, OP_ADD, OP_SUB, OP_NEG, OP_SQR, OP_INV, OP_FROM_MONT, OP_TO_MONT = range(8)
# self-test hooks (include/zolt_gpu_internal.h)
OP_MUL29, OP_SQR29, OP_X3_29, OP_INV_XGCD, OP_INV_SAFEGCD = 9, 10, 11, 12, 13
OP_FP2_MUL, OP_FP2_SQR, OP_FP2_INV = 14, 15, 16  # Fp2 self-test hooks: consecutive element pairs are (c0, c1)
# Fp12 self-test hooks: 12 consecutive elements are one Fp12 in the order of a GT element (csrc/fp12.hip.h)
OP_FP12_MUL, OP_FP12_SQR, OP_FP12_INV, OP_FP12_CONJ, OP_FP12_FROB1, OP_FP12_FROB2, OP_FP12_FROB3, OP_FP12_EXP_X = range(17, 25)
# the same through the wave pairing engine's tower (csrc/fp12_wave.hip.h); MUL_034: the first three Fp2 of each element of b are c0, c3, c4
(OP_FP12W_MUL, OP_FP12W_SQR, OP_FP12W_INV, OP_FP12W_CONJ, OP_FP12W_FROB1, OP_FP12W_FROB2, OP_FP12W_FROB3, OP_FP12W_EXP_X,
 OP_FP12W_MUL_034) = range(40, 49)
OP_DORY_V1, OP_DORY_V2, OP_DORY_S1, OP_DORY_S2 = 32, 33, 34, 35  # the state of a Dory opening session (a = one word holding the handle)
SC_HIGH_HALF, SC_LOW_PAIR = 0, 1

# every symbol include/zolt_gpu.h declares, with its ctypes signature: GENERATED from the header (tools/gen_bindings.py -> _abi.py), so the
# binding cannot drift from the C ABI; apply() fails with AttributeError if the loaded library lacks one of them
from . import _abi  # noqa: E402

SYMBOLS = _abi.SYMBOLS
# test / bench scaffolding of include/zolt_gpu_internal.h (not part of the drop-in boundary)
INTERNAL_SYMBOLS = _abi.INTERNAL_SYMBOLS
_abi.apply(_lib)
if _lib.zg_abi_version() >> 16 != _abi.ZG_ABI_MAJOR:
    raise ImportError(f"{LIB_PATH}: ABI major {_lib.zg_abi_version() >> 16}, this binding was generated for {_abi.ZG_ABI_MAJOR}")


class MsmConfig(C.Structure):
    _fields_ = [("window_bits", C.c_int), ("precompute_levels", C.c_int), ("expected_uses", C.c_int)]



_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)


class ZgError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = _lib.zg_last_error()
        super().__init__(f"{where}: error {code}: {msg.decode() if msg else ''}")


def _chk(rc, where):
    if rc != OK:
        raise ZgError(rc, where)


def _h(a):
    """host numpy array -> uint64* (None passes NULL)"""
    return None if a is None else a.ctypes.data_as(_u64p)


def _hb(a):
    return None if a is None else a.ctypes.data_as(_u8p)


def _d(ptr):
    """device address (int) -> void*"""
    return C.c_void_p(int(ptr) if ptr else None)


def _c(a, dtype=np.uint64):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def version():
    return _lib.zg_version().decode()


def device_count():
    return int(_lib.zg_device_count())


def init(device=-1):
    _chk(_lib.zg_init(C.c_int(device)), "zg_init")


def init_devices(n=0):
    """one process, several GPUs (devices 0..n-1; n <= 0: all visible)"""
    _chk(_lib.zg_init_devices(C.c_int(n)), "zg_init_devices")


def n_devices():
    return int(_lib.zg_n_devices())


def shutdown():
    _lib.zg_shutdown()


import atexit as _atexit  # noqa: E402

_atexit.register(lambda: _lib.zg_shutdown())  # communicators and the runtime's idle resources are released while HIP and RCCL are still alive


def abi_version():
    """(major, minor) of the loaded library's C ABI"""
    v = int(_lib.zg_abi_version())
    return v >> 16, v & 0xFFFF


def abi_features():
    return int(_lib.zg_abi_features())


def dev_trim():
    """return the device pool's idle blocks to the driver"""
    _chk(_lib.zg_dev_trim(), "zg_dev_trim")


def sync():
    _chk(_lib.zg_sync(), "zg_sync")


def last_error():
    m = _lib.zg_last_error()
    return m.decode() if m else ""


class DeviceBuffer:
    """Raw device memory through the C ABI itself (zg_dev_alloc / zg_memcpy_*): what a host without its own HIP binding uses
    (the Zig shim), and what keeps this module free of torch."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _chk(_lib.zg_dev_alloc(C.c_size_t(nbytes), C.byref(p)), "zg_dev_alloc")
        self.ptr, self.nbytes = p.value, nbytes

    @classmethod
    def from_host(cls, arr):
        a = np.ascontiguousarray(arr)
        b = cls(max(a.nbytes, 1))
        if a.nbytes:
            _chk(_lib.zg_memcpy_h2d(C.c_void_p(b.ptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)), "zg_memcpy_h2d")
        return b

    def to_host(self, dtype=np.uint64):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _chk(_lib.zg_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(out.nbytes)), "zg_memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            _chk(_lib.zg_dev_free(C.c_void_p(self.ptr)), "zg_dev_free")
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PROF_NAMES = ["msm_digits", "msm_sort", "msm_accumulate", "msm_reduce", "eq_table", "sc_fold", "sc_sums", "combine"]


def profile_begin(max_records=4096):
    _chk(_lib.zg_profile_begin(C.c_int(max_records)), "zg_profile_begin")


def profile_end():
    """-> {kernel name: (total ms, launches)} measured with HIP events on the launch stream"""
    ms = (C.c_double * len(PROF_NAMES))()
    cnt = (C.c_uint64 * len(PROF_NAMES))()
    _chk(_lib.zg_profile_end(ms, cnt), "zg_profile_end")
    return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(PROF_NAMES)}


# ---- field vectors
def field_op(field, op, a, b=None):
    a = _c(a)
    b = _c(b)
    out = np.empty_like(a)
    _chk(_lib.zg_field_op(C.c_int(field), C.c_int(op), _h(a), _h(b), _h(out), C.c_size_t(a.size // 4)), "zg_field_op")
    return out


# ---- field vectors (device): field.BatchOps on resident tables (zolt_gpu.h). The _dev forms take device addresses and an element count
FV_E, FV_TILE = _abi.ZG_FV_E, _abi.ZG_FV_TILE  # elements per lane / per workgroup of the batch inverse and of Horner's rule


def field_op_dev(field, op, d_a, d_b, d_out, n, stream=0):
    _chk(_lib.zg_field_op_dev(C.c_int(field), C.c_int(op), _d(d_a), _d(d_b), _d(d_out), C.c_size_t(n), _d(stream)), "zg_field_op_dev")


def field_scale_dev(field, d_a, n, s, d_out, stream=0):
    _chk(_lib.zg_field_scale_dev(C.c_int(field), _d(d_a), C.c_size_t(n), _h(_c(s)), _d(d_out), _d(stream)), "zg_field_scale_dev")


def field_batch_inverse(field, a):
    a = _c(a)
    out = np.empty_like(a)
    _chk(_lib.zg_field_batch_inverse(C.c_int(field), _h(a), _h(out), C.c_size_t(a.size // 4)), "zg_field_batch_inverse")
    return out


def field_batch_inverse_dev(field, d_a, d_out, n, stream=0):
    _chk(_lib.zg_field_batch_inverse_dev(C.c_int(field), _d(d_a), _d(d_out), C.c_size_t(n), _d(stream)), "zg_field_batch_inverse_dev")


def field_inner_product(field, a, b):
    a, b = _c(a), _c(b)
    if a.size != b.size:
        raise ValueError("field_inner_product: vectors of different lengths")
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_field_inner_product(C.c_int(field), _h(a), _h(b), C.c_size_t(a.size // 4), _h(out)), "zg_field_inner_product")
    return out


def field_inner_product_dev(field, d_a, d_b, n, stream=0):
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_field_inner_product_dev(C.c_int(field), _d(d_a), _d(d_b), C.c_size_t(n), _d(stream), _h(out)), "zg_field_inner_product_dev")
    return out


def field_horner(field, coeffs, x):
    coeffs = _c(coeffs)
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_field_horner(C.c_int(field), _h(coeffs), C.c_size_t(coeffs.size // 4), _h(_c(x)), _h(out)), "zg_field_horner")
    return out


def field_horner_dev(field, d_coeffs, n, x, stream=0):
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_field_horner_dev(C.c_int(field), _d(d_coeffs), C.c_size_t(n), _h(_c(x)), _d(stream), _h(out)), "zg_field_horner_dev")
    return out


def fr_dense_evaluate_dev(d_evals, point, stream=0):
    point = _c(point)
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_fr_dense_evaluate_dev(_d(d_evals), C.c_size_t(point.size // 4), _h(point), _d(stream), _h(out)), "zg_fr_dense_evaluate_dev")
    return out


def selftest_lazy_g1(op, records):
    """zg_selftest_lazy_g1 (include/zolt_gpu_internal.h): the MSM's lazy-limb field forms and group law on raw limbs.
    records: (n, 91) uint32 -> (n, 146) uint32; the layout is csrc/lazy_selftest.hip.h, the model and checker tests/lazy_model.py"""
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 91)
    out = np.empty((rec.shape[0], 146), dtype=np.uint32)
    _chk(_lib.zg_selftest_lazy_g1(C.c_int(op), rec.ctypes.data_as(C.c_void_p), C.c_size_t(rec.shape[0]), out.ctypes.data_as(C.c_void_p)),
         "zg_selftest_lazy_g1")
    return out


def selftest_lazy_fr(op, records, threads=0):
    """zg_selftest_lazy_fr (include/zolt_gpu_internal.h): the sumcheck kernels' lazy Fr arithmetic and 288-bit sums on raw limbs.
    threads == 0: records (n, 146) uint32 -> (n, 146) uint32. Op 8 (the block reduction): records (n, threads, 18) -> (n, 16).
    The layout is csrc/lazy_fr_selftest.hip.h, the model and checker tests/lazy_fr_model.py"""
    rec = np.ascontiguousarray(records, dtype=np.uint32)
    rec = rec.reshape(-1, threads, 18) if threads else rec.reshape(-1, 146)
    out = np.empty((rec.shape[0], 16 if threads else 146), dtype=np.uint32)
    _chk(_lib.zg_selftest_lazy_fr(C.c_int(op), rec.ctypes.data_as(C.c_void_p), C.c_size_t(rec.shape[0]), out.ctypes.data_as(C.c_void_p), C.c_int(threads)),
         "zg_selftest_lazy_fr")
    return out


def selftest_xyzz(group, op, records):
    """zg_selftest_xyzz (include/zolt_gpu_internal.h): the canonical XYZZ group law on raw coordinates, group 0 = G1 (Fp), 1 = G2 (Fp2).
    records: (n, 8 W + 6) uint64 -> (n, 4 W + 2) uint64 with W = 4 or 8; the layout is csrc/xyzz_selftest.hip.h, the model and checker
    tests/xyzz_model.py"""
    w = 8 if group == 1 else 4
    rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 8 * w + 6)
    out = np.empty((rec.shape[0], 4 * w + 2), dtype=np.uint64)
    _chk(_lib.zg_selftest_xyzz(C.c_int(group), C.c_int(op), rec.ctypes.data_as(C.c_void_p), C.c_size_t(rec.shape[0]), out.ctypes.data_as(C.c_void_p)),
         "zg_selftest_xyzz")
    return out


def selftest_small_msm(group, jobs):
    """zg_selftest_small_msm (include/zolt_gpu_internal.h): one launch set of csrc/small_msm.hip.h over G1 (group 0) or G2 (group 1).
    jobs: 1..4 tuples (xy (n, 8 or 16) uint64, inf (n,) uint8 or None, scalars (n, 4) uint64 Montgomery), of any lengths, 0 included
    -> [(xy (8 or 16,) uint64, identity flag)] per job"""
    w = 16 if group == 1 else 8
    xs = [np.ascontiguousarray(j[0], dtype=np.uint64).reshape(-1, w) for j in jobs]
    fs = [None if j[1] is None else np.ascontiguousarray(j[1], dtype=np.uint8).reshape(-1) for j in jobs]
    ss = [np.ascontiguousarray(j[2], dtype=np.uint64).reshape(-1, 4) for j in jobs]
    assert all(len(x) == len(s) and (f is None or len(f) == len(x)) for x, f, s in zip(xs, fs, ss))
    k = len(jobs)
    n = (C.c_size_t * k)(*[len(x) for x in xs])
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    xy = (C.c_void_p * k)(*[ptr(x) for x in xs])
    inf = (C.c_void_p * k)(*[ptr(f) for f in fs])
    sc = (C.c_void_p * k)(*[ptr(s) for s in ss])
    out = np.zeros((k, w + 1), dtype=np.uint64)
    _chk(_lib.zg_selftest_small_msm(C.c_int(group), C.c_int(k), n, xy, inf, sc, out.ctypes.data_as(C.c_void_p)), "zg_selftest_small_msm")
    return [(out[j, :w].copy(), int(out[j, w])) for j in range(k)]


(SHAPE_EQ_TABLE, SHAPE_EQ_SPARTAN, SHAPE_SC_FOLD, SHAPE_SC_SUMS, SHAPE_SC_PAIRSUM, SHAPE_FB, SHAPE_RRW, SHAPE_PSC, SHAPE_HK_FOLD) = (
    _abi.ZG_SHAPE_EQ_TABLE, _abi.ZG_SHAPE_EQ_SPARTAN, _abi.ZG_SHAPE_SC_FOLD, _abi.ZG_SHAPE_SC_SUMS, _abi.ZG_SHAPE_SC_PAIRSUM, _abi.ZG_SHAPE_FB,
    _abi.ZG_SHAPE_RRW, _abi.ZG_SHAPE_PSC, _abi.ZG_SHAPE_HK_FOLD)


def launch_shape(family, a, b=0):
    """zg_selftest_launch_shape (include/zolt_gpu_internal.h): the four words the library's own shape functions give for a kernel family
    (SHAPE_*) at a size, under this process's switches; nothing is launched"""
    out = (C.c_uint32 * 4)()
    _chk(_lib.zg_selftest_launch_shape(C.c_int(family), C.c_size_t(a), C.c_size_t(b), out), "zg_selftest_launch_shape")
    return tuple(int(x) for x in out)


# ---- bases / MSM
class Bases:
    """Device-resident bases (the SRS). Mirrors HyperKZG SetupParams.powers_of_tau_g1."""

    def __init__(self, handle, n):
        self._h = handle
        self.n = n

    @classmethod
    def upload(cls, xy, inf=None, window_bits=0, precompute_levels=0, expected_uses=0):
        xy = _c(xy)
        inf = _c(inf, np.uint8)
        n = xy.size // 8
        cfg = MsmConfig(window_bits, precompute_levels, expected_uses)
        h = C.c_void_p()
        _chk(_lib.zg_g1_bases_upload(_h(xy), _hb(inf), C.c_size_t(n), C.byref(cfg), C.byref(h)), "zg_g1_bases_upload")
        return cls(h, n)

    @classmethod
    def upload_dev(cls, d_xy, d_inf, n, stream=0, window_bits=0, precompute_levels=0):
        cfg = MsmConfig(window_bits, precompute_levels, 0)
        h = C.c_void_p()
        _chk(_lib.zg_g1_bases_upload_dev(_d(d_xy), _d(d_inf), C.c_size_t(n), C.byref(cfg), _d(stream), C.byref(h)),
             "zg_g1_bases_upload_dev")
        return cls(h, n)

    def msm_u64(self, values, n=None, off=0):
        """MSM over scalars given as u64 machine words (zg_msm_g1_u64): = msm(F.fromU64 of every word)"""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        n = v.size if n is None else n
        out = np.empty(8, dtype=np.uint64)
        inf = C.c_uint8(0)
        _chk(_lib.zg_msm_g1_u64(self._h, C.c_size_t(off), C.c_size_t(n), _h(v), _h(out), C.byref(inf)), "zg_msm_g1_u64")
        return out, int(inf.value)

    @classmethod
    def hyperkzg_setup(cls, base_xy, tau, n, want_points=True, window_bits=0, precompute_levels=0, expected_uses=0):
        """HyperKZG.setup's G1 side on the device (zg_hyperkzg_setup): -> (handle, points xy (n, 8) or None, inf (n,) or None)"""
        cfg = MsmConfig(window_bits, precompute_levels, expected_uses)
        xy = np.empty((n, 8), dtype=np.uint64) if want_points else None
        inf = np.zeros(n, dtype=np.uint8) if want_points else None
        h = C.c_void_p()
        _chk(_lib.zg_hyperkzg_setup(_h(_c(base_xy)), _h(_c(tau)), C.c_size_t(n), C.byref(cfg), _h(xy), _hb(inf), C.byref(h)), "zg_hyperkzg_setup")
        return cls(h, n), xy, inf

    def table_bytes(self):
        """bytes of HBM held for the bases: the table of precomputed multiples (levels x 64 B per base), or the plain bases"""
        return int(_lib.zg_g1_bases_table_bytes(self._h))

    def plan(self):
        """(window bits c, windows per scalar, table levels per base) the handle was built with"""
        c, w, l = C.c_int(), C.c_int(), C.c_int()
        _chk(_lib.zg_g1_bases_plan(self._h, C.byref(c), C.byref(w), C.byref(l)), "zg_g1_bases_plan")
        return c.value, w.value, l.value

    def free(self):
        if self._h:
            _chk(_lib.zg_g1_bases_free(self._h), "zg_g1_bases_free")
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def msm(self, scalars, off=0, n=None):
        scalars = _c(scalars)
        n = scalars.size // 4 if n is None else n
        out = np.empty(8, dtype=np.uint64)
        inf = C.c_uint8(0)
        _chk(_lib.zg_msm_g1(self._h, C.c_size_t(off), C.c_size_t(n), _h(scalars), _h(out), C.byref(inf)), "zg_msm_g1")
        return out, int(inf.value)

    def msm_dev(self, d_scalars, n, off=0, stream=0):
        out = np.empty(8, dtype=np.uint64)
        inf = C.c_uint8(0)
        _chk(_lib.zg_msm_g1_dev(self._h, C.c_size_t(off), C.c_size_t(n), _d(d_scalars), _d(stream), _h(out), C.byref(inf)),
             "zg_msm_g1_dev")
        return out, int(inf.value)

    def msm_dev_async(self, d_scalars, n, d_out_xy, d_out_inf, off=0, stream=0):
        _chk(_lib.zg_msm_g1_dev_async(self._h, C.c_size_t(off), C.c_size_t(n), _d(d_scalars), _d(stream), _d(d_out_xy),
                                      _d(d_out_inf)), "zg_msm_g1_dev_async")

    def msm_partial_dev(self, d_scalars, n, d_out_jac, off=0, stream=0):
        _chk(_lib.zg_msm_g1_partial_dev(self._h, C.c_size_t(off), C.c_size_t(n), _d(d_scalars), _d(stream), _d(d_out_jac)),
             "zg_msm_g1_partial_dev")

    def msm_partial_fast_dev(self, d_scalars, n, d_out_jac, off=0, stream=0):
        _chk(_lib.zg_msm_g1_partial_fast_dev(self._h, C.c_size_t(off), C.c_size_t(n), _d(d_scalars), _d(stream), _d(d_out_jac)),
             "zg_msm_g1_partial_fast_dev")

    def msm_batch_dev(self, d_scalars, n, k, d_out9, stream=0):
        """k vectors of n scalars back to back in HBM -> k records of 9 u64 (xy[8] + flag word) in HBM, asynchronous."""
        _chk(_lib.zg_msm_g1_batch_dev(self._h, C.c_size_t(n), _d(d_scalars), C.c_size_t(k), _d(stream), _d(d_out9)), "zg_msm_g1_batch_dev")

    def msm_batch(self, batches, n=None):
        batches = [_c(b) for b in batches]
        k = len(batches)
        n = (batches[0].size // 4 if k else 0) if n is None else n
        arr = (_u64p * max(k, 1))(*[_h(b) for b in batches])
        out = np.empty((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _chk(_lib.zg_msm_g1_batch(self._h, C.c_size_t(n), arr, C.c_size_t(k), _h(out), _hb(inf)), "zg_msm_g1_batch")
        return out, inf


def pool_debug_stats():
    """ZG_POOL_DEBUG counters (include/zolt_gpu_internal.h): {'mode', 'hits', 'suspect_frees', 'blocks_verified', 'bytes_poisoned'}"""
    out = np.zeros(4, dtype=np.uint64)
    mode = int(_lib.zg_pool_debug_stats(_h(out)))
    return {"mode": mode, "hits": int(out[0]), "suspect_frees": int(out[1]), "blocks_verified": int(out[2]), "bytes_poisoned": int(out[3])}


def pool_debug_selftest():
    """breaks the pool's contract on purpose: 1 = ZG_POOL_DEBUG caught it, 0 = mode off; raises on an error"""
    rc = int(_lib.zg_pool_debug_selftest())
    if rc < 0:
        raise ZgError(-rc, "zg_pool_debug_selftest")
    return rc


def sharded_comm_sets_created():
    """test hook (include/zolt_gpu_internal.h): RCCL communicator sets created so far by the one-process multi-GPU path"""
    return int(_lib.zg_sharded_comm_sets_created())


def shard_bounds(n, shards, shard):
    """ParallelMSM's chunk `shard` of `shards` over n points -> (start, len); host arithmetic only (works without a GPU)"""
    st, ln = C.c_size_t(), C.c_size_t()
    _chk(_lib.zg_shard_bounds(C.c_size_t(n), C.c_int(shards), C.c_int(shard), C.byref(st), C.byref(ln)), "zg_shard_bounds")
    return st.value, ln.value


class ShardedBases:
    """The SRS sharded over the devices bound by init_devices (ParallelMSM's contiguous chunks, src/msm/mod.zig:609)."""
    EXCHANGE = {0: "none", 1: "rccl", 2: "p2p"}

    def __init__(self, handle, n):
        self._h = handle
        self.n = n

    @classmethod
    def upload(cls, xy, inf=None, window_bits=0, precompute_levels=0):
        xy = _c(xy)
        inf = _c(inf, np.uint8)
        n = xy.size // 8
        cfg = MsmConfig(window_bits, precompute_levels, 0)
        h = C.c_void_p()
        _chk(_lib.zg_g1_bases_upload_sharded(_h(xy), _hb(inf), C.c_size_t(n), C.byref(cfg), C.byref(h)), "zg_g1_bases_upload_sharded")
        return cls(h, n)

    def shards(self):
        """[(device, start, len)] per shard"""
        out = []
        for i in range(int(_lib.zg_g1_sbases_shards(self._h))):
            d, st, ln = C.c_int(), C.c_size_t(), C.c_size_t()
            _chk(_lib.zg_g1_sbases_shard(self._h, C.c_int(i), C.byref(d), C.byref(st), C.byref(ln)), "zg_g1_sbases_shard")
            out.append((d.value, st.value, ln.value))
        return out

    def exchange(self):
        return self.EXCHANGE[int(_lib.zg_g1_sbases_exchange(self._h))]

    def msm(self, scalars, n=None):
        scalars = _c(scalars)
        n = scalars.size // 4 if n is None else n
        out = np.empty(8, dtype=np.uint64)
        inf = C.c_uint8(0)
        _chk(_lib.zg_msm_g1_sharded(self._h, C.c_size_t(n), _h(scalars), _h(out), C.byref(inf)), "zg_msm_g1_sharded")
        return out, int(inf.value)

    def msm_dev(self, d_scalars_per_shard, n):
        arr = (C.c_void_p * len(d_scalars_per_shard))(*[int(p) if p else None for p in d_scalars_per_shard])
        out = np.empty(8, dtype=np.uint64)
        inf = C.c_uint8(0)
        _chk(_lib.zg_msm_g1_sharded_dev(self._h, C.c_size_t(n), arr, _h(out), C.byref(inf)), "zg_msm_g1_sharded_dev")
        return out, int(inf.value)

    def msm_batch(self, batches, n=None):
        batches = [_c(b) for b in batches]
        k = len(batches)
        n = (batches[0].size // 4 if k else 0) if n is None else n
        arr = (_u64p * max(k, 1))(*[_h(b) for b in batches])
        out = np.empty((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _chk(_lib.zg_msm_g1_batch_sharded(self._h, C.c_size_t(n), arr, C.c_size_t(k), _h(out), _hb(inf)), "zg_msm_g1_batch_sharded")
        return out, inf

    def inflight(self):
        """sharded calls the handle keeps in flight (its slots)"""
        return int(_lib.zg_g1_sbases_inflight(self._h))

    def msm_dev_async(self, d_scalars_per_shard, n, ready_streams=None):
        """-> ticket; the result comes from wait(ticket). ready_streams: per shard the stream whose work fills its scalars (or None)"""
        arr = (C.c_void_p * len(d_scalars_per_shard))(*[int(p) if p else None for p in d_scalars_per_shard])
        rs = None
        if ready_streams is not None:
            rs = (C.c_void_p * len(ready_streams))(*[int(p) if p else None for p in ready_streams])
        t = C.c_uint64(0)
        _chk(_lib.zg_msm_g1_sharded_dev_async(self._h, C.c_size_t(n), arr, rs, C.byref(t)), "zg_msm_g1_sharded_dev_async")
        return int(t.value)

    def msm_batch_async(self, batches, n=None):
        """-> (ticket, k, keepalive); the host vectors must stay alive until wait(ticket)"""
        batches = [_c(b) for b in batches]
        k = len(batches)
        n = (batches[0].size // 4 if k else 0) if n is None else n
        arr = (_u64p * max(k, 1))(*[_h(b) for b in batches])
        t = C.c_uint64(0)
        _chk(_lib.zg_msm_g1_batch_sharded_async(self._h, C.c_size_t(n), arr, C.c_size_t(k), C.byref(t)), "zg_msm_g1_batch_sharded_async")
        return int(t.value), k, batches

    def wait(self, ticket, k=1):
        out = np.empty((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _chk(_lib.zg_sharded_wait(self._h, C.c_uint64(ticket), _h(out), _hb(inf)), "zg_sharded_wait")
        return out, inf

    def free(self):
        if self._h:
            _chk(_lib.zg_g1_sbases_free(self._h), "zg_g1_sbases_free")
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def g1_affine_add_batch(a_xy, a_inf, b_xy, b_inf):
    """AffinePoint.add per pair (src/msm/mod.zig:74-103) -> (xy (n,8), inf (n,))"""
    a_xy, b_xy = _c(a_xy), _c(b_xy)
    a_inf, b_inf = _c(a_inf, np.uint8), _c(b_inf, np.uint8)
    n = a_xy.size // 8
    out = np.empty((n, 8), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g1_affine_add_batch(_h(a_xy), _hb(a_inf), _h(b_xy), _hb(b_inf), C.c_size_t(n), _h(out), _hb(oinf)), "zg_g1_affine_add_batch")
    return out, oinf


def fr_scale(a, s):
    a = _c(a)
    out = np.empty_like(a)
    _chk(_lib.zg_fr_scale(_h(a), C.c_size_t(a.size // 4), _h(_c(s)), _h(out)), "zg_fr_scale")
    return out


def combine_partials_dev(d_partials, k, stream=0):
    out = np.empty(8, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(_lib.zg_g1_combine_partials_dev(_d(d_partials), C.c_size_t(k), _d(stream), _h(out), C.byref(inf)),
         "zg_g1_combine_partials_dev")
    return out, int(inf.value)


def combine_partials_dev_async(d_partials, k, d_out_xy, d_out_inf, stream=0):
    _chk(_lib.zg_g1_combine_partials_dev_async(_d(d_partials), C.c_size_t(k), _d(stream), _d(d_out_xy), _d(d_out_inf)),
         "zg_g1_combine_partials_dev_async")


def combine_partials_batch_dev_async(d_partials, ranks, rank_stride, m, d_out9, stream=0):
    """m results behind one exchange: rank r's m records at d_partials + r * rank_stride words; result j at d_out9 + 9 j"""
    _chk(_lib.zg_g1_combine_partials_batch_dev_async(_d(d_partials), C.c_size_t(ranks), C.c_size_t(rank_stride), C.c_size_t(m), _d(stream),
                                                     _d(d_out9)), "zg_g1_combine_partials_batch_dev_async")


def g1_scalar_mul_batch(xy, inf, scalars):
    xy, inf, scalars = _c(xy), _c(inf, np.uint8), _c(scalars)
    n = scalars.size // 4
    out = np.empty((n, 8), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g1_scalar_mul_batch(_h(xy), _hb(inf), _h(scalars), C.c_size_t(n), _h(out), _hb(oinf)), "zg_g1_scalar_mul_batch")
    return out, oinf


def g1_fixed_base_mul_batch(base_xy, scalars, base_inf=0):
    """scalars[i] * base for one shared base (HyperKZG.setup) -> (xy (n,8), inf (n,))"""
    base_xy, scalars = _c(base_xy), _c(scalars)
    n = scalars.size // 4
    out = np.empty((n, 8), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g1_fixed_base_mul_batch(_h(base_xy), C.c_uint8(base_inf), _h(scalars), C.c_size_t(n), _h(out), _hb(oinf)),
         "zg_g1_fixed_base_mul_batch")
    return out, oinf


def g1_is_on_curve_batch(xy, inf=None):
    xy, inf = _c(xy), _c(inf, np.uint8)
    n = xy.size // 8
    out = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g1_is_on_curve_batch(_h(xy), _hb(inf), C.c_size_t(n), _hb(out)), "zg_g1_is_on_curve_batch")
    return out


def _g2_pairs(fn, where, words, a_xy, a_inf, b_xy, b_inf, extra=()):
    a_xy, b_xy = _c(a_xy), _c(b_xy)
    a_inf, b_inf = _c(a_inf, np.uint8), _c(b_inf, np.uint8)
    n = a_xy.size // words
    out = np.empty((n, words), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(fn(_h(a_xy), _hb(a_inf), _h(b_xy), _hb(b_inf), *extra, C.c_size_t(n), _h(out), _hb(oinf)), where)
    return out, oinf


def g2_is_on_curve_batch(xy, inf=None):
    """y^2 == x^3 + 3/(9+u) per point (src/poly/commitment/dory.zig computeG2YSquared); points are (n,16): x.c0, x.c1, y.c0, y.c1"""
    xy, inf = _c(xy), _c(inf, np.uint8)
    n = xy.size // 16
    out = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g2_is_on_curve_batch(_h(xy), _hb(inf), C.c_size_t(n), _hb(out)), "zg_g2_is_on_curve_batch")
    return out


def g2_affine_add_batch(a_xy, a_inf, b_xy, b_inf):
    """G2Point.add per pair (src/field/pairing.zig:839-875) -> (xy (n,16), inf (n,))"""
    return _g2_pairs(_lib.zg_g2_affine_add_batch, "zg_g2_affine_add_batch", 16, a_xy, a_inf, b_xy, b_inf)


def g2_scalar_mul_batch(xy, inf, scalars):
    """G2Point.scalarMul per (point, scalar) pair (pairing.zig:880-919) -> (xy (n,16), inf (n,))"""
    xy, inf, scalars = _c(xy), _c(inf, np.uint8), _c(scalars)
    n = scalars.size // 4
    out = np.empty((n, 16), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g2_scalar_mul_batch(_h(xy), _hb(inf), _h(scalars), C.c_size_t(n), _h(out), _hb(oinf)), "zg_g2_scalar_mul_batch")
    return out, oinf


def g2_fixed_base_mul_batch(base_xy, scalars, base_inf=0):
    """scalars[i] * base for one shared G2 base (dory.zig:963-966, 1513-1519) -> (xy (n,16), inf (n,))"""
    base_xy, scalars = _c(base_xy), _c(scalars)
    n = scalars.size // 4
    out = np.empty((n, 16), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _chk(_lib.zg_g2_fixed_base_mul_batch(_h(base_xy), C.c_uint8(base_inf), _h(scalars), C.c_size_t(n), _h(out), _hb(oinf)),
         "zg_g2_fixed_base_mul_batch")
    return out, oinf


def g2_axpy_batch(a_xy, a_inf, b_xy, b_inf, s):
    """out[i] = s * a[i] + b[i] in G2, one scalar for the vector (dory.zig:1582-1583, 1621-1624) -> (xy (n,16), inf (n,))"""
    return _g2_pairs(_lib.zg_g2_axpy_batch, "zg_g2_axpy_batch", 16, a_xy, a_inf, b_xy, b_inf, (_h(_c(s)),))


def g1_axpy_batch(a_xy, a_inf, b_xy, b_inf, s):
    """out[i] = s * a[i] + b[i] in G1 (dory.zig:1579-1580, 1616-1619) -> (xy (n,8), inf (n,))"""
    return _g2_pairs(_lib.zg_g1_axpy_batch, "zg_g1_axpy_batch", 8, a_xy, a_inf, b_xy, b_inf, (_h(_c(s)),))


def msm_g2(xy, inf, scalars, n=None):
    """msmG2 (dory.zig:693-703): sum_i scalars[i] * points[i] -> (xy (16,), inf)"""
    xy, inf, scalars = _c(xy), _c(inf, np.uint8), _c(scalars)
    n = min(xy.size // 16, scalars.size // 4) if n is None else n
    out = np.empty(16, dtype=np.uint64)
    oinf = C.c_uint8(0)
    _chk(_lib.zg_msm_g2(_h(xy), _hb(inf), _h(scalars), C.c_size_t(n), _h(out), C.byref(oinf)), "zg_msm_g2")
    return out, int(oinf.value)


def msm_g2_dev(d_xy, d_inf, d_scalars, n, d_out17, stream=0):
    """the same over device pointers; d_out17 receives xy[16] and a flag word"""
    _chk(_lib.zg_msm_g2_dev(_d(d_xy), _d(d_inf), _d(d_scalars), C.c_size_t(n), _d(stream), _d(d_out17)), "zg_msm_g2_dev")


# ---- pairings (include/zolt_gpu.h, "Pairings (Dory)"): G1 (n,8) + flags, G2 (n,16) + flags, GT elements (n,48)
def _pair_batch(fn, where, g1_xy, g1_inf, g2_xy, g2_inf):
    g1_xy, g2_xy = _c(g1_xy), _c(g2_xy)
    g1_inf, g2_inf = _c(g1_inf, np.uint8), _c(g2_inf, np.uint8)
    n = min(g1_xy.size // 8, g2_xy.size // 16)
    out = np.empty((n, 48), dtype=np.uint64)
    _chk(fn(_h(g1_xy), _hb(g1_inf), _h(g2_xy), _hb(g2_inf), C.c_size_t(n), _h(out)), where)
    return out


def miller_loop_batch(g1_xy, g1_inf, g2_xy, g2_inf):
    """millerLoopArkworks per pair (src/field/pairing.zig:1561-1628), unreduced; an identity on either side -> one -> (n,48)"""
    return _pair_batch(_lib.zg_miller_loop_batch, "zg_miller_loop_batch", g1_xy, g1_inf, g2_xy, g2_inf)


def pairing_batch(g1_xy, g1_inf, g2_xy, g2_inf):
    """pairingFp per pair (pairing.zig:1276-1286) -> (n,48)"""
    return _pair_batch(_lib.zg_pairing_batch, "zg_pairing_batch", g1_xy, g1_inf, g2_xy, g2_inf)


def final_exponentiation_batch(gt):
    """finalExponentiation per element (pairing.zig:1653-1681); zero -> one -> (n,48)"""
    gt = _c(gt)
    n = gt.size // 48
    out = np.empty((n, 48), dtype=np.uint64)
    _chk(_lib.zg_final_exponentiation_batch(_h(gt), C.c_size_t(n), _h(out)), "zg_final_exponentiation_batch")
    return out


def multi_pairing(g1_xy, g1_inf, g2_xy, g2_inf, seg=None):
    """k multi-pairings in one launch set (multiPairG1G2, dory.zig:673-690, per segment): seg = k + 1 ascending offsets into the n pairs
    (None: one product over all of them) -> (k,48)"""
    g1_xy, g2_xy = _c(g1_xy), _c(g2_xy)
    g1_inf, g2_inf = _c(g1_inf, np.uint8), _c(g2_inf, np.uint8)
    n = min(g1_xy.size // 8, g2_xy.size // 16)
    seg = np.ascontiguousarray([0, n] if seg is None else seg, dtype=np.uint64)
    k = max(seg.size - 1, 0)
    out = np.empty((k, 48), dtype=np.uint64)
    _chk(_lib.zg_multi_pairing(_h(g1_xy), _hb(g1_inf), _h(g2_xy), _hb(g2_inf), C.c_size_t(n), _h(seg), C.c_size_t(k), _h(out)), "zg_multi_pairing")
    return out


def multi_pairing_dev(d_g1_xy, d_g1_inf, d_g2_xy, d_g2_inf, n, d_seg, k, d_out_gt, stream=0):
    """the same over device pointers (d_seg: k + 1 uint64 offsets on the device); d_out_gt receives k * 48 words"""
    _chk(_lib.zg_multi_pairing_dev(_d(d_g1_xy), _d(d_g1_inf), _d(d_g2_xy), _d(d_g2_inf), C.c_size_t(n), _d(d_seg), C.c_size_t(k), _d(stream),
                                   _d(d_out_gt)), "zg_multi_pairing_dev")


# ---- which kernels compute them (include/zolt_gpu.h, "Pairings (engine)"): process-wide, needs no device, same bits either way
PAIRING_ENGINE_LANE, PAIRING_ENGINE_WAVE = 0, 1


def pairing_engine_set(engine):
    _chk(_lib.zg_pairing_engine_set(C.c_int(engine)), "zg_pairing_engine_set")


def pairing_engine_get():
    return int(_lib.zg_pairing_engine_get())


@_contextlib.contextmanager
def pairing_engine(engine):
    """run a block under `engine`, then restore the engine that was set before (also when the block raises)"""
    before = pairing_engine_get()
    pairing_engine_set(engine)
    try:
        yield engine
    finally:
        pairing_engine_set(before)


def fr_dense_evaluate(evals, point):
    evals, point = _c(evals), _c(point)
    out = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_fr_dense_evaluate(_h(evals), C.c_size_t(point.size // 4), _h(point), _h(out)), "zg_fr_dense_evaluate")
    return out


def hyperkzg_open(bases, evals, point, value):
    """HyperKZG.open on the device -> (quotient commitments (v,8), inf flags (v,), final_eval)."""
    evals, point, value = _c(evals), _c(point), _c(value)
    v = point.size // 4
    q = np.zeros((v, 8), dtype=np.uint64)
    qinf = np.zeros(v, dtype=np.uint8)
    fin = np.zeros(4, dtype=np.uint64)
    _chk(_lib.zg_hyperkzg_open(bases._h, _h(evals), C.c_size_t(evals.size // 4), _h(point), C.c_size_t(v), _h(value), _h(q),
                               _hb(qinf), _h(fin)), "zg_hyperkzg_open")
    return q, qinf, fin


def hyperkzg_open_dev(bases, d_evals, n_evals, point, value, stream=0):
    """HyperKZG.open with the table resident in HBM -> (quotient commitments (v,8), inf flags (v,), final_eval)."""
    point, value = _c(point), _c(value)
    v = point.size // 4
    q = np.zeros((v, 8), dtype=np.uint64)
    qinf = np.zeros(v, dtype=np.uint8)
    fin = np.zeros(4, dtype=np.uint64)
    _chk(_lib.zg_hyperkzg_open_dev(bases._h, _d(d_evals), C.c_size_t(n_evals), _h(point), C.c_size_t(v), _h(value), _d(stream), _h(q),
                                   _hb(qinf), _h(fin)), "zg_hyperkzg_open_dev")
    return q, qinf, fin


def hyperkzg_batch_open(bases, polys, point):
    """HyperKZG.batchOpen -> (quotient xy[nq,8], inf[nq], evaluations[k,4], final_eval, gamma)."""
    polys = [_c(p) for p in polys]
    point = _c(point)
    k, v = len(polys), point.size // 4
    ptrs = (C.c_void_p * max(k, 1))(*[p.ctypes.data if p.size else None for p in polys])
    lens = (C.c_size_t * max(k, 1))(*[p.size // 4 for p in polys])
    q = np.zeros((max(v, 1), 8), dtype=np.uint64)
    qi = np.zeros(max(v, 1), dtype=np.uint8)
    nq = C.c_size_t(0)
    ev = np.zeros((max(k, 1), 4), dtype=np.uint64)
    fin = np.zeros(4, dtype=np.uint64)
    gam = np.zeros(4, dtype=np.uint64)
    _chk(_lib.zg_hyperkzg_batch_open(bases._h, ptrs, lens, C.c_size_t(k), _h(point), C.c_size_t(v), _h(q), _hb(qi), C.byref(nq), _h(ev),
                                     _h(fin), _h(gam)), "zg_hyperkzg_batch_open")
    return q[:nq.value], qi[:nq.value], ev[:k], fin, gam


# ---- poly
def fr_eq_table(r, scale=None):
    r = _c(r)
    v = r.size // 4
    out = np.empty((1 << v, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_eq_table(_h(r), C.c_size_t(v), _h(_c(scale)), _h(out)), "zg_fr_eq_table")
    return out


def fr_eq_table_dev(r, d_out, scale=None, stream=0):
    r = _c(r)
    _chk(_lib.zg_fr_eq_table_dev(_h(r), C.c_size_t(r.size // 4), _h(_c(scale)), _d(d_out), _d(stream)), "zg_fr_eq_table_dev")


def fr_eq_plus_one_table(r):
    """out[j] = EqPlusOnePolynomial.mle(r, bits(j)) (zg_fr_eq_plus_one_table)"""
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    out = np.empty((1 << r.shape[0], 4), dtype=np.uint64)
    _chk(_lib.zg_fr_eq_plus_one_table(_h(r), C.c_size_t(r.shape[0]), _h(out)), "zg_fr_eq_plus_one_table")
    return out


def fr_eq_plus_one_table_dev(r, d_out, stream=0):
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    _chk(_lib.zg_fr_eq_plus_one_table_dev(_h(r), C.c_size_t(r.shape[0]), _d(d_out), _d(stream)), "zg_fr_eq_plus_one_table_dev")


def fr_eq_prefix_tables(tau):
    """GruenSplitEqPolynomial's prefix tables (split_eq.zig:122-171) of tau[0..v): list of v+1 arrays, table k = eq(tau[0..k), .)"""
    tau = _c(np.asarray(tau, dtype=np.uint64).reshape(-1, 4))
    v = tau.shape[0]
    out = np.empty(((2 << v) - 1, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_eq_prefix_tables(_h(tau), C.c_size_t(v), _h(out)), "zg_fr_eq_prefix_tables")
    return [out[(1 << k) - 1:(2 << k) - 1] for k in range(v + 1)]


def fr_eq_prefix_tables_dev(tau, d_out, stream=0):
    tau = _c(np.asarray(tau, dtype=np.uint64).reshape(-1, 4))
    _chk(_lib.zg_fr_eq_prefix_tables_dev(_h(tau), C.c_size_t(tau.shape[0]), _d(d_out), _d(stream)), "zg_fr_eq_prefix_tables_dev")


def fr_rows_mle(rows, r):
    """out[i] = sum_t eq(r, t) * rows[t][i] for a cycle-major (T, k, 4) matrix — R1CSInputEvaluator.computeClaimedInputs (zg_fr_rows_mle)"""
    rows = _c(rows)
    assert rows.ndim == 3 and rows.shape[2] == 4
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    out = np.empty((rows.shape[1], 4), dtype=np.uint64)
    _chk(_lib.zg_fr_rows_mle(_h(rows), C.c_size_t(rows.shape[0]), C.c_size_t(rows.shape[1]), _h(r), C.c_size_t(r.shape[0]), _h(out)), "zg_fr_rows_mle")
    return out


def fr_rows_mle_dev(d_rows, n_rows, k, r, stream=0):
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    out = np.empty((k, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_rows_mle_dev(_d(d_rows), C.c_size_t(n_rows), C.c_size_t(k), _h(r), C.c_size_t(r.shape[0]), _d(stream), _h(out)), "zg_fr_rows_mle_dev")
    return out


def fr_rows_affine(rows, coeffs, ntab, g, n_pad=None, k=None):
    """tables[t][i * g + j] = C[t*g + j][k] + sum_col C[t*g + j][col] * rows[i][col] (zg_fr_rows_affine): rows (T, stride, 4) cycle-major,
    coeffs (ntab * g, k + 1, 4) with the constant last -> ntab arrays of (n_pad * g, 4). k > stride: a sliding window — the maps of row i
    read into the rows after it, and the last k - stride elements of `rows` are only ever read as such a tail (n_rows = (T * stride - k) //
    stride + 1)."""
    rows, coeffs = _c(rows), _c(coeffs)
    stride = rows.shape[1]
    k = stride if k is None else k
    assert rows.ndim == 3 and rows.shape[2] == 4 and coeffs.shape == (ntab * g, k + 1, 4) and k >= stride
    n_rows = rows.shape[0] if k == stride else (rows.shape[0] * stride - k) // stride + 1
    n_pad = n_rows if n_pad is None else n_pad
    outs = [np.empty((n_pad * g, 4), dtype=np.uint64) for _ in range(ntab)]
    ptrs = (C.c_void_p * ntab)(*[o.ctypes.data for o in outs])
    _chk(_lib.zg_fr_rows_affine(_h(rows), C.c_size_t(n_rows), C.c_size_t(k), C.c_size_t(stride), _h(coeffs), C.c_size_t(ntab), C.c_size_t(g),
                                C.c_size_t(n_pad), ptrs), "zg_fr_rows_affine")
    return outs


COL_ZERO, COL_U8, COL_U32, COL_U64, COL_I64, COL_I128, COL_U128, COL_FR, COL_BIT, COL_MUL, COL_LUT = range(11)
_COL_DTYPE = {COL_U8: np.uint8, COL_U32: np.uint32, COL_U64: np.uint64, COL_I64: np.int64, COL_I128: np.uint64, COL_U128: np.uint64, COL_FR: np.uint64,
              COL_MUL: np.uint64}  # (COL_MUL's optional addend is a 128-bit two's-complement column)


class Column(C.Structure):
    """zg_col_t: one typed integer column of zg_fr_rows_from_columns"""
    _fields_ = [("kind", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("data", C.c_void_p), ("aux", C.c_void_p)]


def _columns(cols, n_rows, device):
    """cols: list of (kind, data, a, b[, aux]) — data a numpy array (host) or a device address (device=True), None for COL_ZERO / COL_MUL;
    COL_LUT: data = the index per row (a bytes each), aux = the table of b elements"""
    arr = (Column * len(cols))()
    keep = []
    for i, spec in enumerate(cols):
        kind, data = spec[0], spec[1] if len(spec) > 1 else None
        a, b = (spec[2] if len(spec) > 2 else 0), (spec[3] if len(spec) > 3 else 0)
        aux = spec[4] if len(spec) > 4 else None
        ptr = aptr = None
        if aux is not None:
            if device:
                aptr = int(aux)
            else:
                t = np.ascontiguousarray(aux, dtype=np.uint64)
                assert t.size == 4 * b, (i, t.shape, b)
                keep.append(t)
                aptr = t.ctypes.data
        if data is not None:
            if device:
                ptr = int(data)
            else:
                dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[a] if kind == COL_LUT else (_COL_DTYPE.get(kind) or {1: np.uint8, 4: np.uint32, 8: np.uint64}[b])
                h = np.ascontiguousarray(data, dtype=dt)
                per = {COL_I128: 2, COL_U128: 2, COL_FR: 4, COL_MUL: 2}.get(kind, 1)
                assert h.size == n_rows * per, (i, kind, h.shape, n_rows)
                keep.append(h)
                ptr = h.ctypes.data
        arr[i] = Column(kind, a, b, ptr, aptr)
    return arr, keep


def fr_rows_from_columns(cols, n_rows, d_rows=None):
    """The witness matrix built on the device from integer columns (zg_fr_rows_from_columns): rows[row][c] = column c's value at `row`
    as a Montgomery element. d_rows: a device address to fill (returns None); None: the (n_rows, n_cols, 4) matrix comes back to the host."""
    arr, keep = _columns(cols, n_rows, device=False)
    buf = None
    if d_rows is None:
        buf = DeviceBuffer(max(n_rows * len(cols) * 32, 32))
        d_rows = buf.ptr
    _chk(_lib.zg_fr_rows_from_columns(arr, C.c_size_t(len(cols)), C.c_size_t(n_rows), _d(d_rows)), "zg_fr_rows_from_columns")
    del keep
    if buf is None:
        return None
    out = buf.to_host()[:n_rows * len(cols) * 4].reshape(n_rows, len(cols), 4)
    buf.free()
    return out


def fr_rows_from_columns_dev(cols, n_rows, d_rows, stream=0):
    """the same with the columns resident in HBM (data = device addresses); asynchronous"""
    arr, _ = _columns(cols, n_rows, device=True)
    _chk(_lib.zg_fr_rows_from_columns_dev(arr, C.c_size_t(len(cols)), C.c_size_t(n_rows), _d(d_rows), _d(stream)), "zg_fr_rows_from_columns_dev")


def fr_lt_table(r):
    """out[j] = LtPolynomial(r).evaluateAtIndex(j) over the cube (zg_fr_lt_table); index bit i <-> r[i]"""
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    out = np.empty((1 << r.shape[0], 4), dtype=np.uint64)
    _chk(_lib.zg_fr_lt_table(_h(r), C.c_size_t(r.shape[0]), _h(out)), "zg_fr_lt_table")
    return out


def fr_lt_table_dev(r, d_out, stream=0):
    r = _c(np.asarray(r, dtype=np.uint64).reshape(-1, 4))
    _chk(_lib.zg_fr_lt_table_dev(_h(r), C.c_size_t(r.shape[0]), _d(d_out), _d(stream)), "zg_fr_lt_table_dev")


def fr_write_tables_dev(n, cycle, word, pre, post, r_eq, d_inc, d_wa, stream=0):
    """ValEvaluation's inc / wa (n entries each, device) from the list of writes (zg_fr_write_tables_dev): inc[cycle] = F(post) - F(pre),
    wa[cycle] = eq(r_eq, word); r_eq (log_k, 4) in EqPolynomial order"""
    cycle, word, pre, post = _c(cycle, np.uint32), _c(word, np.uint32), _c(pre), _c(post)
    r_eq = _c(np.asarray(r_eq, dtype=np.uint64).reshape(-1, 4))
    m = cycle.size
    assert word.size == pre.size == post.size == m
    _chk(_lib.zg_fr_write_tables_dev(C.c_size_t(n), C.c_size_t(m), _hb(cycle), _hb(word), _h(pre), _h(post), _h(r_eq) if r_eq.size else None,
                                     C.c_size_t(r_eq.shape[0]), _d(d_inc), _d(d_wa), _d(stream)), "zg_fr_write_tables_dev")


def fr_weighted_colsum(table, rows, cols, weights):
    """out[k][c] = sum_r weights[k][r] * table[r * cols + c] (zg_fr_weighted_colsum): table (rows * cols, 4), weights (m, rows, 4), m <= 4
    -> (m, cols, 4)"""
    table, weights = _c(table), _c(weights)
    m = weights.size // (4 * rows)
    assert table.size == rows * cols * 4 and weights.size == m * rows * 4
    out = np.empty((m, cols, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_weighted_colsum(_h(table), C.c_size_t(rows), C.c_size_t(cols), _h(weights), C.c_size_t(m), _h(out)), "zg_fr_weighted_colsum")
    return out


def fr_weighted_colsum_dev(d_table, rows, cols, d_weights, m, d_out, stream=0):
    _chk(_lib.zg_fr_weighted_colsum_dev(_d(d_table), C.c_size_t(rows), C.c_size_t(cols), _d(d_weights), C.c_size_t(m), _d(d_out), _d(stream)),
         "zg_fr_weighted_colsum_dev")


def fr_rows_affine_dev(d_rows, n_rows, k, coeffs, ntab, g, n_pad, d_tables, stream=0, stride=0):
    coeffs = _c(coeffs)
    assert coeffs.size == ntab * g * (k + 1) * 4 and len(d_tables) == ntab
    ptrs = (C.c_void_p * ntab)(*[int(p) for p in d_tables])
    _chk(_lib.zg_fr_rows_affine_dev(_d(d_rows), C.c_size_t(n_rows), C.c_size_t(k), C.c_size_t(stride), _h(coeffs), C.c_size_t(ntab), C.c_size_t(g),
                                    C.c_size_t(n_pad), ptrs, _d(stream)), "zg_fr_rows_affine_dev")


def fr_rows_affine_records_dev(d_rows, n_rows, k, coeffs, record, first, d_out, stream=0, stride=0):
    """d_out[i * record + first + c] = map_c(row_i) for the nout <= 16 maps of coeffs (nout, k + 1, 4) (zg_fr_rows_affine_records_dev)"""
    coeffs = _c(coeffs)
    nout = coeffs.shape[0]
    assert coeffs.shape == (nout, k + 1, 4)
    _chk(_lib.zg_fr_rows_affine_records_dev(_d(d_rows), C.c_size_t(n_rows), C.c_size_t(k), C.c_size_t(stride), _h(coeffs), C.c_size_t(nout), C.c_size_t(record),
                                            C.c_size_t(first), _d(d_out), _d(stream)), "zg_fr_rows_affine_records_dev")


def fr_rows_affine_prodsum_dev(d_rows, n_rows, k, coeffs, npairs, d_weights, g, stream=0, stride=0):
    """out[p] = sum_i W[i * g + p % g] * A_p(row_i) * B_p(row_i) (zg_fr_rows_affine_prodsum_dev) -> (npairs, 4)"""
    coeffs = _c(coeffs)
    assert coeffs.size == 2 * npairs * (k + 1) * 4
    out = np.empty((npairs, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_rows_affine_prodsum_dev(_d(d_rows), C.c_size_t(n_rows), C.c_size_t(k), C.c_size_t(stride), _h(coeffs), C.c_size_t(npairs), _d(d_weights),
                                            C.c_size_t(g), _h(out), _d(stream)), "zg_fr_rows_affine_prodsum_dev")
    return out


def fr_bind_low(table, r):
    t = np.array(table, dtype=np.uint64, copy=True).reshape(-1, 4)
    n = t.shape[0]
    _chk(_lib.zg_fr_bind_low(_h(t), C.c_size_t(n), _h(_c(r))), "zg_fr_bind_low")
    return t[: n // 2].copy()


def fr_bind_high(table, r):
    t = _c(table).reshape(-1, 4)
    n = t.shape[0]
    out = np.empty((n // 2, 4), dtype=np.uint64)
    _chk(_lib.zg_fr_bind_high(_h(t), C.c_size_t(n), _h(_c(r)), _h(out)), "zg_fr_bind_high")
    return out


def fr_spartan_combine(eq, az, bz, cz):
    eq, az, bz, cz = _c(eq), _c(az), _c(bz), _c(cz)
    out = np.empty_like(eq)
    _chk(_lib.zg_fr_spartan_combine(_h(eq), _h(az), _h(bz), _h(cz), C.c_size_t(eq.size // 4), _h(out)), "zg_fr_spartan_combine")
    return out


def fr_spartan_combine_dev(d_eq, d_az, d_bz, d_cz, n, d_out, stream=0):
    _chk(_lib.zg_fr_spartan_combine_dev(_d(d_eq), _d(d_az), _d(d_bz), _d(d_cz), C.c_size_t(n), _d(d_out), _d(stream)),
         "zg_fr_spartan_combine_dev")


def fr_bit_split_sums(vals, idx128, bit):
    """sums of vals[j] split by bit `bit` of the u128 index (n,2) -> (sum0, sum1)"""
    vals, idx128 = _c(vals), _c(idx128)
    s0 = np.empty(4, dtype=np.uint64)
    s1 = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_fr_bit_split_sums(_h(vals), _h(idx128), C.c_size_t(vals.size // 4), C.c_uint(bit), _h(s0), _h(s1)), "zg_fr_bit_split_sums")
    return s0, s1


def fr_bit_split_sums_dev(d_vals, d_idx128, n, bit, stream=0):
    s0 = np.empty(4, dtype=np.uint64)
    s1 = np.empty(4, dtype=np.uint64)
    _chk(_lib.zg_fr_bit_split_sums_dev(_d(d_vals), _d(d_idx128), C.c_size_t(n), C.c_uint(bit), _d(stream), _h(s0), _h(s1)),
         "zg_fr_bit_split_sums_dev")
    return s0, s1


def selftest_handoff(blocks, threads=512, iters=200, busy=True):
    """zg_selftest_handoff: (words that differed, launches that elected exactly one last arriver)"""
    bad = C.c_uint64(0)
    done = C.c_uint64(0)
    _chk(_lib.zg_selftest_handoff(C.c_uint(blocks), C.c_uint(threads), C.c_uint(iters), C.c_int(1 if busy else 0), C.byref(bad), C.byref(done)),
         "zg_selftest_handoff")
    return int(bad.value), int(done.value)


class SumcheckVerificationFailed(RuntimeError):
    """error.SumcheckVerificationFailed (src/subprotocols/mod.zig:175-178)."""


def _run_sumcheck_call(fn, ptr, n, extra, where):
    v = max(n.bit_length() - 1, 0)
    claim = np.empty(4, dtype=np.uint64)
    rounds = np.empty((v, 2, 4), dtype=np.uint64)
    chal = np.empty((v, 4), dtype=np.uint64)
    fin = np.empty(4, dtype=np.uint64)
    res = C.c_uint8(0)
    rc = fn(ptr, C.c_size_t(n), *extra, _h(claim), _h(rounds) if v else None, _h(chal) if v else None, _h(fin), C.byref(res))
    if rc == ERR_VERIFY:
        raise SumcheckVerificationFailed(last_error())
    _chk(rc, where)
    return {"claim": claim, "rounds": rounds, "final_point": chal, "final_eval": fin, "result": bool(res.value)}


def run_sumcheck(evals):
    """runSumcheck (src/subprotocols/mod.zig:302-354), prover and toy verifier both on the device."""
    e = _c(evals)
    return _run_sumcheck_call(_lib.zg_run_sumcheck, _h(e), e.size // 4, (), "zg_run_sumcheck")


def run_sumcheck_dev(d_evals, n, stream=0):
    return _run_sumcheck_call(_lib.zg_run_sumcheck_dev, _d(d_evals), n, (_d(stream),), "zg_run_sumcheck_dev")


class SumcheckSession:
    """Device-resident Sumcheck(F).Prover table (src/subprotocols/mod.zig:50-134)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, evals, layout=SC_HIGH_HALF):
        e = _c(evals)
        h = C.c_void_p()
        _chk(_lib.zg_sumcheck_open(_h(e), C.c_size_t(e.size // 4), C.c_int(layout), C.byref(h)), "zg_sumcheck_open")
        return cls(h)

    @classmethod
    def open_dev(cls, d_evals, n, layout=SC_HIGH_HALF, stream=0, borrow=False):
        """borrow: no copy — the session reads the caller's device table until its first bind has run (zg_sumcheck_open_dev_borrowed);
        the caller keeps it alive and unchanged until then"""
        h = C.c_void_p()
        if borrow:
            _chk(_lib.zg_sumcheck_open_dev_borrowed(_d(d_evals), C.c_size_t(n), C.c_int(layout), _d(stream), C.byref(h)), "zg_sumcheck_open_dev_borrowed")
        else:
            _chk(_lib.zg_sumcheck_open_dev(_d(d_evals), C.c_size_t(n), C.c_int(layout), _d(stream), C.byref(h)), "zg_sumcheck_open_dev")
        return cls(h)

    @classmethod
    def open_column(cls, col, n_rows, n, layout=SC_HIGH_HALF):
        """a session whose table is ONE integer column widened on the device: entries [0, n_rows) from `col` (a fr_rows_from_columns
        column spec, host data), [n_rows, n) zero (zg_sumcheck_open_column)"""
        arr, keep = _columns([col], n_rows, device=False)
        h = C.c_void_p()
        _chk(_lib.zg_sumcheck_open_column(arr, C.c_size_t(n_rows), C.c_size_t(n), C.c_int(layout), C.byref(h)), "zg_sumcheck_open_column")
        del keep
        return cls(h)

    @classmethod
    def open_spartan_dev(cls, r, d_az, d_bz, d_cz, layout=SC_HIGH_HALF, scale=None, stream=0):
        """f = eq(r, .) * (Az*Bz - Cz) built straight into a new session (round 0's sums included), zg_sumcheck_open_spartan_dev."""
        r = _c(r)
        h = C.c_void_p()
        _chk(_lib.zg_sumcheck_open_spartan_dev(_h(r), C.c_size_t(r.size // 4), _h(_c(scale)), _d(d_az), _d(d_bz), _d(d_cz), C.c_int(layout),
                                               _d(stream), C.byref(h)), "zg_sumcheck_open_spartan_dev")
        return cls(h)

    def round_sums(self):
        g0 = np.empty(4, dtype=np.uint64)
        g1 = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_round_sums(self._h, _h(g0), _h(g1)), "zg_sumcheck_round_sums")
        return g0, g1

    def bind(self, r):
        _chk(_lib.zg_sumcheck_bind(self._h, _h(_c(r))), "zg_sumcheck_bind")

    def __len__(self):
        return int(_lib.zg_sumcheck_len(self._h))

    def final(self):
        out = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_final(self._h, _h(out)), "zg_sumcheck_final")
        return out

    def read(self):
        out = np.empty((len(self), 4), dtype=np.uint64)
        _chk(_lib.zg_sumcheck_read(self._h, _h(out)), "zg_sumcheck_read")
        return out

    def gather(self, idx):
        """table[idx[i]] of the current table -> (n, 4)"""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.empty((idx.size, 4), dtype=np.uint64)
        _chk(_lib.zg_sumcheck_gather(self._h, _h(idx), C.c_size_t(idx.size), _h(out)), "zg_sumcheck_gather")
        return out

    def raf_round(self, base, current_power):
        """RAF cubic round sums s(0), s(2) over this LOW_PAIR session's table (zg_sumcheck_raf_round)"""
        s0 = np.empty(4, dtype=np.uint64)
        s2 = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_raf_round(self._h, _h(_c(base)), C.c_uint64(current_power), _h(s0), _h(s2)), "zg_sumcheck_raf_round")
        return s0, s2

    def raf_claim(self, base, step=8):
        """sum_k t[k] * F.fromU64(base + step * k) over the current table: RafEvaluationProver.computeInitialClaim (zg_sumcheck_raf_claim)"""
        out = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_raf_claim(self._h, C.c_uint64(base), C.c_uint64(step), _h(out)), "zg_sumcheck_raf_claim")
        return out

    def bit_round(self, d_idx128, n_idx, bit):
        """LassoProver.computeAddressRoundPoly's sum_0 / sum_1 over the session's first n_idx entries (zg_sumcheck_bit_round)"""
        s0 = np.empty(4, dtype=np.uint64)
        s1 = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_bit_round(self._h, _d(d_idx128), C.c_size_t(n_idx), C.c_uint(bit), _h(s0), _h(s1)), "zg_sumcheck_bit_round")
        return s0, s1

    def bit_bind(self, d_idx128, n_idx, bit, r):
        """LassoProver.receiveChallenge's address branch in place; -> the new claim (zg_sumcheck_bit_bind)"""
        claim = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_bit_bind(self._h, _d(d_idx128), C.c_size_t(n_idx), C.c_uint(bit), _h(_c(r)), _h(claim)), "zg_sumcheck_bit_bind")
        return claim

    def round_sums_dev(self, d_out8):
        _chk(_lib.zg_sumcheck_round_sums_dev(self._h, _d(d_out8)), "zg_sumcheck_round_sums_dev")

    def read_dev(self, d_out):
        _chk(_lib.zg_sumcheck_read_dev(self._h, _d(d_out)), "zg_sumcheck_read_dev")

    def close(self):
        if self._h:
            _chk(_lib.zg_sumcheck_close(self._h), "zg_sumcheck_close")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PSC_PAIR_SUM = 256  # ZG_PSC_PAIR_SUM


class PscTerm(C.Structure):
    """zg_psc_term: one product term of zg_psc_round_expr"""
    _fields_ = [("n_prod", C.c_int), ("prod", C.c_int * 4), ("n_lin", C.c_int), ("lin", C.c_int * 4), ("lin_coeff", C.c_uint64 * 16)]


class ProductSumcheckSession:
    """k multilinear tables folded together (LowToHigh) with product-form round evaluations (zg_psc_*): the loops of
    ValEvaluationProver, ValFinalProver, OutputSumcheckProver, InstructionLookupsClaimReduction and ProductVirtualRemainderProver."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, tables):
        tabs = [_c(t).reshape(-1, 4) for t in tables]
        n = tabs[0].shape[0]
        assert all(t.shape[0] == n for t in tabs)
        ptrs = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
        h = C.c_void_p()
        _chk(_lib.zg_psc_open(ptrs, C.c_size_t(len(tabs)), C.c_size_t(n), C.byref(h)), "zg_psc_open")
        return cls(h)

    def table_dev(self, table):
        """device address of a table's current entries (zg_psc_table_dev): valid until the next bind / close"""
        p = C.c_void_p()
        _chk(_lib.zg_psc_table_dev(self._h, C.c_size_t(table), C.byref(p)), "zg_psc_table_dev")
        return p.value

    @classmethod
    def open_dev(cls, d_tables, n, stream=0):
        ptrs = (C.c_void_p * len(d_tables))(*[int(p) for p in d_tables])
        h = C.c_void_p()
        _chk(_lib.zg_psc_open_dev(ptrs, C.c_size_t(len(d_tables)), C.c_size_t(n), _d(stream), C.byref(h)), "zg_psc_open_dev")
        return cls(h)

    def __len__(self):
        return int(_lib.zg_psc_len(self._h))

    def tables(self):
        return int(_lib.zg_psc_tables(self._h))

    def round_evals(self, prod_idx, lin_idx=(), lin_coeff=None):
        """[p(0), p(1), p(2), p(3)] of sum_g prod_j T[prod_idx[j]](t) * sum_m lin_coeff[m] T[lin_idx[m]](t)"""
        pi = (C.c_int * max(len(prod_idx), 1))(*prod_idx)
        li = (C.c_int * max(len(lin_idx), 1))(*lin_idx)
        co = _c(lin_coeff) if len(lin_idx) else None
        out = np.empty((4, 4), dtype=np.uint64)
        _chk(_lib.zg_psc_round_evals(self._h, pi, C.c_size_t(len(prod_idx)), li, _h(co), C.c_size_t(len(lin_idx)), _h(out)), "zg_psc_round_evals")
        return out

    def round_expr(self, terms):
        """[p(0..3)] of a SUM of product terms; terms: list of (prod_idx, lin_idx, lin_coeff) with lin_coeff (len(lin_idx), 4) or None,
        or (prod_idx, lin_idx, lin_coeff, True) for a ZG_PSC_PAIR_SUM term: (T[p0] T[p1] + T[p2] T[p3]) * L"""
        arr = (PscTerm * len(terms))()
        for t, term in zip(arr, terms):
            prod_idx, lin_idx, coeff = term[:3]
            t.n_prod, t.n_lin = len(prod_idx) | (PSC_PAIR_SUM if len(term) > 3 and term[3] else 0), len(lin_idx)
            for j, v in enumerate(prod_idx):
                t.prod[j] = v
            for m, v in enumerate(lin_idx):
                t.lin[m] = v
            if len(lin_idx):
                flat = _c(coeff).reshape(-1)
                for i in range(4 * len(lin_idx)):
                    t.lin_coeff[i] = int(flat[i])
        out = np.empty((4, 4), dtype=np.uint64)
        _chk(_lib.zg_psc_round_expr(self._h, arr, C.c_size_t(len(terms)), _h(out)), "zg_psc_round_expr")
        return out

    def set_points(self, points):
        """bit t of `points`: the round calls compute p(t); the other slots come back as zero (zg_psc_set_points)"""
        _chk(_lib.zg_psc_set_points(self._h, C.c_uint(points)), "zg_psc_set_points")

    def round_gruen(self, prod_idx, d_e_out, n_out, d_e_in, n_in):
        """Gruen's (t0, t_inf) under the split-eq weights E_out x E_in (device pointers)"""
        pi = (C.c_int * max(len(prod_idx), 1))(*prod_idx)
        t0 = np.empty(4, dtype=np.uint64)
        ti = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_psc_round_gruen(self._h, pi, C.c_size_t(len(prod_idx)), _d(d_e_out), C.c_size_t(n_out), _d(d_e_in), C.c_size_t(n_in),
                                     _h(t0), _h(ti)), "zg_psc_round_gruen")
        return t0, ti

    def bind(self, r):
        _chk(_lib.zg_psc_bind(self._h, _h(_c(r))), "zg_psc_bind")

    def read(self, table):
        out = np.empty((len(self), 4), dtype=np.uint64)
        _chk(_lib.zg_psc_read(self._h, C.c_size_t(table), _h(out)), "zg_psc_read")
        return out

    def gather(self, table, idx):
        """T[table][idx[i]] of the current tables -> (n, 4)"""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.empty((idx.size, 4), dtype=np.uint64)
        _chk(_lib.zg_psc_gather(self._h, C.c_size_t(table), _h(idx), C.c_size_t(idx.size), _h(out)), "zg_psc_gather")
        return out

    def final(self):
        out = np.empty((self.tables(), 4), dtype=np.uint64)
        _chk(_lib.zg_psc_final(self._h, _h(out)), "zg_psc_final")
        return out

    def close(self):
        if self._h:
            _chk(_lib.zg_psc_close(self._h), "zg_psc_close")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DORY_VMV_WORDS, DORY_FIRST_WORDS, DORY_SECOND_WORDS, DORY_FINAL_WORDS = (_abi.ZG_DORY_VMV_WORDS, _abi.ZG_DORY_FIRST_WORDS, _abi.ZG_DORY_SECOND_WORDS,
                                                                          _abi.ZG_DORY_FINAL_WORDS)


class DoryOpenSession:
    """openWithTranscript's reduce-and-fold loop resident on the device (zg_dory_open_*): begin uploads everything once, a round is
    first_message() -> second_message(beta, beta_inv) -> fold(alpha, alpha_inv), final(gamma, gamma_inv) closes the proof. Messages are
    flat uint64 records in the layouts of include/zolt_gpu.h; `vmv` is the VMV message begin returned. begin_key begins the same session
    over a resident DoryKey, on DoryCommitmentScheme.open's schedule; run(challenges) is every round and the final message in one call."""

    def __init__(self, handle, vmv, sigma):
        self._h = handle
        self.vmv = vmv
        self.sigma = sigma
        self._key = None

    @classmethod
    def begin(cls, g1_vec, g2_vec, row_commitments, v_vec, right_vec, left_vec, nu, sigma):
        """g1_vec / g2_vec / row_commitments: (xy, inf) with inf None for "no identities"; the scalar vectors (n, 4) Montgomery Fr"""
        g1, g1i = _c(g1_vec[0]).reshape(-1, 8), _c(g1_vec[1], np.uint8)
        g2, g2i = _c(g2_vec[0]).reshape(-1, 16), _c(g2_vec[1], np.uint8)
        rows, rowsi = _c(row_commitments[0]).reshape(-1, 8), _c(row_commitments[1], np.uint8)
        v, right, left = (_c(a).reshape(-1, 4) for a in (v_vec, right_vec, left_vec))
        n_gens = min(g1.shape[0], g2.shape[0])
        if not 0 <= nu <= sigma <= 63:
            raise ValueError(f"DoryOpenSession.begin: 0 <= nu <= sigma required, got nu = {nu}, sigma = {sigma}")
        if (g1i is not None and g1i.size < n_gens) or (g2i is not None and g2i.size < n_gens) or (rowsi is not None and rowsi.size < rows.shape[0]):
            raise ValueError("DoryOpenSession.begin: a flag array is shorter than its points")
        if right.shape[0] < (1 << sigma) or left.shape[0] < (1 << nu):
            raise ValueError("DoryOpenSession.begin: right_vec needs 2^sigma and left_vec 2^nu scalars")
        vmv = np.empty(DORY_VMV_WORDS, dtype=np.uint64)
        h = C.c_void_p()
        _chk(_lib.zg_dory_open_begin(_h(g1), _hb(g1i), _h(g2), _hb(g2i), C.c_size_t(n_gens), _h(rows) if rows.shape[0] else None, _hb(rowsi),
                                     C.c_size_t(rows.shape[0]), _h(v) if v.shape[0] else None, C.c_size_t(v.shape[0]), _h(right), _h(left),
                                     C.c_uint32(nu), C.c_uint32(sigma), _h(vmv), C.byref(h)), "zg_dory_open_begin")
        return cls(h, vmv, sigma)

    @classmethod
    def begin_key(cls, key, row_commitments, v_vec, right_vec, left_vec, nu, sigma):
        """the same over a resident DoryKey (zg_dory_open_key_begin): the generators and the MSM handle are the key's, read in place, and
        the rounds run DoryCommitmentScheme.open's schedule — 2^sigma G1 against 2^nu G2 generators. The key must outlive the session."""
        rows, rowsi = _c(row_commitments[0]).reshape(-1, 8), _c(row_commitments[1], np.uint8)
        v, right, left = (_c(a).reshape(-1, 4) for a in (v_vec, right_vec, left_vec))
        if not 0 <= nu <= 63 or not 0 <= sigma <= 63:
            raise ValueError(f"DoryOpenSession.begin_key: nu = {nu}, sigma = {sigma}")
        if rowsi is not None and rowsi.size < rows.shape[0]:
            raise ValueError("DoryOpenSession.begin_key: a flag array is shorter than its points")
        if right.shape[0] < (1 << sigma) or left.shape[0] < (1 << nu):
            raise ValueError("DoryOpenSession.begin_key: right_vec needs 2^sigma and left_vec 2^nu scalars")
        vmv = np.empty(DORY_VMV_WORDS, dtype=np.uint64)
        h = C.c_void_p()
        _chk(_lib.zg_dory_open_key_begin(key._h if key is not None else None, _h(rows) if rows.shape[0] else None, _hb(rowsi), C.c_size_t(rows.shape[0]),
                                         _h(v) if v.shape[0] else None, C.c_size_t(v.shape[0]), _h(right), _h(left), C.c_uint32(nu), C.c_uint32(sigma),
                                         _h(vmv), C.byref(h)), "zg_dory_open_key_begin")
        ses = cls(h, vmv, sigma)
        ses._key = key  # the key is not collected under the session
        return ses

    def run(self, challenges):
        """every round and the final message in one call and one synchronisation (zg_dory_open_run), right after begin. challenges:
        (beta, beta_inv, alpha, alpha_inv) per round, then (gamma, gamma_inv), Montgomery Fr, (4 sigma + 2, 4)
        -> (first (sigma, 218), second (sigma, 148), final (26,))"""
        ch = _c(challenges).reshape(-1, 4)
        if ch.shape[0] != 4 * self.sigma + 2:
            raise ValueError(f"DoryOpenSession.run: {4 * self.sigma + 2} challenge scalars expected, got {ch.shape[0]}")
        first = np.empty((self.sigma, DORY_FIRST_WORDS), dtype=np.uint64)
        second = np.empty((self.sigma, DORY_SECOND_WORDS), dtype=np.uint64)
        final = np.empty(DORY_FINAL_WORDS, dtype=np.uint64)
        _chk(_lib.zg_dory_open_run(self._h, _h(ch), _h(first) if self.sigma else None, _h(second) if self.sigma else None, _h(final)), "zg_dory_open_run")
        return first, second, final

    def __len__(self):
        return int(_lib.zg_dory_open_len(self._h))

    def first_message(self):
        out = np.empty(DORY_FIRST_WORDS, dtype=np.uint64)
        _chk(_lib.zg_dory_open_first_message(self._h, _h(out)), "zg_dory_open_first_message")
        return out

    def second_message(self, beta, beta_inv):
        out = np.empty(DORY_SECOND_WORDS, dtype=np.uint64)
        _chk(_lib.zg_dory_open_second_message(self._h, _h(_c(beta)), _h(_c(beta_inv)), _h(out)), "zg_dory_open_second_message")
        return out

    def fold(self, alpha, alpha_inv):
        _chk(_lib.zg_dory_open_fold(self._h, _h(_c(alpha)), _h(_c(alpha_inv))), "zg_dory_open_fold")

    def final(self, gamma, gamma_inv):
        out = np.empty(DORY_FINAL_WORDS, dtype=np.uint64)
        _chk(_lib.zg_dory_open_final(self._h, _h(_c(gamma)), _h(_c(gamma_inv)), _h(out)), "zg_dory_open_final")
        return out

    def _hook(self, op, out, n):
        word = np.array([self._h.value if isinstance(self._h, C.c_void_p) else (self._h or 0)], dtype=np.uint64)
        _chk(_lib.zg_field_op(C.c_int(FR), C.c_int(op), _h(word), None, _h(out), C.c_size_t(n)), "zg_field_op(ZG_OP_DORY_*)")

    def wait(self):
        """returns when the session's enqueued work (a fold) has run: a state hook with room for nothing"""
        self._hook(OP_DORY_S1, None, 0)

    def state(self):
        """(v1 (xy, inf), v2 (xy, inf), s1, s2) over the live length: the self-test read-back (ZG_OP_DORY_* of zg_field_op)"""
        n = len(self)
        r1, r2 = np.zeros((n, 9), dtype=np.uint64), np.zeros((n, 17), dtype=np.uint64)
        s1, s2 = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        for op, out in ((OP_DORY_V1, r1), (OP_DORY_V2, r2), (OP_DORY_S1, s1), (OP_DORY_S2, s2)):
            self._hook(op, out, n)
        return (np.ascontiguousarray(r1[:, :8]), r1[:, 8].astype(np.uint8)), (np.ascontiguousarray(r2[:, :16]), r2[:, 16].astype(np.uint8)), s1, s2

    def close(self):
        if self._h:
            _chk(_lib.zg_dory_open_close(self._h), "zg_dory_open_close")
            self._h = None
            self._key = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DORY_POLY_FR, DORY_POLY_U64, DORY_POLY_CHUNK64, DORY_POLY_CHUNK128 = (_abi.ZG_DORY_POLY_FR, _abi.ZG_DORY_POLY_U64, _abi.ZG_DORY_POLY_CHUNK64,
                                                                         _abi.ZG_DORY_POLY_CHUNK128)
_DORY_POLY_WORDS = {DORY_POLY_FR: 4, DORY_POLY_U64: 1, DORY_POLY_CHUNK64: 1, DORY_POLY_CHUNK128: 2}


class DoryKey:
    """Both generator vectors of a Dory SRS, the digit table d * g1_vec[c] (d = 1..255) and an MSM handle over g1_vec, resident on the
    device (zg_dory_key_*): what dory_commit_batch commits over."""

    def __init__(self, handle, g1_0=None, g2_0=None):
        self._h = handle
        self.g1_0, self.g2_0 = g1_0, g2_0  # host copies of the first generators (xy, inf): what a verifier setup serialises beside its GT values

    @classmethod
    def create(cls, g1_vec, g2_vec):
        """g1_vec = (xy (n1, 8), inf or None), g2_vec = (xy (n2, 16), inf or None)"""
        g1, g1i = _c(g1_vec[0]).reshape(-1, 8), _c(g1_vec[1], np.uint8)
        g2, g2i = _c(g2_vec[0]).reshape(-1, 16), _c(g2_vec[1], np.uint8)
        if (g1i is not None and g1i.size < g1.shape[0]) or (g2i is not None and g2i.size < g2.shape[0]):
            raise ValueError("DoryKey.create: a flag array is shorter than its points")
        h = C.c_void_p()
        _chk(_lib.zg_dory_key_create(_h(g1), _hb(g1i), C.c_size_t(g1.shape[0]), _h(g2) if g2.shape[0] else None, _hb(g2i), C.c_size_t(g2.shape[0]),
                                     C.byref(h)), "zg_dory_key_create")
        return cls(h, (g1[0].copy(), 0 if g1i is None else int(g1i[0]) & 1), (g2[0].copy(), 0 if g2i is None else int(g2i[0]) & 1) if g2.shape[0] else None)

    @classmethod
    def from_bytes(cls, g1_data, g1_encoding, g2_data, g2_encoding, flags=0):
        """create over both vectors as the records of a file (POINT_BYTES_*), decoded on the device and built where they lie
        (zg_dory_key_from_bytes); PointBytesError on a bad record, its first_bad a G1 index or n_g1 + a G2 index"""
        where = "zg_dory_key_from_bytes"
        a1, n1 = _records(g1_data, 1, g1_encoding, where)
        a2, n2 = _records(g2_data, 2, g2_encoding, where)
        h, bad = C.c_void_p(), C.c_size_t(n1 + n2)
        rc = _lib.zg_dory_key_from_bytes(_hb(a1) if n1 else None, C.c_size_t(n1), C.c_uint32(g1_encoding), _hb(a2) if n2 else None, C.c_size_t(n2),
                                         C.c_uint32(g2_encoding), C.c_uint32(flags), C.byref(h), C.byref(bad))
        _chk_records(rc, where, bad, n1 + n2)
        key = cls(h)
        del key.g1_0, key.g2_0  # decoded from copies of their records when first read (__getattr__): a prover never reads them
        s1, s2 = point_record_bytes(1, g1_encoding), point_record_bytes(2, g2_encoding)
        key._first = (bytes(a1[:s1]), g1_encoding, bytes(a2[:s2]) if n2 else None, g2_encoding)
        return key

    def __getattr__(self, name):
        first = self.__dict__.get("_first")
        if name not in ("g1_0", "g2_0") or first is None:
            raise AttributeError(name)
        del self._first
        xy, inf = g1_points_from_bytes(first[0], first[1])
        self.g1_0, self.g2_0 = (xy[0], int(inf[0])), None
        if first[2] is not None:
            xy, inf = g2_points_from_bytes(first[2], first[3])
            self.g2_0 = (xy[0], int(inf[0]))
        return self.__dict__[name]

    def lens(self):
        """(n_g1, n_g2)"""
        a, b = C.c_size_t(), C.c_size_t()
        _chk(_lib.zg_dory_key_len(self._h, C.byref(a), C.byref(b)), "zg_dory_key_len")
        return int(a.value), int(b.value)

    def table_bytes(self):
        return 255 * 64 * self.lens()[0]

    def free(self):
        if self._h:
            _chk(_lib.zg_dory_key_free(self._h), "zg_dory_key_free")
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- points from bytes (include/zolt_gpu.h, "Points from bytes")
POINT_BYTES_BE, POINT_BYTES_LE, POINT_BYTES_ARK, POINT_BYTES_ARK_COMPRESSED = (_abi.ZG_POINT_BYTES_BE, _abi.ZG_POINT_BYTES_LE, _abi.ZG_POINT_BYTES_ARK,
                                                                               _abi.ZG_POINT_BYTES_ARK_COMPRESSED)
POINT_BYTES_CHECK = _abi.ZG_POINT_BYTES_CHECK


def point_record_bytes(group, encoding):
    """bytes of one record: group 1 (G1) or 2 (G2)"""
    return (32 if group == 1 else 64) * (1 if encoding == POINT_BYTES_ARK_COMPRESSED else 2)


class PointBytesError(ZgError):
    """a bad record: first_bad is the smallest bad index, reason "PointNotOnCurve" or "DecompressionFailed\""""

    def __init__(self, code, where, first_bad):
        super().__init__(code, where)
        self.first_bad = first_bad
        self.reason = "DecompressionFailed" if "DecompressionFailed" in str(self) else "PointNotOnCurve" if "PointNotOnCurve" in str(self) else None


def _records(data, group, encoding, where):
    """bytes-like or uint8 array -> (contiguous uint8 array, n); a trailing partial record is an error"""
    a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    if encoding not in (POINT_BYTES_BE, POINT_BYTES_LE, POINT_BYTES_ARK, POINT_BYTES_ARK_COMPRESSED):
        raise ValueError(f"{where}: unknown encoding {encoding}")
    size = point_record_bytes(group, encoding)
    if a.size % size:
        raise ValueError(f"{where}: {a.size} bytes are not whole records of {size}")
    return a, a.size // size


def _chk_records(rc, where, bad, n_good):
    if rc == ERR_INVALID and int(bad.value) < n_good:
        raise PointBytesError(rc, where, int(bad.value))
    _chk(rc, where)


def _points_from_bytes(group, data, encoding, flags):
    where = "zg_g1_points_from_bytes" if group == 1 else "zg_g2_points_from_bytes"
    a, n = _records(data, group, encoding, where)
    xy = np.zeros((n, 8 * group), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    bad = C.c_size_t(n)
    rc = getattr(_lib, where)(_hb(a) if n else None, C.c_size_t(n), C.c_uint32(encoding), C.c_uint32(flags), _h(xy), _hb(inf), C.byref(bad))
    _chk_records(rc, where, bad, n)
    return xy, inf


def g1_points_from_bytes(data, encoding, flags=0):
    """n records of `encoding` -> (xy (n, 8) Montgomery, inf (n,)), decoded on the device (zg_g1_points_from_bytes); PointBytesError
    with first_bad and reason on a bad record"""
    return _points_from_bytes(1, data, encoding, flags)


def g2_points_from_bytes(data, encoding, flags=0):
    """-> (xy (n, 16), inf (n,)); an identity is written as G2Point.identity() (zg_g2_points_from_bytes)"""
    return _points_from_bytes(2, data, encoding, flags)


def bases_from_bytes(data, encoding, flags=0, window_bits=0, precompute_levels=0, expected_uses=0):
    """Bases.upload over the decoded records, which never leave the device (zg_g1_bases_from_bytes) -> Bases"""
    a, n = _records(data, 1, encoding, "zg_g1_bases_from_bytes")
    cfg = MsmConfig(window_bits, precompute_levels, expected_uses)
    h, bad = C.c_void_p(), C.c_size_t(n)
    rc = _lib.zg_g1_bases_from_bytes(_hb(a) if n else None, C.c_size_t(n), C.c_uint32(encoding), C.c_uint32(flags), C.byref(cfg), C.byref(h), C.byref(bad))
    _chk_records(rc, "zg_g1_bases_from_bytes", bad, n)
    return Bases(h, n)


def _dory_batch_args(polys, device):
    """polys: [(kind, data, aux, shift, bits)] (aux / shift / bits None or 0 where the kind has none); data a numpy array of the kind's
    words — or, device = True, (device address, length in entries) and aux a device address -> the plain arrays of the C call"""
    k = len(polys)
    kinds = np.zeros(k, dtype=np.uint32)
    lens = np.zeros(k, dtype=np.uint64)
    shifts, bits = np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint32)
    data, aux = (C.c_void_p * max(k, 1))(), (C.c_void_p * max(k, 1))()
    keep = []
    for j, (kind, d, a, shift, nbits) in enumerate(polys):
        kinds[j], shifts[j], bits[j] = kind, shift or 0, nbits or 0
        if device:
            data[j], lens[j] = (int(d[0]) or None), int(d[1])
            aux[j] = int(a) if a else None
            continue
        words = _DORY_POLY_WORDS.get(int(kind), 1)  # (an unknown kind is the library's to refuse)
        if not (isinstance(d, np.ndarray) and d.dtype == np.uint64 and d.flags.c_contiguous):  # (an array passed as it is keeps its address)
            d = np.ascontiguousarray(d, dtype=np.uint64)
        keep.append(d)
        lens[j] = d.size // words
        data[j] = d.ctypes.data if d.size else None
        if a is not None:
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
                a = np.ascontiguousarray(a, dtype=np.uint8)
            if a.size < lens[j]:
                raise ValueError("dory_commit_batch: a sign array is shorter than its polynomial")
            keep.append(a)
            aux[j] = a.ctypes.data if a.size else None
    return k, kinds, data, aux, lens, shifts, bits, keep


def dory_commit_batch(key, polys, want_rows=False):
    """DoryCommitmentScheme.commit for every polynomial of `polys` in one call (zg_dory_commit_batch): [(kind, data, aux, shift, bits)]
    -> gt (k, 48), or (gt, [(rows_xy (2^nu_j, 8), rows_inf)] per polynomial) with want_rows. Arrays that are the same object cross once."""
    k, kinds, data, aux, lens, shifts, bits, keep = _dory_batch_args(polys, False)
    gt = np.empty((k, 48), dtype=np.uint64)
    off = np.zeros(k + 1, dtype=np.uint64)
    rows = None
    if want_rows:
        # the row counts follow from the lengths (2^nu, nu = num_vars - (num_vars + 1) / 2)
        total = sum(0 if n == 0 else 1 << (max(int(n).bit_length() - 1, 1) - (max(int(n).bit_length() - 1, 1) + 1) // 2) for n in lens)
        rows = np.zeros((max(total, 1), 9), dtype=np.uint64)
    _chk(_lib.zg_dory_commit_batch(key._h, C.c_size_t(k), kinds.ctypes.data_as(C.c_void_p), data, aux, lens.ctypes.data_as(C.c_void_p),
                                   shifts.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), _h(gt) if k else None, _h(rows),
                                   off.ctypes.data_as(C.c_void_p)), "zg_dory_commit_batch")
    del keep
    if not want_rows:
        return gt
    return gt, [(np.ascontiguousarray(rows[int(off[j]):int(off[j + 1]), :8]), (rows[int(off[j]):int(off[j + 1]), 8] & 1).astype(np.uint8)) for j in range(k)]


def dory_commit_batch_dev(key, polys, d_out_gt, d_out_rows=0, stream=0):
    """the same over device data: polys = [(kind, (device address, entries), aux device address or 0, shift, bits)]; d_out_gt receives
    k * 48 words, d_out_rows (optional) the 9-word row records -> the k + 1 row offsets"""
    k, kinds, data, aux, lens, shifts, bits, _ = _dory_batch_args(polys, True)
    off = np.zeros(k + 1, dtype=np.uint64)
    _chk(_lib.zg_dory_commit_batch_dev(key._h, C.c_size_t(k), kinds.ctypes.data_as(C.c_void_p), data, aux, lens.ctypes.data_as(C.c_void_p),
                                       shifts.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), _d(stream), _d(d_out_gt), _d(d_out_rows),
                                       off.ctypes.data_as(C.c_void_p)), "zg_dory_commit_batch_dev")
    return off


def dory_commit_split():
    """where this thread's last dory_commit_batch spent its time, ms per stage (ZG_OP_DORY_COMMIT_SPLIT; measured only under
    ZG_DORY_COMMIT_TIMES=1, zeros otherwise)"""
    out = np.zeros(5, dtype=np.uint64)
    _chk(_lib.zg_field_op(C.c_int(FR), C.c_int(_abi.ZG_OP_DORY_COMMIT_SPLIT), None, None, _h(out), C.c_size_t(5)), "zg_field_op(ZG_OP_DORY_COMMIT_SPLIT)")
    return dict(zip(("upload", "row_sums", "horner_affine", "miller", "product_final_exp"), (float(x) for x in out.view(np.float64))))


# ---- Dory verifier setup (include/zolt_gpu.h, "Dory verifier setup")
def dory_verifier_setup_levels(n_g1):
    """K + 1 for n_g1 generators, K = floor(log2 n_g1); 0 for 0 (zg_dory_verifier_setup_levels)"""
    return int(_lib.zg_dory_verifier_setup_levels(C.c_size_t(n_g1)))


def _dory_vsetup_split(out, levels):
    return out[:levels].copy(), out[levels:2 * levels].copy(), out[2 * levels:3 * levels].copy()


def dory_verifier_setup(key):
    """DoryVerifierSetup.fromSRS's pairings (src/zkvm/preprocessing.zig:889-973) over a resident key, one launch set
    -> (chi, delta_1r, delta_2r), each (K + 1, 48)"""
    cap = dory_verifier_setup_levels(key.lens()[0])
    out = np.empty((3 * max(cap, 1), 48), dtype=np.uint64)
    levels = C.c_size_t()
    _chk(_lib.zg_dory_verifier_setup(key._h, _h(out), C.c_size_t(cap), C.byref(levels)), "zg_dory_verifier_setup")
    return _dory_vsetup_split(out, int(levels.value))


def dory_verifier_setup_points(g1_xy, g1_inf, g2_xy, g2_inf):
    """the same from host points (flags may be None): no key, no digit table -> (chi, delta_1r, delta_2r)"""
    g1, g1i = _c(g1_xy).reshape(-1, 8), _c(g1_inf, np.uint8)
    g2, g2i = _c(g2_xy).reshape(-1, 16), _c(g2_inf, np.uint8)
    if (g1i is not None and g1i.size < g1.shape[0]) or (g2i is not None and g2i.size < g2.shape[0]):
        raise ValueError("dory_verifier_setup_points: a flag array is shorter than its points")
    cap = dory_verifier_setup_levels(g1.shape[0])
    out = np.empty((3 * max(cap, 1), 48), dtype=np.uint64)
    levels = C.c_size_t()
    _chk(_lib.zg_dory_verifier_setup_points(_h(g1) if g1.shape[0] else None, _hb(g1i), C.c_size_t(g1.shape[0]), _h(g2) if g2.shape[0] else None, _hb(g2i),
                                            C.c_size_t(g2.shape[0]), _h(out), C.c_size_t(cap), C.byref(levels)), "zg_dory_verifier_setup_points")
    return _dory_vsetup_split(out, int(levels.value))


class RegistersRwSession:
    """Stage4GruenProver's dense tables on the device (zg_rrw_*)"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, log_t, rs1, rs2, rd, reg_vals, inc, gamma):
        rs1, rs2, rd = _c(rs1, np.uint8), _c(rs2, np.uint8), _c(rd, np.uint8)
        reg_vals, inc, gamma = _c(reg_vals), _c(inc), _c(gamma)
        T = 1 << log_t
        assert rs1.size == rs2.size == rd.size == T and reg_vals.size == 32 * T and inc.size == 4 * T
        h = C.c_void_p()
        _chk(_lib.zg_rrw_open(C.c_size_t(log_t), _hb(rs1), _hb(rs2), _hb(rd), _h(reg_vals), _h(inc), _h(gamma), C.byref(h)), "zg_rrw_open")
        return cls(h)

    @classmethod
    def open_trace(cls, log_t, rs1, rs2, rd, rd_value, gamma):
        """the same session from the write column alone (zg_rrw_open_trace): the register file and inc are rebuilt on the device"""
        rs1, rs2, rd = _c(rs1, np.uint8), _c(rs2, np.uint8), _c(rd, np.uint8)
        rd_value, gamma = _c(rd_value), _c(gamma)
        T = 1 << log_t
        assert rs1.size == rs2.size == rd.size == rd_value.size == T
        h = C.c_void_p()
        _chk(_lib.zg_rrw_open_trace(C.c_size_t(log_t), _hb(rs1), _hb(rs2), _hb(rd), _h(rd_value), _h(gamma), C.byref(h)), "zg_rrw_open_trace")
        return cls(h)

    def cycles(self):
        return int(_lib.zg_rrw_cycles(self._h))

    def registers(self):
        return int(_lib.zg_rrw_registers(self._h))

    def round_cycle_gruen(self, d_e_out, n_out, d_e_in, n_in):
        a, b = np.empty(4, dtype=np.uint64), np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_rrw_round_cycle_gruen(self._h, _d(d_e_out), C.c_size_t(n_out), _d(d_e_in), C.c_size_t(n_in), _h(a), _h(b)), "zg_rrw_round_cycle_gruen")
        return a, b

    def set_eq(self, eq):
        eq = _c(eq)
        _chk(_lib.zg_rrw_set_eq(self._h, _h(eq), C.c_size_t(eq.size // 4)), "zg_rrw_set_eq")

    def round_address(self, with_e1=False):
        """(e0, e2), or (e0, e1, e2) with the t = 1 value computed from the tables"""
        a, b, c = (np.empty(4, dtype=np.uint64) for _ in range(3))
        _chk(_lib.zg_rrw_round_address(self._h, _h(a), _h(c) if with_e1 else None, _h(b)), "zg_rrw_round_address")
        return (a, c, b) if with_e1 else (a, b)

    def round_cycle(self, with_e1=False):
        """(e0, e2, e3), or (e0, e1, e2, e3)"""
        a, b, c, d = (np.empty(4, dtype=np.uint64) for _ in range(4))
        _chk(_lib.zg_rrw_round_cycle(self._h, _h(a), _h(d) if with_e1 else None, _h(b), _h(c)), "zg_rrw_round_cycle")
        return (a, d, b, c) if with_e1 else (a, b, c)

    def bind_cycle(self, r):
        _chk(_lib.zg_rrw_bind_cycle(self._h, _h(_c(r))), "zg_rrw_bind_cycle")

    def bind_address(self, r):
        _chk(_lib.zg_rrw_bind_address(self._h, _h(_c(r))), "zg_rrw_bind_address")

    def final(self):
        """{val, rd_wa, ra, rs1_ra, rs2_ra, inc, eq}: entry [0][0] of every table"""
        out = np.empty((7, 4), dtype=np.uint64)
        _chk(_lib.zg_rrw_final(self._h, _h(out)), "zg_rrw_final")
        return dict(zip(("val", "rd_wa", "ra", "rs1_ra", "rs2_ra", "inc", "eq"), out))

    def close(self):
        if self._h:
            _chk(_lib.zg_rrw_close(self._h), "zg_rrw_close")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RamRwSession:
    """RamReadWriteCheckingProver's entry list and dense tables behind zg_rwc_*: the cycle-phase walk and the field arithmetic on the
    device, the address-phase walk on the host inside the library"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, log_k, log_t, cycle, address, val_coeff, prev_val, next_val, inc, val_init, r_cycle):
        cycle, address = _c(cycle, np.uint32), _c(address, np.uint32)
        val_coeff, prev_val, next_val = _c(val_coeff), _c(prev_val), _c(next_val)
        inc, val_init, r_cycle = _c(inc), _c(val_init), _c(r_cycle)
        n = cycle.size
        assert address.size == val_coeff.size == prev_val.size == next_val.size == n
        assert inc.size == 4 << log_t and val_init.size == 4 << log_k and r_cycle.size == 4 * log_t
        h = C.c_void_p()
        _chk(_lib.zg_rwc_open(C.c_size_t(log_k), C.c_size_t(log_t), C.c_size_t(n), _hb(cycle), _hb(address), _h(val_coeff), _h(prev_val), _h(next_val),
                              _h(inc), _h(val_init), _h(r_cycle), C.byref(h)), "zg_rwc_open")
        return cls(h)

    @classmethod
    def open_writes(cls, log_k, log_t, cycle, address, val_coeff, prev_val, next_val, is_write, val_init, r_cycle):
        """zg_rwc_open_writes: inc is formed on the device from the entries marked as writes"""
        cycle, address, is_write = _c(cycle, np.uint32), _c(address, np.uint32), _c(is_write, np.uint8)
        val_coeff, prev_val, next_val = _c(val_coeff), _c(prev_val), _c(next_val)
        val_init, r_cycle = _c(val_init), _c(r_cycle)
        n = cycle.size
        assert address.size == val_coeff.size == prev_val.size == next_val.size == is_write.size == n
        assert val_init.size == 4 << log_k and r_cycle.size == 4 * log_t
        h = C.c_void_p()
        _chk(_lib.zg_rwc_open_writes(C.c_size_t(log_k), C.c_size_t(log_t), C.c_size_t(n), _hb(cycle), _hb(address), _h(val_coeff), _h(prev_val),
                                     _h(next_val), _hb(is_write), _h(val_init), _h(r_cycle), C.byref(h)), "zg_rwc_open_writes")
        return cls(h)

    def entries(self):
        return int(_lib.zg_rwc_entries(self._h))

    def cycles(self):
        return int(_lib.zg_rwc_cycles(self._h))

    def round_cycle(self, d_e_out, n_out, d_e_in, n_in, gamma):
        a, b = np.empty(4, dtype=np.uint64), np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_rwc_round_cycle(self._h, _d(d_e_out), C.c_size_t(n_out), _d(d_e_in), C.c_size_t(n_in), _h(_c(gamma)), _h(a), _h(b)), "zg_rwc_round_cycle")
        return a, b

    def bind_cycle(self, r):
        _chk(_lib.zg_rwc_bind_cycle(self._h, _h(_c(r))), "zg_rwc_bind_cycle")

    def round_address(self, addr_round, challenges, gamma):
        ch = _c(np.asarray(challenges, dtype=np.uint64).reshape(-1, 4))
        assert ch.shape[0] == addr_round
        a, b = np.empty(4, dtype=np.uint64), np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_rwc_round_address(self._h, C.c_size_t(addr_round), _h(ch) if addr_round else None, _h(_c(gamma)), _h(a), _h(b)), "zg_rwc_round_address")
        return a, b

    def bind_address(self, addr_round, r):
        _chk(_lib.zg_rwc_bind_address(self._h, C.c_size_t(addr_round), _h(_c(r))), "zg_rwc_bind_address")

    def opening(self, r_address, r_cycle):
        out = np.empty((3, 4), dtype=np.uint64)
        ra, rc = _c(np.asarray(r_address, dtype=np.uint64).reshape(-1, 4)), _c(np.asarray(r_cycle, dtype=np.uint64).reshape(-1, 4))
        _chk(_lib.zg_rwc_opening(self._h, _h(ra) if ra.size else None, _h(rc) if rc.size else None, _h(out)), "zg_rwc_opening")
        return out[0], out[1], out[2]

    def cycle_scalars(self):
        a, b = np.empty(4, dtype=np.uint64), np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_rwc_cycle_scalars(self._h, _h(a), _h(b)), "zg_rwc_cycle_scalars")
        return a, b

    def read_entries(self, coefficients=True):
        """-> (cycle, address, ra_coeff, val_coeff, prev_val, next_val) arrays of the current list"""
        n = self.entries()
        cyc, adr = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        ra, val = np.empty((n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)
        prev, nxt = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        _chk(_lib.zg_rwc_read_entries(self._h, _hb(cyc), _hb(adr), _h(ra) if coefficients else None, _h(val) if coefficients else None, _h(prev), _h(nxt)),
             "zg_rwc_read_entries")
        return cyc, adr, ra, val, prev, nxt

    def close(self):
        if self._h:
            _chk(_lib.zg_rwc_close(self._h), "zg_rwc_close")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedSumcheckSession:
    """Sumcheck(F).Prover over a table sharded across the devices bound by init_devices (zg_sumcheck_*_sharded)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, evals, layout=SC_HIGH_HALF):
        e = _c(evals)
        h = C.c_void_p()
        _chk(_lib.zg_sumcheck_open_sharded(_h(e), C.c_size_t(e.size // 4), C.c_int(layout), C.byref(h)), "zg_sumcheck_open_sharded")
        return cls(h)

    def shards(self):
        return int(_lib.zg_sumcheck_shards(self._h))

    def round_sums(self):
        g0 = np.empty(4, dtype=np.uint64)
        g1 = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_round_sums_sharded(self._h, _h(g0), _h(g1)), "zg_sumcheck_round_sums_sharded")
        return g0, g1

    def bind(self, r):
        _chk(_lib.zg_sumcheck_bind_sharded(self._h, _h(_c(r))), "zg_sumcheck_bind_sharded")

    def __len__(self):
        return int(_lib.zg_sumcheck_len_sharded(self._h))

    def final(self):
        out = np.empty(4, dtype=np.uint64)
        _chk(_lib.zg_sumcheck_final_sharded(self._h, _h(out)), "zg_sumcheck_final_sharded")
        return out

    def close(self):
        if self._h:
            _chk(_lib.zg_sumcheck_close_sharded(self._h), "zg_sumcheck_close_sharded")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
