"""The section "field vectors (device)" of include/zolt_gpu.h on the GPU, for Fr and Fp, bit for bit against the integer model
(tests/field_vectors_model.py): the batch inverse at every length through two workgroup tiles and across the grid-stride wrap, with zeros
wherever the kernel groups elements, in place, host and device forms; zg_field_op_dev and zg_field_scale_dev against zg_field_op; the inner
product, Horner's rule and the resident dense evaluation at the sizes where a chunk, a wave, a tile or the grid ends; a call enqueued
behind a producer on a stream of its own; the refusals; the Python and C++ mirrors. The tile and the elements per lane come from
include/zolt_gpu_internal.h. One model result per field is computed once and shared.

    python -m pytest tests/test_gpu_field_vectors.py -m gpu -q --durations=0"""
import os
import subprocess

import numpy as np
import pytest

from tests import field_vectors_model as M

pytestmark = pytest.mark.gpu
ROOT = M.ROOT
E, TILE = M.E, M.TILE
N = 4 * TILE + 3  # the longest vector: with ZG_FV_BLOCKS=2 the batch inverse and Horner wrap at 2 * TILE, the inner product at 512
FIELDS = [pytest.param(M.FR, id="fr"), pytest.param(M.FP, id="fp")]
CAPS = [pytest.param(None, id="default_grid"), pytest.param("2", id="two_workgroups")]
SIZES = sorted({0, 1, E - 1, E, E + 1, 63, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, N})


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


class Data:
    """one field's shared vectors: values, their limbs, the element-wise inverses, resident copies (read only after construction)"""

    def __init__(self, zl, field):
        self.field, self.mod = field, M.MODS[field]
        vals = M.random_values(self.mod, N, 40 + field)
        vals[:8] = M.edge_values(self.mod)
        for z in (5, 255, 256, TILE - 1, TILE, 2 * TILE, N - 1, *range(300, N, 97)):
            vals[z] = 0
        self.a, self.b = vals, M.random_values(self.mod, N, 50 + field)
        self.a_l, self.b_l = M.to_limbs(self.a, self.mod), M.to_limbs(self.b, self.mod)
        self.inv_l = M.to_limbs(M.batch_inverse(self.a, self.mod), self.mod)
        self.d_a, self.d_b = zl.DeviceBuffer.from_host(self.a_l), zl.DeviceBuffer.from_host(self.b_l)


@pytest.fixture(scope="module")
def data(zl):
    made = {}

    def get(field):
        if field not in made:
            made[field] = Data(zl, field)
        return made[field]

    return get


@pytest.fixture
def cap(request, monkeypatch):
    """ZG_FV_BLOCKS for the test's calls (the library reads it at every call)"""
    def set_cap(value):
        if value is None:
            monkeypatch.delenv("ZG_FV_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("ZG_FV_BLOCKS", value)
    return set_cap


SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _sentinel_buffer(zl, n):
    return zl.DeviceBuffer.from_host(np.full((max(n, 1), 4), SENTINEL, dtype=np.uint64))


def _dev_inverse(zl, field, limbs):
    """zg_field_batch_inverse_dev out of place -> (n, 4); nothing past n is written"""
    n = len(limbs)
    d_in, d_out = zl.DeviceBuffer.from_host(limbs), _sentinel_buffer(zl, n + 1)
    zl.field_batch_inverse_dev(field, d_in.ptr, d_out.ptr, n)
    got = d_out.to_host().reshape(-1, 4)
    assert np.all(got[n:] == SENTINEL)
    d_in.free()
    d_out.free()
    return got[:n]


# ---- batch inverse
@pytest.mark.parametrize("field", FIELDS)
def test_batch_inverse_at_every_length_through_two_tiles(zl, data, field):
    """n = 0 .. 2 * tile + 1 on prefixes of one vector (the value is element-wise, so the expected result is the prefix of one model run);
    nothing past n is written"""
    d = data(field)
    top = 2 * TILE + 1
    d_out = _sentinel_buffer(zl, top + 1)
    for n in range(top + 1):
        zl.field_batch_inverse_dev(field, d.d_a.ptr, d_out.ptr, n)
        got = d_out.to_host().reshape(-1, 4)
        assert np.array_equal(got[:n], d.inv_l[:n]), n
        assert np.all(got[n:] == SENTINEL), n
    d_out.free()


@pytest.mark.parametrize("field", FIELDS)
def test_batch_inverse_across_the_grid_stride_wrap(zl, data, field, cap):
    """two workgroups: one below, at and one above the size where a workgroup takes its second tile, and a third trip"""
    d = data(field)
    cap("2")
    for n in (2 * TILE - 1, 2 * TILE, 2 * TILE + 1, N):
        assert np.array_equal(_dev_inverse(zl, field, d.a_l[:n]), d.inv_l[:n]), n
    cap("1")
    assert np.array_equal(_dev_inverse(zl, field, d.a_l[:2 * TILE + 1]), d.inv_l[:2 * TILE + 1])


def _zero_patterns():
    n = 3 * TILE
    lane = [7 + 256 * k for k in range(E)]                                    # everything lane 7 of the first tile owns
    wave = [TILE + 256 * k + t for k in range(E) for t in range(64, 128)]     # everything wave 1 of the second tile owns
    return n, {"first": [0], "last": [n - 1], "lane": lane, "wave": wave, "every": list(range(n)), "alternating": list(range(0, n, 2)),
               "all_but_one_per_lane": [i for i in range(n) if (i % TILE) // 256 != 3]}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("pattern", ["first", "last", "lane", "wave", "every", "alternating", "all_but_one_per_lane"])
def test_batch_inverse_zero_placement(zl, data, field, pattern):
    d = data(field)
    n, pats = _zero_patterns()
    # the vector is b[i % 256] (no zero among them), so 256 model inverses serve every pattern
    idx = np.arange(n) % 256
    limbs, want = d.b_l[idx].copy(), M.to_limbs(M.batch_inverse(d.b[:256], d.mod), d.mod)[idx].copy()
    limbs[pats[pattern]] = 0
    want[pats[pattern]] = 0
    assert np.array_equal(_dev_inverse(zl, field, limbs), want)
    assert np.array_equal(zl.field_batch_inverse(field, limbs), want)


@pytest.mark.parametrize("field", FIELDS)
def test_batch_inverse_values_in_place_and_both_forms(zl, data, field):
    """1, -1, 2 and random values; out == a equal to out of place; the host-pointer and _dev forms agree; the words of ZG_OP_INV"""
    d = data(field)
    one, minus_one, two = M.to_limbs([1, d.mod - 1, 2], d.mod)
    n = 2 * TILE + 77
    limbs = d.a_l[:n].copy()
    limbs[8:11] = [one, minus_one, two]
    host = zl.field_batch_inverse(field, limbs)
    assert np.array_equal(host[8], one) and np.array_equal(host[9], minus_one) and np.array_equal(host[10], M.to_limbs([(d.mod + 1) // 2], d.mod)[0])
    assert np.array_equal(host, zl.field_op(field, zl.OP_INV, limbs))  # Fermat, one exponentiation per element: word for word
    assert np.array_equal(_dev_inverse(zl, field, limbs), host)
    buf = zl.DeviceBuffer.from_host(limbs)
    zl.field_batch_inverse_dev(field, buf.ptr, buf.ptr, n)
    assert np.array_equal(buf.to_host().reshape(-1, 4)[:n], host)
    buf.free()
    same = limbs.copy()
    assert zl._lib.zg_field_batch_inverse(field, same.ctypes.data, same.ctypes.data, n) == 0 and np.array_equal(same, host)  # host form in place
    # the known answer of the reference's own test: a * a^-1 = 1 for 2, 3, 5
    three = M.to_limbs([2, 3, 5], d.mod)
    assert np.array_equal(zl.field_op(field, zl.OP_MUL, three, zl.field_batch_inverse(field, three)), np.tile(one, (3, 1)))


@pytest.mark.parametrize("field", FIELDS)
def test_the_reference_loop_differs_only_when_the_first_element_is_zero(zl, field):
    """the divergence the header states, on the device: equal to BatchOps.batchInverse restated (model) whenever a[0] != 0, element-wise
    where the reference zeroes everything"""
    mod = M.MODS[field]
    for name, v in M.generator_vectors(mod):
        got = M.from_limbs(zl.field_batch_inverse(field, M.to_limbs(v, mod)), mod)
        assert got == M.batch_inverse(v, mod), name
        if v[0] != 0:
            assert got == M.reference_batch_inverse(v, mod), name


# ---- element-wise ops and the scale on device pointers
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", CAPS)
def test_field_op_dev_and_scale_dev_match_the_host_forms(zl, data, field, grid, cap):
    d = data(field)
    cap(grid)
    sizes = (1, 255, 256, 257) if grid is None else (511, 512, 513, 1030)
    s = d.b_l[3]
    for n in sizes:
        d_out = _sentinel_buffer(zl, n + 1)
        for op in range(8):
            two = op <= zl.OP_SUB
            want = zl.field_op(field, op, d.a_l[:n], d.b_l[:n] if two else None)
            zl.field_op_dev(field, op, d.d_a.ptr, d.d_b.ptr if two else 0, d_out.ptr, n)  # unary ops: d_b = NULL
            got = d_out.to_host().reshape(-1, 4)
            assert np.array_equal(got[:n], want) and np.all(got[n:] == SENTINEL), (op, n)
            inplace = zl.DeviceBuffer.from_host(d.a_l[:n])
            zl.field_op_dev(field, op, inplace.ptr, d.d_b.ptr if two else 0, inplace.ptr, n)
            assert np.array_equal(inplace.to_host().reshape(-1, 4)[:n], want), (op, n)
            inplace.free()
        want = zl.field_op(field, zl.OP_MUL, d.a_l[:n], np.tile(s, (n, 1)))
        zl.field_scale_dev(field, d.d_a.ptr, n, s, d_out.ptr)
        got = d_out.to_host().reshape(-1, 4)
        assert np.array_equal(got[:n], want) and np.all(got[n:] == SENTINEL), n
        inplace = zl.DeviceBuffer.from_host(d.a_l[:n])
        zl.field_scale_dev(field, inplace.ptr, n, s, inplace.ptr)
        assert np.array_equal(inplace.to_host().reshape(-1, 4)[:n], want), n
        inplace.free()
        d_out.free()
    if field == M.FR:
        assert np.array_equal(want, zl.fr_scale(d.a_l[:sizes[-1]], s))


# ---- inner product, Horner, dense evaluation
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", CAPS)
def test_inner_product(zl, data, field, grid, cap):
    d = data(field)
    cap(grid)
    for n in SIZES:
        want = M.to_limbs([M.inner_product(d.a[:n], d.b[:n], d.mod)], d.mod)[0]
        assert np.array_equal(zl.field_inner_product_dev(field, d.d_a.ptr, d.d_b.ptr, n), want), n
        if n in (0, 1, E + 1, 65, 513, TILE + 1, N):
            assert np.array_equal(zl.field_inner_product(field, d.a_l[:n], d.b_l[:n]), want), n
    sq = M.to_limbs([M.inner_product(d.b, d.b, d.mod)], d.mod)[0]
    assert np.array_equal(zl.field_inner_product_dev(field, d.d_b.ptr, d.d_b.ptr, N), sq)  # the same table twice
    assert np.array_equal(zl.field_inner_product(field, d.b_l, d.b_l), sq)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", CAPS)
def test_horner(zl, data, field, grid, cap):
    d = data(field)
    cap(grid)
    for x in (0, 1, d.mod - 1, M.random_values(d.mod, 1, 61 + field)[0]):
        xl = M.to_limbs([x], d.mod)[0]
        for n in SIZES:
            want = M.to_limbs([M.horner(d.b[:n], x, d.mod)], d.mod)[0]
            assert np.array_equal(zl.field_horner_dev(field, d.d_b.ptr, n, xl), want), (x, n)
            if n in (0, 1, E + 1, TILE + 1, N):
                assert np.array_equal(zl.field_horner(field, d.b_l[:n], xl), want), (x, n)
    # zeros among the coefficients, a zero leading coefficient included
    xl = M.to_limbs([3], d.mod)[0]
    assert np.array_equal(zl.field_horner_dev(field, d.d_a.ptr, N, xl), M.to_limbs([M.horner(d.a, 3, d.mod)], d.mod)[0])


@pytest.mark.parametrize("grid", CAPS)
def test_dense_evaluate_dev_matches_the_host_pointer_form(zl, data, grid, cap):
    d = data(M.FR)
    cap(grid)
    for num_vars in range(13):
        n = 1 << num_vars
        point = d.a_l[1000:1000 + num_vars]
        got = zl.fr_dense_evaluate_dev(d.d_b.ptr, point)
        assert np.array_equal(got, zl.fr_dense_evaluate(d.b_l[:n], point)), num_vars
    # the multilinear extension at a corner is the table entry: index bit j pairs with point[j]
    corner = M.to_limbs([1, 0, 1, 1], M.R)
    assert np.array_equal(zl.fr_dense_evaluate_dev(d.d_b.ptr, corner), d.b_l[0b1101])


# ---- streams, refusals, mirrors
@pytest.mark.parametrize("field", FIELDS)
def test_a_call_enqueued_behind_a_producer_on_another_stream_reads_its_output(zl, data, field):
    """on a stream of the caller's: ZG_OP_INV (Fermat, slow) writes a table, the batch inverse enqueued behind it inverts it back, a scale
    and an inner product follow — every step reads what the step before it wrote"""
    import torch
    d = data(field)
    n = N
    work = torch.cuda.Stream()
    d_t, d_u = zl.DeviceBuffer.from_host(np.zeros((n, 4), dtype=np.uint64)), _sentinel_buffer(zl, n)
    zl.field_op_dev(field, zl.OP_INV, d.d_b.ptr, 0, d_t.ptr, n, stream=work.cuda_stream)       # producer
    zl.field_batch_inverse_dev(field, d_t.ptr, d_u.ptr, n, stream=work.cuda_stream)             # b again (b has no zero)
    zl.field_scale_dev(field, d_u.ptr, n, d.b_l[0], d_u.ptr, stream=work.cuda_stream)
    got = zl.field_inner_product_dev(field, d_u.ptr, d_t.ptr, n, stream=work.cuda_stream)       # sum of b0 * b[i] / b[i] = n * b0
    assert np.array_equal(got, M.to_limbs([n * d.b[0]], d.mod)[0])
    assert np.array_equal(d_u.to_host().reshape(-1, 4)[:n], zl.field_op(field, zl.OP_MUL, d.b_l, np.tile(d.b_l[0], (n, 1))))
    d_t.free()
    d_u.free()


def test_refusals_and_their_error_text(zl, data):
    d = data(M.FR)
    out4 = np.zeros(4, dtype=np.uint64)
    L, p4 = zl._lib, out4.ctypes.data
    a, b = d.d_a.ptr, d.d_b.ptr
    scratch = zl.DeviceBuffer(64 * 32)
    o = scratch.ptr

    def refused(rc, text):
        assert rc == zl.ERR_INVALID, rc
        assert text in zl.last_error(), zl.last_error()

    # an output that overlaps an input without being it
    refused(L.zg_field_batch_inverse_dev(0, a, a + 32, 8, None), "overlaps")
    refused(L.zg_field_batch_inverse_dev(0, a + 32, a, 8, None), "overlaps")
    refused(L.zg_field_batch_inverse_dev(0, a, a + 7 * 32, 8, None), "overlaps")
    assert L.zg_field_batch_inverse_dev(0, a, o, 8, None) == 0 and L.zg_field_batch_inverse_dev(0, o, o + 8 * 32, 8, None) == 0  # adjacent is fine
    refused(L.zg_field_op_dev(0, zl.OP_ADD, a, b, b, 8, None), "overlaps")
    refused(L.zg_field_op_dev(0, zl.OP_ADD, a, b, b + 32, 8, None), "overlaps")
    refused(L.zg_field_op_dev(0, zl.OP_NEG, a, None, a + 32, 8, None), "overlaps")
    assert L.zg_field_op_dev(0, zl.OP_NEG, o, o + 32, o, 8, None) == 0  # a unary op ignores b
    refused(L.zg_field_scale_dev(0, a, 8, p4, a + 64, None), "overlaps")
    host = d.a_l[:16].copy()
    refused(L.zg_field_batch_inverse(0, host.ctypes.data, host.ctypes.data + 32, 8), "overlaps")
    # fields and ops
    for field in (-1, 2):
        refused(L.zg_field_batch_inverse_dev(field, a, o, 8, None), "unknown field")
        refused(L.zg_field_batch_inverse(field, host.ctypes.data, host.ctypes.data, 8), "unknown field")
        refused(L.zg_field_inner_product_dev(field, a, b, 8, None, p4), "unknown field")
        refused(L.zg_field_horner_dev(field, a, 8, p4, None, p4), "unknown field")
        refused(L.zg_field_scale_dev(field, a, 8, p4, o, None), "unknown field")
        refused(L.zg_field_op_dev(field, zl.OP_ADD, a, b, o, 8, None), "unknown field")
    for op in (-1, 8, zl.OP_MUL29, zl.OP_INV_SAFEGCD, zl.OP_FP2_MUL, zl.OP_FP12_MUL, zl.OP_DORY_V1, zl.OP_FP12W_MUL):
        refused(L.zg_field_op_dev(1, op, a, b, o, 12, None), "ZG_OP_MUL .. ZG_OP_TO_MONT")  # the self-test codes stay with zg_field_op
    # null data with n > 0, no room for a scalar
    refused(L.zg_field_op_dev(0, zl.OP_ADD, a, None, o, 8, None), "null")
    refused(L.zg_field_op_dev(0, zl.OP_ADD, None, b, o, 8, None), "null")
    refused(L.zg_field_scale_dev(0, a, 8, None, o, None), "null")
    refused(L.zg_field_batch_inverse_dev(0, a, None, 8, None), "null")
    refused(L.zg_field_batch_inverse(0, None, host.ctypes.data, 8), "null")
    refused(L.zg_field_inner_product_dev(0, a, None, 8, None, p4), "null")
    refused(L.zg_field_inner_product(0, host.ctypes.data, None, 8, p4), "null")
    refused(L.zg_field_inner_product_dev(0, a, b, 8, None, None), "no output")
    refused(L.zg_field_horner_dev(0, a, 8, None, None, p4), "null")
    refused(L.zg_field_horner(0, None, 8, p4, p4), "null")
    refused(L.zg_field_horner(0, host.ctypes.data, 8, p4, None), "no output")
    refused(L.zg_fr_dense_evaluate_dev(None, 0, None, None, p4), "zg_fr_dense_evaluate_dev")
    refused(L.zg_fr_dense_evaluate_dev(a, 3, None, None, p4), "zg_fr_dense_evaluate_dev")
    refused(L.zg_fr_dense_evaluate_dev(a, 31, host.ctypes.data, None, p4), "zg_fr_dense_evaluate_dev")
    # n == 0: fine without data, and the scalars are zero
    assert L.zg_field_op_dev(0, zl.OP_ADD, None, None, None, 0, None) == 0 and L.zg_field_scale_dev(1, None, 0, None, None, None) == 0
    assert L.zg_field_batch_inverse_dev(1, None, None, 0, None) == 0 and L.zg_field_batch_inverse(0, None, None, 0) == 0
    for call in (lambda: L.zg_field_inner_product_dev(0, None, None, 0, None, p4), lambda: L.zg_field_inner_product(1, None, None, 0, p4),
                 lambda: L.zg_field_horner_dev(1, None, 0, None, None, p4), lambda: L.zg_field_horner(0, None, 0, None, p4)):
        out4[:] = 7
        assert call() == 0 and not out4.any()
    scratch.free()


def test_python_mirror_on_the_reference_known_answers(zl):
    """api.BatchOps on src/field/mod.zig:1452-1494 (and the inner product of :1445-1449)"""
    from zolt_amd import api
    B = api.BatchOps
    fr = lambda vs: np.stack([api.fr_from_int(v) for v in vs])  # noqa: E731
    a, b = fr([1, 2, 3, 4]), fr([5, 6, 7, 8])
    assert np.array_equal(B.batchAdd(a, b), fr([6, 8, 10, 12]))
    assert np.array_equal(B.batchSub(b, a), fr([4, 4, 4, 4]))
    assert np.array_equal(B.batchMul(a, b), fr([5, 12, 21, 32]))
    assert np.array_equal(B.batchMulScalar(a, api.fr_from_int(9)), fr([9, 18, 27, 36]))
    assert np.array_equal(B.batchSquare(a), fr([1, 4, 9, 16]))
    assert np.array_equal(B.innerProduct(a, b), api.fr_from_int(70)) and np.array_equal(B.multiScalarMulLinear(a, b), api.fr_from_int(70))
    assert np.array_equal(B.hornerEval(a, api.fr_from_int(2)), api.fr_from_int(49))
    assert np.array_equal(B.innerProduct(fr(range(1, 9)), fr(range(10, 18))), api.fr_from_int(528))
    nz = fr([2, 3, 5])
    assert np.array_equal(B.batchMul(nz, B.batchInverse(nz)), fr([1, 1, 1]))
    assert np.array_equal(B.batchInverse(fr([0, 2, 0])), fr([0, pow(2, -1, api.R_MOD), 0]))  # element-wise where the reference gives zeros
    none = np.zeros((0, 4), dtype=np.uint64)
    assert not B.hornerEval(none, api.fr_from_int(2)).any() and not B.innerProduct(none, none).any() and B.batchInverse(none).shape == (0, 4)
    fp = lambda vs: M.to_limbs(list(vs), M.P)  # noqa: E731
    assert np.array_equal(B.innerProduct(fp([1, 2, 3, 4]), fp([5, 6, 7, 8]), field=zl.FP), fp([70])[0])
    assert np.array_equal(B.hornerEval(fp([1, 2, 3, 4]), fp([2])[0], field=zl.FP), fp([49])[0])


def test_cpp_mirror_prints_what_the_python_mirror_computes(zl, tmp_path):
    """tests/cpp/test_field_vectors_mirror.cpp: zolt::BatchOps and zolt::BatchOps::Dev on the known answers and on a vector with zeros"""
    from zolt_amd import api
    exe = str(tmp_path / "test_field_vectors_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_field_vectors_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-400:] + res.stderr[-400:]
    lines = dict(l.split(" ", 1) for l in res.stdout.strip().splitlines())
    assert lines.pop("known_answers") == "ok"
    n = 600
    v = np.stack([api.fr_from_int(0 if i % 7 == 3 else i * i + 3) for i in range(n)])
    w = np.stack([api.fr_from_int(2 * i + 1) for i in range(n)])
    hx = lambda words: "".join("%016x" % int(x) for x in np.asarray(words, dtype=np.uint64).reshape(-1))  # noqa: E731
    B = api.BatchOps
    want = {"inverse": hx(B.batchInverse(v)), "inner": hx(B.innerProduct(v, w)), "horner": hx(B.hornerEval(v, api.fr_from_int(5))),
            "scaled": hx(B.batchMulScalar(v, api.fr_from_int(11))), "sum": hx(B.batchAdd(v, w))}
    for key, val in want.items():
        assert lines["host_" + key] == val, key
        assert lines["dev_" + key] == val, key
