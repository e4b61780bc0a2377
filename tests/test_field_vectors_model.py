"""The section "field vectors (device)" without a GPU: the model (tests/field_vectors_model.py) on the reference's own known answers, the
reference's batchInverse loop against the element-wise value the entry points compute, the lane functions of the kernels
(zolt_amd/csrc/field_vec.hip.h) compiled for the host and run over the generator's vectors — once as they are, once as a stand-alone
program under -fsanitize=address,undefined — and the section's symbols, feature bit and generated bindings.

    python -m pytest tests/test_field_vectors_model.py -q --durations=0"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import field_vectors_model as M

ROOT = M.ROOT
needs_hipcc = pytest.mark.skipif(not os.path.exists(M.HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

SECTION = ["zg_field_op_dev", "zg_field_scale_dev", "zg_field_batch_inverse", "zg_field_batch_inverse_dev", "zg_field_inner_product",
           "zg_field_inner_product_dev", "zg_field_horner", "zg_field_horner_dev", "zg_fr_dense_evaluate_dev"]


# ---- the model
def test_the_reference_known_answers():
    """src/field/mod.zig:1421-1494: inner product 70, Horner 49, inner product 528, a * a^-1 = 1 for 2, 3, 5"""
    for mod in M.MODS:
        a, b = [1, 2, 3, 4], [5, 6, 7, 8]
        assert M.inner_product(a, b, mod) == 70
        assert M.horner(a, 2, mod) == 49
        assert M.inner_product(list(range(1, 9)), list(range(10, 18)), mod) == 528
        for inv in (M.batch_inverse, M.reference_batch_inverse):
            got = inv([2, 3, 5], mod)
            assert [x * y % mod for x, y in zip([2, 3, 5], got)] == [1, 1, 1]
        assert M.horner([], 7, mod) == 0 and M.inner_product([], [], mod) == 0 and M.batch_inverse([], mod) == []


def test_representation_round_trip():
    for mod in M.MODS:
        vals = M.edge_values(mod) + [0]
        limbs = M.to_limbs(vals, mod)
        assert M.from_limbs(limbs, mod) == vals
    # Montgomery one: the low words zolt_amd/csrc/field.hip.h carries
    assert int(M.to_limbs([1], M.R)[0][0]) == 0xac96341c4ffffffb and int(M.to_limbs([1], M.P)[0][0]) == 0xd35d438dc58f0d9d


def test_reference_loop_equals_the_element_wise_value_unless_the_first_element_is_zero():
    """the divergence include/zolt_gpu.h states: BatchOps.batchInverse seeds products[0] = a[0] unguarded (:1241), so a[0] = 0 zeroes every
    output; on every other vector — zeros in any later position included — the loop is the element-wise value"""
    seen_equal = seen_differ = 0
    for mod in M.MODS:
        for name, v in M.generator_vectors(mod):
            loop, elem = M.reference_batch_inverse(v, mod), M.batch_inverse(v, mod)
            assert all(x * y % mod == (1 if x else 0) for x, y in zip(v, elem)), name
            if v[0] != 0:
                assert loop == elem, name
                seen_equal += 1
            else:
                assert loop == [0] * len(v), name
                assert (loop != elem) == any(x != 0 for x in v[1:]), name
                seen_differ += loop != elem
    assert seen_equal >= 50 and seen_differ >= 10
    # the vectors that matter are there: a non-zero first element with zeros elsewhere, a zero first element with non-zero ones elsewhere
    names = [n for n, _ in M.generator_vectors(M.R)]
    for want in ("n17_last", "n17_group", "n17_all_but_first", "n17_first", "n17_first_group", "n9_alternating", "n9_odd", "n8_slot7"):
        assert want in names, want


# ---- the lane functions on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return M.compile_host(str(tmp_path_factory.mktemp("field_vec_host") / "field_vec_host"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return M.compile_host(str(tmp_path_factory.mktemp("field_vec_host_san") / "field_vec_host_san"), extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _groups(mod, seed):
    """groups of E elements: zeros in every single position, in every pair of neighbours, everywhere, nowhere; edge and random values"""
    E = M.E
    rnd = M.random_values(mod, 4 * E, seed)
    groups = [rnd[:E], (M.edge_values(mod) * E)[:E], [1] * E, [mod - 1] * E, [0] * E]
    for k in range(E):
        g = list(rnd[E:2 * E])
        g[k] = 0
        groups.append(g)
        g = list(rnd[2 * E:3 * E])
        g[k] = g[(k + 1) % E] = 0
        groups.append(g)
        g = [0] * E
        g[k] = rnd[3 * E + k]
        groups.append(g)
    return groups


def _check_lane_functions(run):
    outs = []
    for field, mod in enumerate(M.MODS):
        groups = _groups(mod, 90 + field)
        flat = [v for g in groups for v in g]
        got = run(field, M.OP_INV_GROUPS, M.to_limbs(flat, mod))
        assert np.array_equal(got, M.to_limbs(M.batch_inverse(flat, mod), mod))
        outs.append(got)
        for x in (0, 1, mod - 1, M.random_values(mod, 1, 7)[0]):
            xl = M.to_limbs([x], mod)[0]
            got = run(field, M.OP_HORNER_CHUNKS, M.to_limbs(flat, mod), xl)
            assert np.array_equal(got, M.to_limbs([M.horner(g, x, mod) for g in groups], mod)), x
            outs.append(got)
            for n in (0, 1, M.E - 1, M.E, M.E + 1, 3 * M.E + 2, len(flat)):
                got = run(field, M.OP_HORNER, M.to_limbs(flat[:n], mod), xl)
                assert np.array_equal(got, M.to_limbs([M.horner(flat[:n], x, mod)], mod)), (x, n)
                outs.append(got)
    return outs


@needs_hipcc
def test_lane_functions_on_the_host(harness):
    """fv_inv_group over groups with zeros in every position, fv_horner_chunk, and the ladder / weight composition of a whole Horner"""
    _check_lane_functions(harness)


@needs_hipcc
def test_lane_functions_under_asan_and_ubsan(harness, harness_san):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined: its outputs are the plain build's"""
    for a, b in zip(_check_lane_functions(harness_san), _check_lane_functions(harness)):
        assert np.array_equal(a, b)


# ---- the section in the header, the library and the bindings
def test_section_symbols_feature_bit_and_bindings():
    from zolt_amd import _abi, lib
    hdr = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert re.search(r"#define ZG_FEATURE_FIELD_VECTORS 2048u\b", hdr) and "field vectors (device)" in hdr
    assert re.search(r"#define ZG_ABI_MINOR 11\b", hdr)
    assert "products[0] = a[0]" in hdr and ":1241" in hdr  # the divergence from the reference is stated where the entry points are declared
    assert _abi.ZG_FEATURE_FIELD_VECTORS == 2048 and _abi.ZG_FV_TILE == 256 * _abi.ZG_FV_E == M.TILE
    assert lib.abi_features() & _abi.ZG_FEATURE_FIELD_VECTORS and lib.abi_version() == (1, 11)
    for name in SECTION:
        assert name in _abi.PROTOS and hasattr(lib._lib, name), name
    v, z, i = C.c_void_p, C.c_size_t, C.c_int
    assert _abi.PROTOS["zg_field_op_dev"] == (i, [i, i, v, v, v, z, v])
    assert _abi.PROTOS["zg_field_scale_dev"] == (i, [i, v, z, v, v, v])
    assert _abi.PROTOS["zg_field_batch_inverse"] == (i, [i, v, v, z]) and _abi.PROTOS["zg_field_batch_inverse_dev"] == (i, [i, v, v, z, v])
    assert _abi.PROTOS["zg_field_inner_product"] == (i, [i, v, v, z, v]) and _abi.PROTOS["zg_field_inner_product_dev"] == (i, [i, v, v, z, v, v])
    assert _abi.PROTOS["zg_field_horner"] == (i, [i, v, z, v, v]) and _abi.PROTOS["zg_field_horner_dev"] == (i, [i, v, z, v, v, v])
    assert _abi.PROTOS["zg_fr_dense_evaluate_dev"] == (i, [v, z, v, v, v])
    zig = open(os.path.join(ROOT, "zig", "gpu", "ffi.zig")).read()
    for name in SECTION:
        assert f"pub extern fn {name}(" in zig, name
    assert "pub const FEATURE_FIELD_VECTORS" in zig


def test_mirrors_carry_the_reference_names():
    from zolt_amd import api
    names = ("batchAdd", "batchSub", "batchMul", "batchMulScalar", "batchSquare", "innerProduct", "hornerEval", "batchInverse", "multiScalarMulLinear")
    for n in names:
        assert callable(getattr(api.BatchOps, n)), n
    hpp = open(os.path.join(ROOT, "zolt_amd", "host", "field_vectors.hpp")).read()
    zig = open(os.path.join(ROOT, "zig", "gpu", "backend.zig")).read()
    body = zig[zig.index("pub const BatchOps = struct"):]
    for n in names:
        assert re.search(r"\b%s\(" % n, hpp), n
        assert "pub fn %s(" % n in body, n
    assert '#include "field_vectors.hpp"' in open(os.path.join(ROOT, "zolt_amd", "host", "zolt_host.hpp")).read()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-device path cannot be observed")
def test_without_a_device_every_entry_point_says_so():
    from zolt_amd import lib
    a = np.zeros((2, 4), dtype=np.uint64)
    calls = [lambda: lib.field_batch_inverse(lib.FR, a), lambda: lib.field_inner_product(lib.FP, a, a), lambda: lib.field_horner(lib.FR, a, a[0]),
             lambda: lib.field_op_dev(lib.FR, lib.OP_ADD, 64, 64, 64, 1), lambda: lib.field_scale_dev(lib.FR, 64, 1, a[0], 64),
             lambda: lib.field_batch_inverse_dev(lib.FP, 64, 64, 1), lambda: lib.field_inner_product_dev(lib.FR, 64, 64, 1),
             lambda: lib.field_horner_dev(lib.FR, 64, 1, a[0]), lambda: lib.fr_dense_evaluate_dev(64, a)]
    for call in calls:
        with pytest.raises(lib.ZgError) as e:
            call()
        assert e.value.code == lib.ERR_NO_DEVICE
