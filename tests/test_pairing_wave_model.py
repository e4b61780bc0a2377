"""The wave pairing engine without a GPU: its decomposition restated in Python (tests/pairing_wave_model.py) against the big-integer
model of tests/pairing_model.py; the kernels' own lane map compiled for the host (tests/cpp/pairing_wave_host.cpp), exhaustively; and the
surface of the section "Pairings (engine)". The design has no cyclotomic square and no separate squaring or sparse map: the square is the
product of a value with itself and the sparse product is the product with the zero-padded line, so one index algebra is checked."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import g2_model as G2
from tests import pairing_model as M
from tests import pairing_wave_model as W
from tests.test_gpu_pairing import _tower_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = M.P, M.R


# ---------------------------------------------------------------- the decomposition against the model
@pytest.fixture(scope="module")
def tower():
    return _tower_inputs()  # zero, one, all coefficients p - 1, single-coefficient elements, 200 random elements


def test_the_36_product_form_equals_mul(tower):
    a, b = tower
    assert [W.collect(W.mul(W.spread(u), W.spread(v))) for u, v in zip(a, b)] == [M.mul(u, v) for u, v in zip(a, b)]


def test_the_square_is_the_product_with_itself_and_equals_sqr(tower):
    a, _ = tower
    assert [W.collect(W.sqr(W.spread(u))) for u in a] == [M.sqr(u) for u in a]


def test_the_sparse_form_equals_mul_by_034(tower):
    a, b = tower
    rng = random.Random(34)
    r2 = lambda: (rng.randrange(P), rng.randrange(P))  # noqa: E731
    sparse = [(r2(), r2(), r2()) for _ in a]
    sparse[3], sparse[4], sparse[5], sparse[6] = ((0, 0), r2(), r2()), (r2(), (0, 0), r2()), (r2(), r2(), (0, 0)), ((0, 0), (0, 0), (0, 0))
    assert [W.collect(W.mul_by_034(W.spread(u), *s)) for u, s in zip(a, sparse)] == [M.mul_by_034(u, *s) for u, s in zip(a, sparse)]


def test_a_product_with_a_level_beside_it_leaves_both_right(tower):
    """mul_side: the 36 busy lanes' product is the Fp12 product and lane 36 + s holds u * v, whatever the other lanes multiply"""
    a, b = tower
    rng = random.Random(5)
    for u, v in list(zip(a, b))[-8:]:
        us = [(rng.randrange(P), rng.randrange(P)) for _ in range(W.LANES)]
        vs = [(rng.randrange(P), rng.randrange(P)) for _ in range(W.LANES)]
        f, t = W.mul_side(W.spread(u), W.spread(v), us, vs)
        assert W.collect(f) == M.mul(u, v)
        assert all(t[L] == G2.f2_mul(us[L], vs[L]) for L in range(W.SIDE0, W.LANES))


def test_halving_is_the_product_by_one_half():
    rng = random.Random(2)
    for c in [0, 1, 2, P - 1, P - 2] + [rng.randrange(P) for _ in range(50)]:
        assert W.half((c, P - 1 - c)) == (c * M.TWO_INV % P, (P - 1 - c) * M.TWO_INV % P)


def test_the_levelled_miller_loop_is_the_models():
    """the steps' levels (5, 3, 4 products for a doubling, 2, 6, 3, 4 for an addition), the shared instructions of f^2 and f * line, the
    closing steps as two more turns of the loop: the UNREDUCED value of millerLoopArkworks"""
    rng = random.Random(0xD0C1)
    for _ in range(2):
        p, q = M.g1_mul(M.G1_GEN, rng.randrange(1, R)), G2.scalar_mul(G2.G, rng.randrange(1, R))
        assert W.miller_loop(p, q) == M.miller_loop(p, q)


# ---------------------------------------------------------------- the kernels' lane map on the host
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no C++ compiler: the host harness compiles the kernels' own header")
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_lane_map_exhaustively(tmp_path, flags):
    exe = str(tmp_path / "pairing_wave_host")
    subprocess.run([CXX, "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "zolt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pairing_wave_host.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    rec = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if ln]
    lanes = {int(r[1]): tuple(int(x) for x in r[2:]) for r in rec if r[0] == "L"}
    assert sorted(lanes) == list(range(64))
    row = {L: v[0] for L, v in lanes.items()}
    col = {L: v[1] for L, v in lanes.items()}
    busy = [L for L, v in lanes.items() if v[2]]
    # each (i, j) is taken exactly once, by a busy lane; lane i holds column i, so that a_i can be fetched from it
    assert sorted((row[L], col[L]) for L in busy) == [(i, j) for i in range(6) for j in range(6)] and len(busy) == 36
    assert all(col[i] == i for i in range(6)) and all(0 <= row[L] < 6 and col[L] == L % 6 for L in lanes)
    # the xi mark is set exactly when i + j >= 6
    assert all(bool(lanes[L][3]) == (row[L] + col[L] >= 6) for L in lanes)
    # output k receives exactly the pairs with i + j = k (mod 6), each once, from busy lanes only: idle lanes contribute nothing
    srcs = {}
    for r in rec:
        if r[0] == "S":
            srcs.setdefault(int(r[1]), []).append(int(r[3]))
    assert sorted(srcs) == list(range(6))
    for k, ls in srcs.items():
        assert all(L in busy for L in ls)
        assert sorted((row[L], col[L]) for L in ls) == sorted((i, (k - i) % 6) for i in range(6))
    assert sorted(L for ls in srcs.values() for L in ls) == sorted(busy)
    # the sparse operand: c0, c3, c4 at the columns of w^0, w^1, w^3, zero elsewhere — so 18 busy lanes multiply by a coefficient
    assert all(lanes[L][5] == {0: 0, 1: 1, 3: 2}.get(col[L], -1) for L in lanes)
    assert sum(1 for L in busy if lanes[L][5] >= 0) == 18
    # memory order: c_{k & 1}.c_{k >> 1} of fp12_load is the model's TOWER_ORDER, a permutation
    assert all(M.TOWER_ORDER[lanes[L][4]] == col[L] for L in lanes)
    # the Miller steps: every level's products sit in distinct lanes past the busy 36, and the counts are the formulas'
    side = {int(r[1]): int(r[2]) for r in rec if r[0] == "P"}
    assert len(set(side.values())) == len(side) == 28 and all(36 <= L < 64 for L in side.values()) and all(side[s] == 36 + s for s in side)
    dbl = [int(r[2]) for r in rec if r[0] == "D"]
    add = [int(r[2]) for r in rec if r[0] == "A"]
    assert tuple(dbl) == W.DBL_PRODUCTS and tuple(add) == W.ADD_PRODUCTS and max(dbl + add) <= len(side)
    # 12 products and 2 halvings for double_in_place with its line's two scalings (10 + 2 of the reference, whose scalings by 1/2 are
    # the halvings); 15 for add_in_place with its two (13 + 2)
    assert sum(dbl) == 12 and sum(add) == 15
    # and the Python restatement uses the same map
    assert all((W.row(L), W.col(L), int(W.busy(L)), int(W.xi(L)), W.mem_slot(W.col(L)), W.sparse_slot(W.col(L))) == lanes[L] for L in lanes)
    assert all(W.src(k, t) == srcs[k][t] for k in range(6) for t in range(6))


# ---------------------------------------------------------------- the surface
def test_header_section_and_feature_bit():
    hdr = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "Pairings (engine)" in hdr and "#define ZG_FEATURE_PAIRING_WAVE 256u" in hdr
    assert "#define ZG_PAIRING_ENGINE_LANE 0" in hdr and "#define ZG_PAIRING_ENGINE_WAVE 1" in hdr


def test_abi_has_the_constants_and_both_signatures():
    import ctypes as C
    from zolt_amd import _abi, lib
    assert (_abi.ZG_PAIRING_ENGINE_LANE, _abi.ZG_PAIRING_ENGINE_WAVE, _abi.ZG_FEATURE_PAIRING_WAVE) == (0, 1, 256)
    assert _abi.PROTOS["zg_pairing_engine_set"] == (C.c_int, [C.c_int]) and _abi.PROTOS["zg_pairing_engine_get"] == (C.c_int, [])
    assert "zg_pairing_engine_set" in lib.SYMBOLS and "zg_pairing_engine_get" in lib.SYMBOLS
    assert (_abi.ZG_OP_FP12W_MUL, _abi.ZG_OP_FP12W_MUL_034) == (40, 48) == (lib.OP_FP12W_MUL, lib.OP_FP12W_MUL_034)
    assert lib.abi_version() == (1, 11) and lib.abi_features() & _abi.ZG_FEATURE_PAIRING_WAVE
    assert (lib.PAIRING_ENGINE_LANE, lib.PAIRING_ENGINE_WAVE) == (0, 1)


def test_the_setter_needs_no_device():
    from zolt_amd import api, lib
    start = lib.pairing_engine_get()
    try:
        lib.pairing_engine_set(1)
        assert lib.pairing_engine_get() == 1
        with pytest.raises(lib.ZgError) as ei:
            lib.pairing_engine_set(7)
        assert ei.value.code == lib.ERR_INVALID and lib.pairing_engine_get() == 1
        with lib.pairing_engine(0):
            assert lib.pairing_engine_get() == 0
        assert lib.pairing_engine_get() == 1
        with pytest.raises(KeyError):
            with api.Dory.pairing_engine(0):
                raise KeyError("inside")
        assert lib.pairing_engine_get() == 1
    finally:
        lib.pairing_engine_set(start)
    assert lib.pairing_engine_get() == start


def test_a_compute_entry_point_under_wave_without_a_gpu_reports_no_device():
    from zolt_amd import lib
    if os.path.exists("/dev/kfd"):
        return  # a GPU is present: the no-device answer cannot be observed (tests/test_gpu_pairing_wave.py runs the engine instead)
    with lib.pairing_engine(lib.PAIRING_ENGINE_WAVE):
        for call in (lambda: lib.final_exponentiation_batch(M.gt_pack([M.ONE])),
                     lambda: lib.field_op(lib.FP, lib.OP_FP12W_SQR, M.gt_pack([M.ONE]).reshape(-1, 4))):
            with pytest.raises(lib.ZgError) as ei:
                call()
            assert ei.value.code == lib.ERR_NO_DEVICE
