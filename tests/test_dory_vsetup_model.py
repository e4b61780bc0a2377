"""The model of the Dory verifier setup (tests/dory_vsetup_model.py: fromSRS, multiPair, serialize of src/zkvm/preprocessing.zig:833-1166)
against bilinearity; the homomorphism the device form relies on; the serialised lengths and point encodings; the header section and its
bindings; the lane decode and the segment table of the kernels, compiled for the host from their own header; and the entry points'
answers without a device.

    python -m pytest tests/test_dory_vsetup_model.py -q --durations=0"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dory_vsetup_model as VM
from tests import g2_model as G2
from tests import pairing_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = G2.R
A, B = [3, 5], [7, 2]  # g1[i] = A[i] G, g2[i] = B[i] H


@pytest.fixture(scope="module")
def e_gen():
    return PM.pairing(PM.G1_GEN, G2.G)


@pytest.fixture(scope="module")
def srs2():
    return [PM.g1_mul(PM.G1_GEN, a) for a in A], [G2.scalar_mul(G2.G, b) for b in B]


@pytest.fixture(scope="module")
def setup2(srs2):
    return VM.from_srs(*srs2)


# ---------------------------------------------------------------- the model against bilinearity
def test_k0_is_one_pairing_and_three_ones(e_gen, srs2):
    vs = VM.from_srs(srs2[0][:1], srs2[1][:1])
    assert vs.chi == [PM.power(e_gen, A[0] * B[0])] and vs.ht == vs.chi[0]
    assert vs.delta_1l == vs.delta_1r == vs.delta_2l == vs.delta_2r == [PM.ONE]
    assert vs.max_log_n == 0 and vs.g1_0 == vs.h1 == srs2[0][0] and vs.g2_0 == vs.h2 == srs2[1][0]


def test_k1_four_pairings_against_bilinearity(e_gen, setup2):
    vs = setup2
    assert vs.chi == [PM.power(e_gen, A[0] * B[0]), PM.power(e_gen, A[0] * B[0] + A[1] * B[1])]
    assert vs.delta_1r == [PM.ONE, PM.power(e_gen, A[1] * B[0])]  # g1[h..2h) against g2[0..h)
    assert vs.delta_2r == [PM.ONE, PM.power(e_gen, A[0] * B[1])]  # g1[0..h) against g2[h..2h)
    assert vs.delta_1l == vs.delta_2l == [PM.ONE, vs.chi[0]]
    assert vs.ht == vs.chi[0] and vs.max_log_n == 2
    # the chi values by repeated multiplication too: e^15 * e^21 = e^36
    acc = PM.ONE
    for _ in range(A[1] * B[1]):
        acc = PM.mul(acc, e_gen)
    assert PM.mul(vs.chi[0], acc) == vs.chi[1]


def test_an_identity_pair_contributes_one(e_gen, srs2):
    g1, g2 = srs2
    vs = VM.from_srs([None, g1[1]], g2)
    assert vs.chi == [PM.ONE, PM.power(e_gen, A[1] * B[1])] and vs.delta_2r[1] == PM.ONE and vs.ht == PM.ONE
    vs = VM.from_srs(g1, [g2[0], None])
    assert vs.chi[1] == vs.chi[0] and vs.delta_2r[1] == PM.ONE and vs.delta_1r[1] == PM.power(e_gen, A[1] * B[0])


def test_short_g2_is_out_of_bounds_and_extra_generators_are_unused(srs2, setup2):
    g1, g2 = srs2
    with pytest.raises(IndexError):
        VM.from_srs(g1, g2[:1])
    vs = VM.from_srs(g1 + [PM.G1_GEN], g2 + [G2.G, G2.G])  # n_g1 = 3: K = 1 still
    assert VM.serialize(vs) == VM.serialize(setup2)


def test_product_of_pairings_is_one_final_exponentiation_of_the_miller_product(srs2):
    """what the device does instead of multiPair's loop: the same inputs, the same value"""
    g1, g2 = srs2
    per_pair = VM.multi_pair(g1, g2)
    miller = PM.mul(PM.miller_loop(g1[0], g2[0]), PM.miller_loop(g1[1], g2[1]))
    assert PM.final_exponentiation(miller) == per_pair == PM.multi_pairing(g1, g2)
    # and chi's running product: exponentiating P_0 and P_0 P_1 gives chi[0] and chi[0] * e(level 1)
    m0 = PM.miller_loop(g1[0], g2[0])
    assert PM.mul(PM.final_exponentiation(m0), PM.pairing(g1[1], g2[1])) == PM.final_exponentiation(PM.mul(m0, PM.miller_loop(g1[1], g2[1])))


# ---------------------------------------------------------------- serialize
def test_serialised_lengths_and_field_order(srs2, setup2):
    g1, g2 = srs2
    for K, vs in ((0, VM.from_srs(g1[:1], g2[:1])), (1, setup2)):
        b = VM.serialize(vs)
        assert len(b) == VM.serialized_len(K) == 5 * (8 + (K + 1) * 384) + 32 + 64 + 32 + 64 + 384 + 8
        pos = 0
        for vec in (vs.delta_1l, vs.delta_1r, vs.delta_2l, vs.delta_2r, vs.chi):
            assert int.from_bytes(b[pos:pos + 8], "little") == K + 1
            assert [PM.from_bytes(b[pos + 8 + 384 * i:pos + 8 + 384 * (i + 1)]) for i in range(K + 1)] == vec
            pos += 8 + 384 * (K + 1)
        assert b[pos:pos + 32] == b[pos + 96:pos + 128] == VM.serialize_g1(g1[0])          # g1_0, h1
        assert b[pos + 32:pos + 96] == b[pos + 128:pos + 192] == VM.serialize_g2(g2[0])    # g2_0, h2
        assert PM.from_bytes(b[pos + 192:pos + 576]) == vs.ht == vs.chi[0]
        assert int.from_bytes(b[pos + 576:], "little") == 2 * K
    one = VM.serialize_gt(PM.ONE)
    assert one == (1).to_bytes(32, "little") + bytes(352)  # standard form, c0.c0.c0 first


def test_point_encodings_identity_and_sign(srs2):
    assert VM.serialize_g1(None) == bytes(24) + (1 << 62).to_bytes(8, "little")
    assert VM.serialize_g2(None) == bytes(56) + (1 << 62).to_bytes(8, "little")
    for p in srs2[0] + [PM.G1_GEN]:
        a, b = VM.serialize_g1(p), VM.serialize_g1(PM.g1_neg(p))
        assert a[:31] == b[:31] and a[31] ^ b[31] == 0x80 and (a[31] & 0x40) == 0  # one of the two carries bit 63, never bit 62
        assert int.from_bytes(a, "little") & ((1 << 254) - 1) == p[0]
        assert bool(a[31] & 0x80) == (not p[1] < G2.P - p[1])
    for q in srs2[1] + [G2.G]:
        a, b = VM.serialize_g2(q), VM.serialize_g2(G2.neg(q))
        assert a[:63] == b[:63] and a[63] ^ b[63] == 0x80 and (a[63] & 0x40) == 0
        assert int.from_bytes(a[:32], "little") == q[0][0] and int.from_bytes(a[32:], "little") & ((1 << 254) - 1) == q[0][1]
    # c1 decides before c0 (:1141-1166): a y with a small c1 and a large c0 is "positive"
    assert VM.lexicographically_less_fp2((G2.P - 1, 1), (1, G2.P - 1)) and not VM.lexicographically_less_fp2((5, 7), (5, 7))
    # y = -y only for y = 0 (no point of the curve): not less, so the flag is set — unlike dory.zig's compressG1, where equal is positive
    assert VM.serialize_g1((1, 0))[31] & 0x80


def test_the_api_mirror_serialises_the_models_bytes(srs2, setup2):
    """api.DoryVerifierSetup over the model's values (no device): the copies it makes and its own serializer"""
    from zolt_amd import api
    g1, g2 = srs2
    g1w, g2w = PM.g1_pack(g1), G2.pack(g2)
    vs = api.DoryVerifierSetup(PM.gt_pack(setup2.chi), PM.gt_pack(setup2.delta_1r), PM.gt_pack(setup2.delta_2r), (g1w[0][0], 0), (g2w[0][0], 0))
    assert vs.serialize() == VM.serialize(setup2)
    assert np.array_equal(vs.delta_1l, PM.gt_pack(setup2.delta_1l)) and np.array_equal(vs.delta_2l, vs.delta_1l)
    assert np.array_equal(vs.ht, vs.chi[0]) and vs.max_log_n == 2
    for p in g1 + [None]:
        w = PM.g1_pack([p])
        assert api.serializeG1(w[0][0], int(w[1][0])) == VM.serialize_g1(p)
        if p is not None:
            w = PM.g1_pack([PM.g1_neg(p)])
            assert api.serializeG1(w[0][0], 0) == VM.serialize_g1(PM.g1_neg(p))
    for q in g2 + [None, G2.neg(g2[0])]:
        w = G2.pack([q])
        assert api.serializeG2(w[0][0], int(w[1][0])) == VM.serialize_g2(q)


# ---------------------------------------------------------------- header, bindings, no device
def test_header_section_and_bindings():
    from zolt_amd import _abi, lib
    text = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "------ Dory verifier setup */" in text and "#define ZG_FEATURE_DORY_VSETUP 128u" in text
    assert text.index("Dory commitments (key and batch) */") < text.index("Dory verifier setup */") < text.index("------ poly tables */")
    assert "#define ZG_ABI_MINOR 11\n" in text
    names = ["zg_dory_verifier_setup_levels", "zg_dory_verifier_setup", "zg_dory_verifier_setup_points"]
    assert all(n in lib.SYMBOLS and hasattr(lib._lib, n) for n in names)
    assert _abi.PROTOS["zg_dory_verifier_setup_levels"] == (C.c_size_t, [C.c_size_t])
    assert _abi.PROTOS["zg_dory_verifier_setup"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    assert _abi.PROTOS["zg_dory_verifier_setup_points"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                      C.c_size_t, C.c_void_p])
    assert _abi.ZG_FEATURE_DORY_VSETUP == 128 and lib.abi_features() & 128 and lib.abi_version() == (1, 11) and _abi.ZG_ABI_MINOR == 11
    assert [lib.dory_verifier_setup_levels(n) for n in (0, 1, 2, 3, 4, 6, 1023, 1024, 65536)] == [0, 1, 2, 2, 3, 3, 10, 11, 17]


def test_bad_arguments_are_invalid_and_nothing_computes_without_a_device():
    from zolt_amd import lib
    g1, g2 = np.zeros((4, 8), dtype=np.uint64), np.zeros((4, 16), dtype=np.uint64)
    out = np.full(3 * 3 * 48, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    levels = C.c_size_t(99)
    fn = lib._lib.zg_dory_verifier_setup_points
    assert lib._lib.zg_dory_verifier_setup(None, p(out), 3, C.byref(levels)) == lib.ERR_INVALID
    assert fn(None, None, 4, p(g2), None, 4, p(out), 3, C.byref(levels)) == lib.ERR_INVALID       # NULL points
    assert fn(p(g1), None, 4, None, None, 4, p(out), 3, C.byref(levels)) == lib.ERR_INVALID
    assert fn(p(g1), None, 0, p(g2), None, 4, p(out), 3, C.byref(levels)) == lib.ERR_INVALID      # n_g1 = 0
    assert fn(p(g1), None, (1 << 16) + 1, p(g2), None, 1 << 17, p(out), 17, C.byref(levels)) == lib.ERR_INVALID
    assert fn(p(g1), None, 4, p(g2), None, 3, p(out), 3, C.byref(levels)) == lib.ERR_INVALID      # n_g2 < 2^K
    assert fn(p(g1), None, 4, p(g2), None, 4, p(out), 2, C.byref(levels)) == lib.ERR_INVALID      # levels_cap < K + 1
    assert fn(p(g1), None, 4, p(g2), None, 4, None, 3, C.byref(levels)) == lib.ERR_INVALID
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and levels.value == 99
    if os.path.exists("/dev/kfd"):
        return  # a GPU is present: the no-device answer cannot be observed (tests/test_gpu_dory_vsetup.py runs the section instead)
    assert fn(p(g1), None, 4, p(g2), None, 4, p(out), 3, C.byref(levels)) == lib.ERR_NO_DEVICE
    assert fn(p(g1), None, 6, p(g2), None, 9, p(out), 5, None) == lib.ERR_NO_DEVICE
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and levels.value == 99


# ---------------------------------------------------------------- the kernels' lane decode on the host
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def _build(tmp, flags):
    path = str(tmp / "dory_vsetup_host")
    subprocess.run([CXX, "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "zolt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "dory_vsetup_host.cpp"),
                    "-o", path], check=True, capture_output=True, text=True)
    return path


def _decode(exe, K):
    lines = subprocess.run([exe, str(K)], check=True, capture_output=True, text=True).stdout.split("\n")
    head = lines[0].split()
    assert head[0] == "L"
    lanes, segs = int(head[1]), int(head[2])
    seg = [int(l.split()[2]) for l in lines[1:segs + 2]]
    pairs = [tuple(int(t) for t in l.split()[1:]) for l in lines[segs + 2:segs + 2 + lanes]]
    assert all(l.startswith("S ") for l in lines[1:segs + 2]) and all(l.startswith("P ") for l in lines[segs + 2:segs + 2 + lanes])
    return lanes, segs, seg, pairs


@pytest.mark.skipif(CXX is None, reason="no C++ compiler: the host harness compiles the kernels' own header")
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_lane_decode_and_segment_table(tmp_path, flags):
    """for K = 0..6: every (family, level, offset) exactly once with fromSRS's indices, and segment s holds exactly its pairs"""
    exe = _build(tmp_path, flags)
    for K in range(7):
        N = 1 << K
        lanes, segs, seg, pairs = _decode(exe, K)
        assert lanes == 3 * N - 2 == len(pairs) and segs == 3 * K + 1 and len(seg) == segs + 1
        assert seg[0] == 0 and seg[-1] == lanes and all(a < b for a, b in zip(seg, seg[1:]))  # ascending, none empty, all lanes covered
        assert [p[0] for p in pairs] == list(range(lanes))
        want = {(0, 0, 0): (0, 0)}
        for k in range(1, K + 1):
            h = 1 << (k - 1)
            for j in range(h):
                want[(0, k, j)] = (h + j, h + j)   # chi[k]'s factor: g1[h..2h) against g2[h..2h)
                want[(1, k, j)] = (h + j, j)       # delta_1r[k]: g1[h..2h) against g2[0..h)
                want[(2, k, j)] = (j, h + j)       # delta_2r[k]: g1[0..h) against g2[h..2h)
        got = {}
        for lane, fam, k, j, i1, i2 in pairs:
            assert (fam, k, j) not in got and i1 < N and i2 < N
            got[(fam, k, j)] = (i1, i2)
        assert got == want
        for s in range(segs):  # segments 0..K diagonal levels, K + k upper level k, 2K + k lower level k
            fam, k = (0, s) if s <= K else (1, s - K) if s <= 2 * K else (2, s - 2 * K)
            inside = [(p[1], p[2], p[3]) for p in pairs[seg[s]:seg[s + 1]]]
            assert inside == [(fam, k, j) for j in range(max(1 << (k - 1), 1) if k else 1)], (K, s)
