"""The Dory verifier setup on the device (zg_dory_verifier_setup[_points]: lib.dory_verifier_setup*, api.DoryVerifierSetup,
zolt::DoryVerifierSetup) against the reference's formula built the reference's way — one pairing WITH its final exponentiation per pair
(zg_pairing_batch on the explicit pair list), multiplied on the host with the model's Fp12 product, chi accumulated level by level
(src/zkvm/preprocessing.zig:833-973) — and against tests/dory_vsetup_model.py alone. Generators are small multiples of the group
generators. Everything is compared on all 48 words, or byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dory_commit_model as DM
from tests import dory_vsetup_model as VM
from tests import g2_model as G2
from tests import pairing_model as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT_ONE = PM.gt_pack([PM.ONE])[0]


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


def _gens(zl, a, b):
    """g1[i] = a[i] G, g2[i] = b[i] H as the ABI's arrays; a scalar of 0 is an identity, written as the reference writes it"""
    from zolt_amd import api
    g1 = zl.g1_fixed_base_mul_batch(api.generator(), DM.fr_pack([x or 1 for x in a]))
    g2 = zl.g2_fixed_base_mul_batch(api.g2_generator(), DM.fr_pack([x or 1 for x in b]))
    g1 = (np.ascontiguousarray(g1[0]).reshape(-1, 8).copy(), np.asarray(g1[1], dtype=np.uint8).copy())
    g2 = (np.ascontiguousarray(g2[0]).reshape(-1, 16).copy(), np.asarray(g2[1], dtype=np.uint8).copy())
    for i, x in enumerate(a):
        if not x:
            g1[0][i], g1[1][i] = 0, 1
    for i, x in enumerate(b):
        if not x:
            g2[0][i], g2[1][i] = G2.IDENTITY_WORDS, 1
    return g1, g2


def _reference_way(zl, g1, g2):
    """fromSRS as the reference runs it: every pair through zg_pairing_batch (a final exponentiation per pair), the products on the host"""
    K = g1[0].shape[0].bit_length() - 1
    pairs = [(0, 0)]
    for k in range(1, K + 1):
        h = 1 << (k - 1)
        pairs += [(h + j, j) for j in range(h)] + [(j, h + j) for j in range(h)] + [(h + j, h + j) for j in range(h)]
    i1, i2 = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    e = PM.gt_unpack(zl.pairing_batch(g1[0][i1], g1[1][i1], g2[0][i2], g2[1][i2]))

    def multi_pair(first, count):  # multiPair (:833-850): result = result.mul(paired), pair by pair
        result = PM.ONE
        for v in e[first:first + count]:
            result = PM.mul(result, v)
        return result

    chi, d1r, d2r = [e[0]], [PM.ONE], [PM.ONE]
    pos = 1
    for k in range(1, K + 1):
        h = 1 << (k - 1)
        d1r.append(multi_pair(pos, h))
        d2r.append(multi_pair(pos + h, h))
        chi.append(PM.mul(chi[k - 1], multi_pair(pos + 2 * h, h)))
        pos += 3 * h
    return PM.gt_pack(chi), PM.gt_pack(d1r), PM.gt_pack(d2r)


def _same(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


# ---------------------------------------------------------------- 1. against the literal reference formula
@pytest.mark.parametrize("n", [1, 2, 4, 8, 32])
def test_against_the_reference_formula(zl, n):
    """n = 32: 94 Miller lanes — two workgroups, sixteen segments"""
    g1, g2 = _gens(zl, [3 + 2 * i for i in range(n)], [5 + 3 * i for i in range(n)])
    got = zl.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1])
    assert got[0].shape == (n.bit_length(), 48)
    assert _same(got, _reference_way(zl, g1, g2))
    assert np.array_equal(got[1][0], GT_ONE) and np.array_equal(got[2][0], GT_ONE)
    assert _same(zl.dory_verifier_setup_points(g1[0], None, g2[0], None), got)  # absent flags = no identities


# ---------------------------------------------------------------- 2. against the model alone
def test_k1_against_the_model_alone(zl):
    a, b = [3, 5], [7, 2]
    g1, g2 = _gens(zl, a, b)
    vs = VM.from_srs([PM.g1_mul(PM.G1_GEN, x) for x in a], [G2.scalar_mul(G2.G, x) for x in b])
    got = zl.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1])
    assert _same(got, (PM.gt_pack(vs.chi), PM.gt_pack(vs.delta_1r), PM.gt_pack(vs.delta_2r)))


# ---------------------------------------------------------------- 3. shapes
def test_shapes_and_refusals(zl):
    g1, g2 = _gens(zl, [2, 3, 4, 5, 6, 7], [9, 8, 7, 6, 5, 4, 3, 2])
    want = _reference_way(zl, (g1[0][:4], g1[1][:4]), (g2[0][:4], g2[1][:4]))
    # n_g1 = 6, n_g2 = 4: K = 2, the generators beyond the first four are not read
    assert _same(zl.dory_verifier_setup_points(g1[0], g1[1], g2[0][:4], g2[1][:4]), want)
    # n_g2 = 2 * n_g1
    assert _same(zl.dory_verifier_setup_points(g1[0][:4], g1[1][:4], g2[0], g2[1]), want)
    # refusals leave the output as it was
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(3 * 3 * 48, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    levels = C.c_size_t(77)
    x1, x2 = np.ascontiguousarray(g1[0]), np.ascontiguousarray(g2[0])
    fn = zl._lib.zg_dory_verifier_setup_points
    assert fn(p(x1), None, 4, p(x2), None, 3, p(out), 3, C.byref(levels)) == zl.ERR_INVALID  # n_g2 = 2^K - 1
    assert fn(p(x1), None, 6, p(x2), None, 3, p(out), 3, C.byref(levels)) == zl.ERR_INVALID
    assert fn(p(x1), None, 4, p(x2), None, 4, p(out), 2, C.byref(levels)) == zl.ERR_INVALID  # levels_cap = K
    assert fn(None, None, 4, p(x2), None, 4, p(out), 3, C.byref(levels)) == zl.ERR_INVALID
    assert fn(p(x1), None, 0, p(x2), None, 4, p(out), 3, C.byref(levels)) == zl.ERR_INVALID
    assert zl._lib.zg_dory_verifier_setup(None, p(out), 3, C.byref(levels)) == zl.ERR_INVALID  # NULL key
    key = zl.DoryKey.create((g1[0][:4], g1[1][:4]), (g2[0][:3], g2[1][:3]))  # a key whose g2_vec is too short
    assert zl._lib.zg_dory_verifier_setup(key._h, p(out), 3, C.byref(levels)) == zl.ERR_INVALID
    key.free()
    key = zl.DoryKey.create((g1[0][:4], g1[1][:4]), (g2[0][:4], g2[1][:4]))
    assert zl._lib.zg_dory_verifier_setup(key._h, p(out), 2, C.byref(levels)) == zl.ERR_INVALID
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and levels.value == 77
    assert zl._lib.zg_dory_verifier_setup(key._h, p(out), 5, C.byref(levels)) == zl.OK and levels.value == 3  # a larger capacity is fine
    key.free()
    assert _same([out[:144].reshape(3, 48), out[144:288].reshape(3, 48), out[288:].reshape(3, 48)], want)


# ---------------------------------------------------------------- 4. identities
@pytest.mark.parametrize("case", ["g1_inner", "g2", "g1_first", "both_sides", "repeated"])
def test_identities_and_repeated_generators(zl, case):
    a, b = [3 + 2 * i for i in range(8)], [5 + 3 * i for i in range(8)]
    if case == "g1_inner":
        a[5] = 0
    elif case == "g2":
        b[2] = 0
    elif case == "g1_first":
        a[0] = 0
    elif case == "both_sides":
        a[3], b[3], b[6] = 0, 0, 0
    else:
        a = [4] * 8  # g1[i] = g1[0] for all i
    g1, g2 = _gens(zl, a, b)
    got = zl.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1])
    assert _same(got, _reference_way(zl, g1, g2))
    if case == "g1_first":
        assert np.array_equal(got[0][0], GT_ONE)  # chi[0] = one
    key = zl.DoryKey.create(g1, g2)
    assert _same(zl.dory_verifier_setup(key), got)
    key.free()


# ---------------------------------------------------------------- 5. key form and points form
def test_key_form_points_form_and_an_undisturbed_key(zl):
    from zolt_amd import api
    n = 16
    g1, g2 = _gens(zl, [3 + 2 * i for i in range(n)], [5 + 3 * i for i in range(n)])
    key = zl.DoryKey.create(g1, g2)
    polys = [("u64", np.arange(1, 65, dtype=np.uint64)), ("fr", DM.fr_pack([1000 + 17 * i for i in range(64)])), ("chunk", np.arange(64, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15), 60, 4)]
    before = api.Dory.batchCommit(key, polys, want_rows=True)
    a = zl.dory_verifier_setup(key)
    b = zl.dory_verifier_setup(key)
    after = api.Dory.batchCommit(key, polys, want_rows=True)
    key.free()
    assert _same(a, b) and _same(a, zl.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1]))
    assert np.array_equal(before[0], after[0])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(before[1], after[1]))


# ---------------------------------------------------------------- 6. mirrors
@pytest.fixture(scope="module")
def setup4(zl):
    from zolt_amd import api
    params = api.Dory.setup(4)  # the reference's own test shape (preprocessing.zig:1187-1216): four generators a side, three levels
    yield params, api.DoryVerifierSetup.fromSRS(params)
    params.deinit()


def test_python_mirror_serialises_the_models_bytes(zl, setup4):
    from zolt_amd import api
    params, vs = setup4
    g1m, g2m = DM.setup(4)
    assert len(g1m) == 4 and len(g2m) == 4
    want = VM.serialize(VM.from_srs(g1m, g2m))
    got = vs.serialize()
    assert len(got) == VM.serialized_len(2) and got == want
    assert vs.chi.shape == (3, 48) and vs.max_log_n == 4
    assert np.array_equal(vs.delta_1l, np.concatenate([GT_ONE.reshape(1, 48), vs.chi[:-1]])) and np.array_equal(vs.delta_2l, vs.delta_1l)
    assert np.array_equal(vs.ht, vs.chi[0]) and np.array_equal(vs.delta_1r[0], GT_ONE) and np.array_equal(vs.delta_2r[0], GT_ONE)
    assert np.array_equal(vs.h1[0], vs.g1_0[0]) and np.array_equal(vs.g1_0[0], np.asarray(params.g1_vec[0]).reshape(-1, 8)[0])
    key = api.Dory.key(params)
    assert api.DoryVerifierSetup.fromSRS(key).serialize() == want  # over a resident key
    key.free()


def test_cpp_mirror_produces_the_same_bytes(zl, setup4, tmp_path):
    """tests/cpp/test_dory_vsetup_mirror.cpp prints zolt::DoryVerifierSetup's serialised bytes for setup(4), from points and over a key"""
    exe = str(tmp_path / "test_dory_vsetup_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dory_vsetup_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    got = {l.split()[0]: l.split()[1] for l in res.stdout.splitlines()}
    want = setup4[1].serialize().hex()
    assert got["points"] == want and got["key"] == want
    assert got["id1"] == VM.serialize_g1(None).hex() and got["id2"] == VM.serialize_g2(None).hex()


# ---------------------------------------------------------------- 7. feature bit
def test_feature_bit(zl):
    from zolt_amd import _abi
    assert zl.abi_features() & 128 and _abi.ZG_FEATURE_DORY_VSETUP == 128 and zl.abi_version() == (1, 11)
    assert [zl.dory_verifier_setup_levels(n) for n in (0, 1, 6, 1024)] == [0, 1, 3, 11]
