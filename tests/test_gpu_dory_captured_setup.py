"""The device's pairings and its Dory verifier setup held to bytes the REFERENCE wrote (tests/golden/dory_verifier_setup_captured.bin,
parsed by tests/dory_captured.py; the models' side is tests/test_dory_captured_setup.py): chi[0] = e(g1_0, g2_0) through every pairing
entry point, the K = 0 verifier setup of that pair through lib, api and the C++ mirror down to the serialised bytes, multi-pairings of
device-made multiples of the pair against powers of chi[0], and the Fp12 hooks on the file's 41 GT values. Every case runs under the
LANE and under the WAVE engine, set only inside `with lib.pairing_engine(...)`. Words and bytes only: no tolerances.

The model's expectations are computed once per module and shared by both engines."""
import os
import random
import subprocess
import types

import numpy as np
import pytest

from tests import dory_captured as DC
from tests import g2_model as G2
from tests import pairing_model as M
from tests import test_gpu_pairing as TP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
ONE_WORDS = M.gt_pack([M.ONE])[0]
ENGINES = pytest.mark.parametrize("engine", ["lane", "wave"])
SEG = [0, 0, 1, 65, 130]
N_POOL = 130


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def cap():
    return DC.parse()


@pytest.fixture(scope="module")
def pair(cap):
    """the reference's g1_0 (1, 8) and g2_0 (1, 16) as the ABI's Montgomery words, with the signs their flags name"""
    return M.g1_pack([cap.g1_0])[0], G2.pack([cap.g2_0])[0]


def _engine(zl, name):
    return zl.pairing_engine(zl.PAIRING_ENGINE_WAVE if name == "wave" else zl.PAIRING_ENGINE_LANE)


# ---------------------------------------------------------------- 1. the single pairing
@ENGINES
def test_single_pairing_is_chi0(zl, cap, pair, engine):
    import torch
    g1, g2 = pair
    chi0 = cap.chi_words[:1]
    none = np.zeros(1, dtype=np.uint8)
    work = torch.cuda.Stream()
    with _engine(zl, engine):
        got = zl.pairing_batch(g1, None, g2, None)
        mil = zl.miller_loop_batch(g1, None, g2, None)
        fe = zl.final_exponentiation_batch(mil)
        multi = zl.multi_pairing(g1, None, g2, None)
        multi_dev = TP._multi_dev(zl, g1, none, g2, none, [0, 1], work.cuda_stream)
        flipped = zl.pairing_batch(np.concatenate([M.g1_pack([M.g1_neg(cap.g1_0)])[0], g1]), None, np.concatenate([g2, G2.pack([G2.neg(cap.g2_0)])[0]]), None)
    assert got.shape == (1, 48) and np.array_equal(got, chi0)
    assert np.array_equal(mil, M.gt_pack([M.miller_loop(cap.g1_0, cap.g2_0)]))  # the unreduced value is the model's
    assert np.array_equal(fe, chi0) and np.array_equal(multi, chi0) and np.array_equal(multi_dev, chi0)
    from zolt_amd import api
    assert api.gt_to_bytes(got[0]) == cap.chi_bytes[0] == cap.ht_bytes
    # either sign flipped alone: the conjugate, which is not chi[0]
    conj = M.gt_pack([M.conj(cap.chi[0])])[0]
    assert np.array_equal(flipped[0], conj) and np.array_equal(flipped[1], conj) and not np.array_equal(conj, chi0[0])


# ---------------------------------------------------------------- 2. the verifier setup at K = 0
def _k0_bytes(cap):
    """serialize (:977-1025) of fromSRS over the ONE pair (g1_0, g2_0), put together from the fixture's own bytes: four vectors of one
    `one`, chi = [chi[0]], then the fixture's g1_0, g2_0, h1, h2, ht as they stand (bytes 17 320 .. 17 896) and max_log_n = 0"""
    one = M.to_bytes(M.ONE)
    out = b"".join((1).to_bytes(8, "little") + g for g in (one, one, one, one, cap.chi_bytes[0]))
    return out + cap.raw[DC.POINTS_AT:17896] + (0).to_bytes(8, "little")


@ENGINES
def test_verifier_setup_at_k0(zl, cap, pair, engine):
    from zolt_amd import api
    g1, g2 = pair
    want = (cap.chi_words[:1], ONE_WORDS.reshape(1, 48), ONE_WORDS.reshape(1, 48))
    want_bytes = _k0_bytes(cap)
    with _engine(zl, engine):
        by_points = zl.dory_verifier_setup_points(g1, None, g2, None)
        key = zl.DoryKey.create((g1, None), (g2, None))
        by_key = zl.dory_verifier_setup(key)
        ser_points = api.DoryVerifierSetup.fromSRS(types.SimpleNamespace(g1_vec=(g1, None), g2_vec=(g2, None))).serialize()
        ser_key = api.DoryVerifierSetup.fromSRS(key).serialize()
        key.free()
    for got in (by_points, by_key):
        assert all(g.shape == (1, 48) and np.array_equal(g, w) for g, w in zip(got, want))
    for ser in (ser_points, ser_key):
        assert ser[-584:-8] == cap.raw[17320:17896]  # g1_0, g2_0, h1, h2, ht
        assert ser == want_bytes


def test_cpp_mirror_serialises_the_fixtures_bytes_at_k0(zl, cap, pair, tmp_path):
    """tests/cpp/test_dory_vsetup_mirror.cpp with a file argument: zolt::DoryVerifierSetup over the one pair, from points and over a key,
    under each engine"""
    exe = str(tmp_path / "test_dory_vsetup_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dory_vsetup_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    words = str(tmp_path / "pair.bin")
    np.concatenate([pair[0].reshape(-1), pair[1].reshape(-1)]).astype("<u8").tofile(words)
    res = subprocess.run([exe, words], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    got = {l.split()[0]: l.split()[1] for l in res.stdout.splitlines()}
    want = _k0_bytes(cap).hex()
    assert sorted(got) == ["lane_key", "lane_points", "wave_key", "wave_points"]
    for name, ser in got.items():
        assert ser[-2 * 584:-16] == cap.raw[17320:17896].hex(), name
        assert ser == want, name


# ---------------------------------------------------------------- 3. products anchored on chi[0]
class Products:
    """130 pairs (a_i g1_0, b_i g2_0), the multiples made on the device by the per-pair scalar multiplication batches; pair 0 is the
    reference's pair itself, pair 1 has a = r - 1 (-g1_0), pair 2 b = r - 1, pair 3 both; G1 is the identity at 5 and at 129, G2 at 70
    and at 129 (flags only: the coordinates under them are garbage). Expected values: ONE M.power of chi[0] per product."""

    def __init__(self, zl, cap, pair):
        rng = random.Random(0xD0C2)
        self.a = [rng.randrange(1, R) for _ in range(N_POOL)]
        self.b = [rng.randrange(1, R) for _ in range(N_POOL)]
        self.a[0], self.b[0] = 1, 1
        self.a[1], self.b[1] = R - 1, 1
        self.a[2], self.b[2] = 1, R - 1
        self.a[3], self.b[3] = R - 1, R - 1
        zeros = np.zeros(N_POOL, dtype=np.uint8)
        self.g1, i1 = zl.g1_scalar_mul_batch(np.tile(pair[0], (N_POOL, 1)), zeros, G2.fr_pack(self.a))
        self.g2, i2 = zl.g2_scalar_mul_batch(np.tile(pair[1], (N_POOL, 1)), zeros, G2.fr_pack(self.b))
        assert not i1.any() and not i2.any()
        # the multiples against the model's group laws, on the edges and one random pair
        p, q = M.g1_unpack(self.g1[[0, 1, 7]], zeros[:3]), G2.unpack(self.g2[[0, 2, 7]], zeros[:3])
        assert p == [cap.g1_0, M.g1_neg(cap.g1_0), M.g1_mul(cap.g1_0, self.a[7])]
        assert q == [cap.g2_0, G2.neg(cap.g2_0), G2.scalar_mul(cap.g2_0, self.b[7])]
        self.i1, self.i2 = zeros.copy(), zeros.copy()
        self.i1[[5, 129]] = 1
        self.i2[[70, 129]] = 1
        self.g1[5], self.g1[129], self.g2[70], self.g2[129] = 0xdeadbeef, 0, 0xfeedface, 0
        self.chi0 = cap.chi[0]
        self._want = {}

    def want(self, lo, hi):
        """chi[0]^(sum a_i b_i mod r) over the pairs lo .. hi - 1 that have no identity -> 48 words"""
        if (lo, hi) not in self._want:
            e = sum(self.a[i] * self.b[i] for i in range(lo, hi) if not self.i1[i] and not self.i2[i]) % R
            self._want[(lo, hi)] = M.gt_pack([M.power(self.chi0, e)])[0]
        return self._want[(lo, hi)]


@pytest.fixture(scope="module")
def products(zl, cap, pair):
    return Products(zl, cap, pair)


@ENGINES
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_product_of_n_pairs_is_a_power_of_chi0(zl, cap, products, engine, n):
    """the lane engine's block edges"""
    pr = products
    with _engine(zl, engine):
        got = zl.multi_pairing(pr.g1[:n], pr.i1[:n], pr.g2[:n], pr.i2[:n])
    assert got.shape == (1, 48) and np.array_equal(got[0], pr.want(0, n))
    if n == 1:
        assert np.array_equal(got, cap.chi_words[:1])


@ENGINES
def test_segmented_products_of_130_pairs(zl, cap, products, engine):
    """n = 130 in segments of 0, 1, 64 and 65 pairs (the product kernel's stride); the device-pointer entry point beside the host one;
    e(-P, Q) = e(P, -Q) = conj(chi[0]) and e(-P, -Q) = chi[0] on the r - 1 multiples"""
    import torch
    pr = products
    work = torch.cuda.Stream()
    with _engine(zl, engine):
        got = zl.multi_pairing(pr.g1, pr.i1, pr.g2, pr.i2, SEG)
        dev = TP._multi_dev(zl, pr.g1, pr.i1, pr.g2, pr.i2, SEG, work.cuda_stream)
        first = zl.pairing_batch(pr.g1[:4], pr.i1[:4], pr.g2[:4], pr.i2[:4])
        ident = zl.pairing_batch(pr.g1[[5, 70, 129]], pr.i1[[5, 70, 129]], pr.g2[[5, 70, 129]], pr.i2[[5, 70, 129]])
    assert got.shape == (4, 48) and np.array_equal(dev, got)
    assert np.array_equal(got[0], ONE_WORDS) and np.array_equal(got[1], cap.chi_words[0])
    for j in range(4):
        assert np.array_equal(got[j], pr.want(SEG[j], SEG[j + 1])), j
    conj = M.gt_pack([M.conj(cap.chi[0])])[0]
    assert np.array_equal(first, np.stack([cap.chi_words[0], conj, conj, cap.chi_words[0]]))
    assert np.array_equal(ident, np.tile(ONE_WORDS, (3, 1)))


# ---------------------------------------------------------------- 4. the tower hooks on the reference's GT values
@pytest.fixture(scope="module")
def tower(cap):
    """the 41 values (25 distinct), a second operand for the product (the next value, cyclically), and the model's answers — each
    computed once per distinct value"""
    vals, words = DC.gt_values(cap)
    assert len(vals) == 41
    memo = {}

    def once(tag, fn, g):
        key = (tag, g)
        if key not in memo:
            memo[key] = fn(g)
        return memo[key]

    other = vals[1:] + vals[:1]
    want = {"MUL": [M.mul(g, h) for g, h in zip(vals, other)], "SQR": [once("sqr", M.sqr, g) for g in vals],
            "FROB1": [M.frobenius(g, 1) for g in vals], "FROB2": [M.frobenius(g, 2) for g in vals], "FROB3": [M.frobenius(g, 3) for g in vals],
            "EXP_X": [once("exp", M.exp_by_x, g) for g in vals], "FINAL": [once("fe", M.final_exponentiation, g) for g in vals]}
    return words, np.concatenate([words[1:], words[:1]]), {k: M.gt_pack(v) for k, v in want.items()}


@ENGINES
def test_tower_hooks_on_the_41_gt_values(zl, tower, engine):
    words, other, want = tower
    op = lambda name: getattr(zl, ("OP_FP12W_" if engine == "wave" else "OP_FP12_") + name)  # noqa: E731
    x, y = words.reshape(-1, 4), other.reshape(-1, 4)
    with _engine(zl, engine):
        run = lambda name, b=None: zl.field_op(zl.FP, op(name), x, b).reshape(-1, 48)  # noqa: E731
        inv, conj = run("INV"), run("CONJ")
        got = {"MUL": run("MUL", y), "SQR": run("SQR"), "FROB1": run("FROB1"), "FROB2": run("FROB2"), "FROB3": run("FROB3"), "EXP_X": run("EXP_X"),
               "FINAL": zl.final_exponentiation_batch(words)}
        unit = run("MUL", conj.reshape(-1, 4))
    assert inv.shape == (41, 48) and np.array_equal(inv, conj)  # unitary values: the inverse IS the conjugate, word for word; no model
    assert not np.array_equal(conj, words)
    assert np.array_equal(unit, np.tile(ONE_WORDS, (41, 1)))  # g * conj(g) = one
    for name, w in want.items():
        assert np.array_equal(got[name], w), name
