"""DoryCommitmentScheme.open (src/poly/commitment/dory.zig:1052-1378) without a device: the two models of tests/dory_open_key_model.py
against the joint opening proof the reference wrote into its own proof file (tests/golden/dory_open_captured.bin, cut out by
tests/golden/make_dory_open_fixture.py), against each other where the captured run does not reach, and against the existing model of
openWithTranscript where the two functions coincide; the round-shape header of the device session against the reference's loop; the
header section and the bindings.

What the fixture pins and what it does not is written down in docs/design/02_oracle_pinning.md."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dory_open_key_model as K
from tests import dory_open_model as D
from tests import g2_model as G2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def captured():
    with open(os.path.join(GOLDEN, "dory_open_captured.bin"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def captured_inputs():
    with open(os.path.join(GOLDEN, "fibonacci.elf"), "rb") as f:
        return K.captured_inputs(f.read(), K.setup_scalars(9))


@pytest.fixture(scope="module")
def captured_exponents(captured_inputs):
    return K.exponents_of(captured_inputs)


# ---------------------------------------------------------------- 1. the captured run
def test_exponent_model_reproduces_the_captured_proof(captured, captured_inputs, captured_exponents):
    """open(setup(9), bytecode_evals, point) with nu = 4, sigma = 5 and five rounds: all 13 868 bytes"""
    assert (captured_inputs["nu"], captured_inputs["sigma"]) == (4, 5) and len(captured) == 908 + 2592 * 5 == 13868
    assert int.from_bytes(captured[800:804], "little") == 5 and captured[-8:] == (4).to_bytes(4, "little") + (5).to_bytes(4, "little")
    assert K.ark_bytes_of_exponents(captured_exponents, 4, 5) == captured


def test_point_model_reproduces_the_captured_proof(captured, captured_inputs):
    """the point-level model on the same inputs: about 200 Python pairings"""
    inp = dict(captured_inputs)
    from tests import pairing_model as PM
    inp["g1_vec"] = PM.g1_pack([K.g1_of(x) for x in inp["a"]])
    inp["rows"] = PM.g1_pack([K.g1_of(x) for x in inp["row_ks"]])
    inp["g2_pts"] = [K.g2_of(x) for x in inp["b"]]
    assert K.ark_bytes(K.points_of(inp), 4, 5) == captured


def test_setup_scalars_are_the_packages():
    from zolt_amd import api
    assert api.Dory.setupScalars(9) == K.setup_scalars(9)
    assert K.open_challenges(2) == [1, 100, 2, 101, 999]


def test_the_captured_g2_points_pin_the_sign_rules_component_order(captured_exponents):
    """fp2IsPositive compares c1 before c0 (dory.zig:320-344). A point tells the two orders apart when its y has c1 and c0 on different
    sides of their negatives; eight of the sixteen G2 points of the captured proof do, so the fixture pins the order."""
    ks = [m[5] for m in captured_exponents["first"]] + [k for m in captured_exponents["second"] for k in m[4:6]] + [captured_exponents["final"][1]]
    telling = []
    for k in ks:
        y = K.g2_of(k)[1]
        ny = G2.f2_neg(y)
        telling.append(((y[1], y[0]) <= (ny[1], ny[0])) != ((y[0], y[1]) <= (ny[0], ny[1])))
    assert len(ks) == 16 and sum(telling) == 8 and telling[1] and telling[-1]  # first[1].e2_beta and final.e2 among them


# ---------------------------------------------------------------- 2. (a) = (b) where the captured run does not reach
SHAPES = {(0, 0): dict(), (0, 1): dict(n_v=1), (1, 1): dict(identity_rows=(1,)), (0, 3): dict(n_v=5, n_rows=0),
          (1, 3): dict(n_rows=1, left_zero_tail=1, identity_g1=(2,)), (2, 2): dict(n_rows=3, identity_rows=(0,), n_v=3, left_zero_tail=2)}


@pytest.mark.parametrize("nu,sigma", sorted(SHAPES))
def test_the_two_models_agree(nu, sigma):
    """an identity row commitment, n_rows < 2^nu, n_v < 2^sigma, a zero tail in left_vec; (0, 3) and (1, 3) are where h < n2"""
    inp = K.make_inputs(nu, sigma, seed=300 + 16 * nu + sigma, **SHAPES[(nu, sigma)])
    assert K.same_records(K.render(K.exponents_of(inp)), K.points_of(inp))


@pytest.mark.parametrize("nu", [1, 2])
def test_point_model_is_open_with_transcript_for_equal_lengths(nu):
    """nu = sigma: open's loop is openWithTranscript's with the constants for challenges"""
    inp = K.make_inputs(nu, nu, seed=41 + nu, n_rows=(1 << nu) - 1)
    want = D.open_model(inp["g1_vec"], inp["g2_pts"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], nu, nu,
                        D.FixedChallenges(K.open_challenges(nu) + [0]))  # (the transcript's closing challenge is drawn and dropped)
    got = K.points_of(inp)
    assert K.same_records(got, want) and K.ark_bytes(got, nu, nu) == want["proof"]


# ---------------------------------------------------------------- 3. the round shapes of the device session
def test_round_shape_header_is_the_references_loop(tmp_path):
    """zolt_amd/csrc/dory_shape.h, compiled for the host with its own main under AddressSanitizer and UBSan, for every nu <= sigma <= 20"""
    exe = str(tmp_path / "dory_shape_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dory_shape_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    want = [(nu, sigma, t) + shape for sigma in range(21) for nu in range(sigma + 1) for t, shape in enumerate(K.schedule(nu, sigma))]
    assert got == want and len(got) == sum(s * (s + 1) for s in range(21))


def test_schedule_of_the_captured_shape():
    assert K.schedule(4, 5) == [(32, 16, 16, 16), (16, 8, 8, 8), (8, 4, 4, 4), (4, 2, 2, 2), (2, 1, 1, 1)]
    assert K.schedule(0, 3) == [(8, 4, 1, 1), (4, 2, 1, 1), (2, 1, 1, 1)]
    assert K.schedule(2, 4) == [(16, 8, 4, 4), (8, 4, 2, 2), (4, 2, 1, 1), (2, 1, 1, 1)]


# ---------------------------------------------------------------- 4. header, bindings, no device
def test_header_section_and_bindings():
    from zolt_amd import _abi, lib
    text = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "------ Dory opening (over a key, `open`) */" in text and "#define ZG_FEATURE_DORY_OPEN_KEY 512u" in text
    assert text.index("Dory verifier setup */") < text.index("Dory opening (over a key, `open`) */") < text.index("------ Pairings (engine) */")
    assert "#define ZG_ABI_MINOR 11\n" in text
    names = ["zg_dory_open_key_begin", "zg_dory_open_run"]
    assert all(n in lib.SYMBOLS and hasattr(lib._lib, n) for n in names)
    assert _abi.PROTOS["zg_dory_open_key_begin"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    assert _abi.PROTOS["zg_dory_open_run"] == (C.c_int, [C.c_void_p] * 5)
    assert _abi.ZG_FEATURE_DORY_OPEN_KEY == 512 and lib.abi_features() & 512 and lib.abi_version() == (1, 11)
    ffi = open(os.path.join(ROOT, "zig", "gpu", "ffi.zig")).read()
    assert "pub const FEATURE_DORY_OPEN_KEY: u32 = 512;" in ffi and all(f"pub extern fn {n}(" in ffi for n in names)


def test_refusals_need_no_device():
    from zolt_amd import lib
    out = np.full(26, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ch = np.zeros(8, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib._lib.zg_dory_open_run(None, p(ch), None, None, p(out)) != 0 and (out == 0xA5A5A5A5A5A5A5A5).all()
    h = C.c_void_p(1)
    vmv = np.zeros(105, dtype=np.uint64)
    assert lib._lib.zg_dory_open_key_begin(None, None, None, 0, None, 0, p(ch), p(ch), 0, 0, p(vmv), C.byref(h)) != 0 and not vmv.any()
