"""Dory opening proofs on the device (zg_dory_open_*: lib.DoryOpenSession, api.Dory.openWithTranscript) against the big-integer model of
tests/dory_open_model.py (pinned by tests/test_dory_open_model.py) and against the same proof composed from the per-call entry points.

The model costs about 22 ms per Miller loop and 45 ms per final exponentiation on a CPU, which puts the (4, 4) case at about 6 s: nothing
larger runs against it. Larger shapes are held to the per-call device route (tools/bench_dory_open.py: per_call_open), whose pieces have
their own model tests (tests/test_gpu_g2.py, tests/test_gpu_pairing.py)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import dory_open_model as D
from tests import g2_model as G2
from tests import pairing_model as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = D.R


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def bench():
    from tools import bench_dory_open
    return bench_dory_open


def _begin(zl, inp):
    return zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]),
                                    G2.fr_pack(inp["left_vec"]), inp["nu"], inp["sigma"])


def _same_state(got, want):
    (v1, v1i), (v2, v2i), s1, s2 = got
    (w1, w1i), w2, ws1, ws2 = want
    return (np.array_equal(v1i, w1i) and np.array_equal(v1, w1) and G2.unpack(v2, v2i) == w2  # identities carry x = y = 0 on both sides
            and G2.fr_unpack(s1) == ws1 and G2.fr_unpack(s2) == ws2)


# ---------------------------------------------------------------- 1. every message, the state after every fold and the proof bytes
CASES = {(1, 1): dict(), (2, 2): dict(zero_v=(1,)), (2, 3): dict(n_rows=3, n_v=7, zero_v=(2,), left_zero_tail=1), (4, 4): dict(zero_v=(0, 5), left_zero_tail=3)}


@pytest.mark.parametrize("nu,sigma", sorted(CASES))
def test_session_equals_the_model(zl, nu, sigma):
    from zolt_amd import api
    inp = D.make_inputs(nu, sigma, seed=1000 + 16 * nu + sigma, **CASES[(nu, sigma)])
    want = D.run_model(inp, D.Transcript(b"Jolt"))
    tr = api.Blake2bTranscript(b"Jolt")
    ses = _begin(zl, inp)
    assert len(ses) == 1 << sigma
    vmv = ses.vmv
    assert np.array_equal(vmv, want["vmv"])
    tr.appendGT(vmv[0:48])
    tr.appendGT(vmv[48:96])
    tr.appendG1Compressed((vmv[96:104], int(vmv[104])))
    firsts, seconds = [], []
    for rnd in range(sigma):
        m = ses.first_message()
        assert np.array_equal(m, want["first"][rnd]), rnd
        firsts.append(m)
        for k in range(4):
            tr.appendGT(m[48 * k:48 * k + 48])
        tr.appendG1Compressed((m[192:200], int(m[200])))
        tr.appendG2Compressed((m[201:217], int(m[217])))
        beta = tr.challengeScalar()
        assert np.array_equal(beta, want["challenges"][rnd][0])
        beta_inv = api.Dory.inverseOrOne(beta)
        assert np.array_equal(beta_inv, want["challenges"][rnd][1])
        m = ses.second_message(beta, beta_inv)
        assert np.array_equal(m, want["second"][rnd]), rnd
        seconds.append(m)
        tr.appendGT(m[0:48])
        tr.appendGT(m[48:96])
        tr.appendG1Compressed((m[96:104], int(m[104])))
        tr.appendG1Compressed((m[105:113], int(m[113])))
        tr.appendG2Compressed((m[114:130], int(m[130])))
        tr.appendG2Compressed((m[131:147], int(m[147])))
        alpha = tr.challengeScalar()
        ses.fold(alpha, api.Dory.inverseOrOne(alpha))
        assert len(ses) == 1 << (sigma - rnd - 1)
        assert _same_state(ses.state(), want["states"][rnd]), rnd
    gamma = tr.challengeScalar()
    final = ses.final(gamma, api.Dory.inverseOrOne(gamma))
    assert np.array_equal(final, want["final"])
    ses.close()
    assert api.DoryProof(vmv, firsts, seconds, final, nu, sigma).toBytes() == want["proof"]


def test_open_with_transcript_from_evaluations(zl):
    """api.Dory.openWithTranscript end to end at (2, 2): row commitments, evaluation vectors and the vector-matrix product from the
    package's own pieces, the proof bytes against the model fed with the oracle's restatements of the same three"""
    from oracle import binding as ob
    from zolt_amd import api
    nu = sigma = 2
    inp = D.make_inputs(nu, sigma, seed=77)
    rng = random.Random(78)
    evals = G2.fr_pack([rng.randrange(R) for _ in range(1 << (nu + sigma))])
    point = G2.fr_pack([rng.randrange(R) for _ in range(nu + sigma)])
    params = api.Dory.SetupParams(inp["g1_vec"], inp["g2_vec"], nu, sigma)
    tr = api.Blake2bTranscript(b"Jolt")
    proof = api.Dory.openWithTranscript(params, evals, point, None, tr)
    params.deinit()
    left, right = ob.dory_evaluation_vectors(point, nu, sigma)
    rows = ob.dory_row_commitments(inp["g1_vec"][0], None, evals, 1 << sigma)
    v = ob.dory_vector_matrix_product(evals, left, nu, sigma)
    mt = D.Transcript(b"Jolt")
    want = D.open_model(inp["g1_vec"], inp["g2_pts"], rows, G2.fr_unpack(v), G2.fr_unpack(right), G2.fr_unpack(left), nu, sigma, mt)
    assert proof.toBytes() == want["proof"]
    assert tr.state == mt.state and tr.n_rounds == mt.n_rounds  # both transcripts end in the same place


# ---------------------------------------------------------------- 2. the session against the per-call composition
def test_session_equals_the_per_call_composition_at_64(zl, bench):
    """sigma = nu = 6: segments of 32 and later 16, 8, ... pairs starting at unequal alignments inside the 64-lane blocks of the Miller
    launch, MSMs of 64 points; one seed drives both routes"""
    inp = bench.make_inputs(6, 6, seed=606, n_rows=50)
    inp["v_vec"][3] = 0
    a, b = bench.session_open(inp), bench.per_call_open(inp)
    assert np.array_equal(a[0], b[0])
    for rnd in range(6):
        assert np.array_equal(a[1][rnd], b[1][rnd]), ("first", rnd)
        assert np.array_equal(a[2][rnd], b[2][rnd]), ("second", rnd)
    assert np.array_equal(a[3], b[3])


# ---------------------------------------------------------------- 3. segment and challenge edges
def test_identity_half_and_zero_beta_at_128(zl, bench):
    """cur = 128 (two 64-lane blocks per segment... one per product here, four products) with v1 all identities on its right half: d1_right is
    one; with beta = 0 and beta_inv = one, as the host's `inverse() orelse one` hands them over, v1 stays as it is, so c_minus is one and
    e1_minus the identity record. The other values against the per-call route."""
    from zolt_amd import api
    inp = bench.make_inputs(7, 7, seed=707, n_rows=64)
    one = PM.gt_pack([PM.ONE])[0]
    zero, fr_one = np.zeros(4, dtype=np.uint64), api.fr_from_int(1)
    ses = zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], 7, 7)
    (v1, v1i), (v2, v2i), s1, s2 = ses.state()
    assert list(v1i) == [0] * 64 + [1] * 64
    m = ses.first_message()
    g1, g2 = inp["g1_vec"], inp["g2_vec"]
    want = api.Dory.multiPairBatch([((v1[:64], v1i[:64]), (g2[0][:64], g2[1][:64])), ((g1[0][:64], g1[1][:64]), (v2[:64], v2i[:64])),
                                    ((g1[0][:64], g1[1][:64]), (v2[64:], v2i[64:]))])
    assert np.array_equal(m[0:48], want[0]) and np.array_equal(m[48:96], one)
    assert np.array_equal(m[96:144], want[1]) and np.array_equal(m[144:192], want[2])
    m2 = ses.second_message(zero, fr_one)
    (u1, u1i), (u2, u2i), _, _ = ses.state()
    assert np.array_equal(u1i, v1i) and np.array_equal(u1[:64], v1[:64])  # beta = 0: v1 unchanged
    w2 = zl.g2_axpy_batch(g2[0][:128], g2[1][:128], v2, v2i, fr_one)  # beta_inv = one: v2[i] += g2_vec[i]
    assert np.array_equal(u2, w2[0]) and np.array_equal(u2i, w2[1])
    c_plus = api.Dory.multiPairG1G2((u1[:64], u1i[:64]), (u2[64:], u2i[64:]))
    assert np.array_equal(m2[0:48], c_plus) and np.array_equal(m2[48:96], one)
    ident = np.zeros(9, dtype=np.uint64)
    ident[8] = 1
    assert np.array_equal(m2[105:114], ident)  # e1_minus = MSM(identities, s2[0..64])
    e2_minus = api.Dory.msmG2((u2[:64], u2i[:64]), s1[64:])
    assert np.array_equal(m2[131:147], e2_minus[0]) and int(m2[147]) == e2_minus[1]
    ses.close()


def test_one_pair_per_product_and_zero_beta_against_the_model(zl):
    """sigma = 1: the first message at cur = 2 pairs one entry per product; beta = 0 -> (0, one), alpha = 0 -> (0, one) through the fold"""
    inp = D.make_inputs(1, 1, seed=11)
    want = D.run_model(inp, D.FixedChallenges([0, 0, 12345, 0]))
    ses = _begin(zl, inp)
    assert np.array_equal(ses.vmv, want["vmv"])
    assert np.array_equal(ses.first_message(), want["first"][0])
    beta, beta_inv, alpha, alpha_inv = want["challenges"][0]
    assert not beta.any() and np.array_equal(beta_inv, G2.fr_pack([1])[0]) and not alpha.any()
    assert np.array_equal(ses.second_message(beta, beta_inv), want["second"][0])
    ses.fold(alpha, alpha_inv)
    assert _same_state(ses.state(), want["states"][0])
    assert np.array_equal(ses.final(want["gamma"], want["gamma_inv"]), want["final"])
    ses.close()


# ---------------------------------------------------------------- 4. errors
def _raw_begin(zl, inp, nu, sigma, n_gens=None, null=()):
    a = {"g1": np.ascontiguousarray(inp["g1_vec"][0]), "g2": np.ascontiguousarray(inp["g2_vec"][0]), "rows": np.ascontiguousarray(inp["rows"][0]),
         "v": G2.fr_pack(inp["v_vec"]), "right": G2.fr_pack(inp["right_vec"]), "left": G2.fr_pack(inp["left_vec"]), "vmv": np.zeros(105, dtype=np.uint64)}
    p = {k: (None if k in null else v.ctypes.data_as(C.POINTER(C.c_uint64))) for k, v in a.items()}
    h = C.c_void_p()
    rc = zl._lib.zg_dory_open_begin(p["g1"], None, p["g2"], None, C.c_size_t(a["g1"].shape[0] if n_gens is None else n_gens), p["rows"], None,
                                    C.c_size_t(a["rows"].shape[0]), p["v"], C.c_size_t(a["v"].shape[0]), p["right"], p["left"], C.c_uint32(nu),
                                    C.c_uint32(sigma), p["vmv"], C.byref(h))
    return rc, h.value


def test_begin_refuses_bad_arguments_and_leaves_no_session(zl):
    inp = D.make_inputs(2, 2, seed=5)
    assert _raw_begin(zl, inp, 3, 2) == (zl.ERR_INVALID, None)  # nu > sigma
    assert _raw_begin(zl, inp, 2, 2, n_gens=3) == (zl.ERR_INVALID, None)  # generator vectors shorter than 2^sigma
    assert _raw_begin(zl, inp, 2, 3) == (zl.ERR_INVALID, None)  # 2^sigma = 8 > the four generators
    for name in ("g1", "g2", "rows", "v", "right", "left", "vmv"):
        assert _raw_begin(zl, inp, 2, 2, null=(name,)) == (zl.ERR_INVALID, None), name
    rc, h = _raw_begin(zl, inp, 2, 2)  # and the same arguments, whole, open a session
    assert rc == 0 and h
    assert zl._lib.zg_dory_open_close(C.c_void_p(h)) == 0


def test_calls_out_of_order_are_errors_and_closing_mid_proof_is_clean(zl):
    inp = D.make_inputs(1, 1, seed=6)
    one = G2.fr_pack([1])[0]
    ses = _begin(zl, inp)
    for bad in (lambda: ses.second_message(one, one), lambda: ses.fold(one, one), lambda: ses.final(one, one)):
        with pytest.raises(zl.ZgError) as err:
            bad()
        assert err.value.code == zl.ERR_INVALID
    first = ses.first_message()
    with pytest.raises(zl.ZgError):
        ses.first_message()
    with pytest.raises(zl.ZgError):
        ses.fold(one, one)
    second = ses.second_message(one, one)
    with pytest.raises(zl.ZgError):
        ses.second_message(one, one)
    with pytest.raises(zl.ZgError):
        ses.final(one, one)
    ses.close()  # mid-proof: before the fold
    ses.close()  # and closing twice is nothing
    # the refused calls changed nothing: a fresh session gives the same messages
    again = _begin(zl, inp)
    assert np.array_equal(again.first_message(), first) and np.array_equal(again.second_message(one, one), second)
    again.fold(one, one)
    again.close()  # with a fold in flight
    with pytest.raises(zl.ZgError):
        zl.DoryOpenSession(None, None, 1).first_message()


def test_flagged_row_commitments_are_identities_whatever_their_coordinates(zl):
    """a row commitment flagged as the identity enters v1 as the reference's identity (x = y = 0), and the messages are those of the same
    opening with that row's coordinates zeroed by the caller"""
    inp = D.make_inputs(2, 2, seed=21)
    flags = np.array([0, 1, 0, 0], dtype=np.uint8)
    clean = inp["rows"][0].copy()
    clean[1] = 0
    got = []
    for xy in (inp["rows"][0], clean):
        ses = zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], (xy, flags), G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]),
                                       G2.fr_pack(inp["left_vec"]), 2, 2)
        (v1, v1i), _, _, _ = ses.state()
        assert list(v1i) == [0, 1, 0, 0] and not v1[1].any() and np.array_equal(v1[[0, 2, 3]], clean[[0, 2, 3]])
        got.append((ses.vmv, ses.first_message()))
        ses.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_state_hooks_answer_only_for_an_open_session(zl):
    """the read-back takes its handle as a data word of zg_field_op: a word that is no open session's handle — field data under a stray op
    code, a session that was closed — is refused before anything is read through it, and so is any field but Fr or a second operand"""
    inp = D.make_inputs(1, 1, seed=8)
    ses = _begin(zl, inp)
    handle = ses._h.value
    out = np.zeros((2, 4), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731

    def hook(word, field=zl.FR, b=None, op=zl.OP_DORY_S1):
        return zl._lib.zg_field_op(C.c_int(field), C.c_int(op), ptr(word), b, ptr(out), C.c_size_t(2))

    mine = np.array([handle], dtype=np.uint64)
    assert hook(mine) == 0 and np.array_equal(out, G2.fr_pack(inp["right_vec"]))
    stray = G2.fr_pack([12345, 6789])  # field elements, as a caller of the element-wise ops would pass them
    for op in (zl.OP_DORY_V1, zl.OP_DORY_V2, zl.OP_DORY_S1, zl.OP_DORY_S2):
        assert hook(stray, op=op) == zl.ERR_INVALID
    assert hook(np.array([handle + 8], dtype=np.uint64)) == zl.ERR_INVALID
    assert hook(mine, field=zl.FP) == zl.ERR_INVALID and hook(mine, b=ptr(stray)) == zl.ERR_INVALID
    ses.close()
    assert hook(mine) == zl.ERR_INVALID  # closed: no longer anybody's handle
    with pytest.raises(zl.ZgError):
        ses.wait()


# ---------------------------------------------------------------- 5. the ABI
def test_feature_bit(zl):
    from zolt_amd import _abi
    assert zl.abi_features() & 32 and _abi.ZG_FEATURE_DORY_OPEN == 32
    assert zl.abi_version() == (1, 11)
    assert (_abi.ZG_DORY_VMV_WORDS, _abi.ZG_DORY_FIRST_WORDS, _abi.ZG_DORY_SECOND_WORDS, _abi.ZG_DORY_FINAL_WORDS) == (105, 218, 148, 26)


# ---------------------------------------------------------------- 6. the C++ mirror
def test_cpp_dory_open_mirror(zl, tmp_path):
    """tests/cpp/test_dory_open_mirror.cpp prints zolt::Dory::openWithTranscript's proof bytes for a fixed input; the Python mirror gives
    the same bytes for the same input"""
    from zolt_amd import api
    exe = str(tmp_path / "test_dory_open_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dory_open_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    got = [l.split()[1] for l in res.stdout.splitlines() if l.startswith("proof ")]
    assert len(got) == 1
    # the same fixed input: nu = 2, sigma = 3, g1_vec[i] = (i + 1) G, g2_vec[i] = (7 i + 3) H, evals[j] = 1000 + 17 j, point[k] = 5 + 3 k
    nu, sigma = 2, 3
    n = 1 << sigma
    g1 = zl.g1_fixed_base_mul_batch(api.generator(), G2.fr_pack([i + 1 for i in range(n)]))
    g2 = zl.g2_fixed_base_mul_batch(api.g2_generator(), G2.fr_pack([7 * i + 3 for i in range(n)]))
    evals = G2.fr_pack([1000 + 17 * j for j in range(1 << (nu + sigma))])
    point = G2.fr_pack([5 + 3 * k for k in range(nu + sigma)])
    params = api.Dory.SetupParams(g1, g2, nu, sigma)
    proof = api.Dory.openWithTranscript(params, evals, point, None, api.Blake2bTranscript(b"Jolt"))
    params.deinit()
    assert got[0] == proof.toBytes().hex()
    assert len(proof.toBytes()) == 800 + 4 + sigma * (1632 + 960) + 96 + 8
