"""DoryCommitmentScheme.open on the device — a session begun over a resident key (zg_dory_open_key_begin) on open's asymmetric round
schedule, and the whole proof in one call (zg_dory_open_run) — against the joint opening proof the reference wrote into its own proof
file (tests/golden/dory_open_captured.bin), against the exponent model of tests/dory_open_key_model.py (pinned on that fixture and on
the point-level model by tests/test_dory_open_key_model.py), and against the session of zg_dory_open_begin where the two coincide.
Every case runs under both pairing engines; a model's records are computed once and shared."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import dory_open_key_model as K
from tests import g2_model as G2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
R = K.R


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(params=[0, 1], ids=["lane", "wave"])
def engine(zl, request):
    with zl.pairing_engine(request.param):
        yield request.param


def _key(zl, inp):
    return zl.DoryKey.create(inp["g1_vec"], inp["g2_vec"])


def _begin_key(zl, key, inp):
    return zl.DoryOpenSession.begin_key(key, inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]), G2.fr_pack(inp["left_vec"]), inp["nu"], inp["sigma"])


def _stepwise(ses, words):
    """the session driven call by call with the challenges of `words` ((4 sigma + 2, 4)) -> records"""
    ch = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    first, second = [], []
    for t in range(ses.sigma):
        first.append(ses.first_message())
        second.append(ses.second_message(ch[4 * t], ch[4 * t + 1]))
        ses.fold(ch[4 * t + 2], ch[4 * t + 3])
        assert len(ses) == 1 << (ses.sigma - t - 1)
    return {"vmv": ses.vmv, "first": first, "second": second, "final": ses.final(ch[4 * ses.sigma], ch[4 * ses.sigma + 1])}


def _run(ses, words):
    first, second, final = ses.run(words)
    assert len(ses) == 1
    return {"vmv": ses.vmv, "first": list(first), "second": list(second), "final": final}


def _open_run(zl, key, inp, words):
    ses = _begin_key(zl, key, inp)
    try:
        return _run(ses, words)
    finally:
        ses.close()


def _words(values):
    return K.challenge_words(values).reshape(-1, 4)


_MODEL, _INPUTS = {}, {}


def _inputs(nu, sigma, seed, **options):
    """K.make_inputs, made once for both engines (its points are Python scalar multiplications)"""
    name = (nu, sigma, seed, tuple(sorted(options.items())))
    if name not in _INPUTS:
        _INPUTS[name] = K.make_inputs(nu, sigma, seed=seed, **options)
    return _INPUTS[name]


def _model(name, inp, challenges=None):
    """the exponent model's records for a named input, computed once for both engines"""
    if name not in _MODEL:
        _MODEL[name] = K.render(K.exponents_of(inp, challenges))
    return _MODEL[name]


# ---------------------------------------------------------------- 1. the captured run: open(setup(9), bytecode_evals, point)
@pytest.fixture(scope="module")
def captured(zl):
    from zolt_amd import api
    with open(os.path.join(GOLDEN, "dory_open_captured.bin"), "rb") as f:
        want = f.read()
    with open(os.path.join(GOLDEN, "fibonacci.elf"), "rb") as f:
        code = f.read()[0x1000:0x1000 + 104]
    evals = G2.fr_pack(list(code) + [0] * 24)
    point = G2.fr_pack([(i + 1) * 12345 for i in range(9)])
    params = api.Dory.setup(9)
    key = api.Dory.key(params)
    yield {"want": want, "code": code, "evals": evals, "point": point, "params": params, "key": key}
    key.free()
    params.deinit()


def test_api_open_reproduces_the_captured_proof(zl, engine, captured):
    from zolt_amd import api
    assert (captured["params"].nu, captured["params"].sigma) == (4, 5) and captured["key"].lens() == (32, 16)
    proof = api.Dory.open(captured["key"], captured["evals"], captured["point"])
    assert len(proof.first_messages) == len(proof.second_messages) == 5
    assert proof.toArkBytes() == captured["want"]
    if engine == 0:  # and over the SetupParams, with a key of its own
        assert api.Dory.open(captured["params"], captured["evals"], captured["point"]).toArkBytes() == captured["want"]


def test_stepwise_calls_reproduce_the_captured_proof(zl, engine, captured):
    from zolt_amd import api
    params = captured["params"]
    rows = api.Dory.computeRowCommitments(params.g1_bases(), captured["evals"], 32)
    assert rows[0].shape[0] == 4
    left, right = api.Dory.computeEvaluationVectors(captured["point"], 4, 5)
    v = api.Dory.computeVectorMatrixProduct(captured["evals"], left, 4, 5)
    ses = zl.DoryOpenSession.begin_key(captured["key"], rows, v, right, left, 4, 5)
    rec = _stepwise(ses, api.Dory.openChallenges(5))
    ses.close()
    assert np.array_equal(api.Dory.openChallenges(5), _words(K.open_challenges(5)))
    assert api.DoryProof(rec["vmv"], rec["first"], rec["second"], rec["final"], 4, 5).toArkBytes() == captured["want"]
    # and with the reference's own row commitments handed over
    assert api.Dory.openWithRowCommitments(captured["key"], captured["evals"], captured["point"], rows).toArkBytes() == captured["want"]


@pytest.fixture(scope="module")
def cpp_mirror(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dory_open_key") / "test_dory_open_key_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dory_open_key_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    return exe


@pytest.mark.parametrize("name", ["lane", "wave"])
def test_cpp_open_reproduces_the_captured_proof(zl, captured, cpp_mirror, name):
    res = subprocess.run([cpp_mirror, captured["code"].hex()], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZG_PAIRING_ENGINE=name))
    assert res.returncode == 0, res.stdout + res.stderr
    got = [l.split()[1] for l in res.stdout.splitlines() if l.startswith("proof ")]
    assert got == [captured["want"].hex()]


# ---------------------------------------------------------------- 2. shapes against the exponent model
# (0, 3) and (2, 4): h < n2; (3, 7) and (6, 7): 128 entries on the G1 side against 8 / 64 on the G2 side — the 64-lane workgroup and wave
# boundaries are crossed on one side only
SHAPES = {(0, 0): dict(), (0, 1): dict(), (1, 1): dict(), (0, 3): dict(n_v=5), (2, 4): dict(n_rows=3, n_v=11, left_zero_tail=1), (3, 3): dict(identity_rows=(2,)),
          (3, 7): dict(n_rows=5, identity_g1=(70,)), (6, 7): dict(n_v=100, identity_rows=(0, 63))}


@pytest.mark.parametrize("nu,sigma", sorted(SHAPES))
def test_stepwise_and_run_equal_the_exponent_model(zl, engine, nu, sigma):
    inp = _inputs(nu, sigma, 500 + 32 * nu + sigma, **SHAPES[(nu, sigma)])
    want = _model(("shape", nu, sigma), inp)
    words = _words(K.open_challenges(sigma))
    key = _key(zl, inp)
    a = _begin_key(zl, key, inp)
    b = _begin_key(zl, key, inp)
    assert len(a) == len(b) == 1 << sigma
    step, run = _stepwise(a, words), _run(b, words)
    a.close()
    b.close()
    key.free()
    assert K.same_records(step, run)
    assert K.same_records(run, want)


# ---------------------------------------------------------------- 3. nu = sigma: the session of zg_dory_open_begin
@pytest.mark.parametrize("n", [3, 4])
def test_key_session_equals_the_plain_session_for_equal_lengths(zl, engine, n):
    inp = _inputs(n, n, 900 + n, n_rows=(1 << n) - 2)
    rng = random.Random(901 + n)
    words = _words([rng.randrange(1, R) for _ in range(2 * n + 1)])
    key = _key(zl, inp)
    a = _begin_key(zl, key, inp)
    b = zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]), G2.fr_pack(inp["left_vec"]), n, n)
    ra, rb = _stepwise(a, words), _stepwise(b, words)
    a.close()
    b.close()
    assert K.same_records(ra, rb)
    c = zl.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]), G2.fr_pack(inp["left_vec"]), n, n)
    rc = _run(c, words)  # run serves a session begun either way
    c.close()
    key.free()
    assert K.same_records(rc, rb)


# ---------------------------------------------------------------- 4. degenerate inputs
DEGENERATE = {"identity_rows_and_generators": ((2, 3), dict(identity_rows=(0, 3), identity_g1=(1, 6), identity_g2=(2,)), None),
              "identity_first_g2_generator": ((1, 2), dict(identity_g2=(0,)), None),
              "no_rows": ((1, 2), dict(n_rows=0), None),
              "few_rows": ((2, 2), dict(n_rows=3), None),
              "rows_past_2^sigma": ((1, 2), dict(n_rows=6), None),
              "no_v": ((1, 2), dict(n_v=0), None),
              "short_v": ((1, 3), dict(n_v=3), None),
              "zero_challenges": ((1, 2), dict(), [0, 7, 5, 0, 0])}  # beta_0 = alpha_1 = gamma = 0, each passed with inverse one


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_inputs_equal_the_exponent_model(zl, engine, name):
    (nu, sigma), options, challenges = DEGENERATE[name]
    inp = _inputs(nu, sigma, sum(name.encode()), **options)
    values = K.open_challenges(sigma) if challenges is None else challenges
    want = _model(("degenerate", name), inp, values)
    words = _words(values)
    if challenges is not None:
        one = G2.fr_pack([1])[0]
        assert not words[0].any() and np.array_equal(words[1], one) and not words[8].any() and np.array_equal(words[9], one)
    key = _key(zl, inp)
    a, b = _begin_key(zl, key, inp), _begin_key(zl, key, inp)
    step, run = _stepwise(a, words), _run(b, words)
    a.close()
    b.close()
    key.free()
    assert K.same_records(step, run) and K.same_records(run, want)


# ---------------------------------------------------------------- 5. refusals
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _raw_key_begin(zl, key_handle, inp, nu, sigma):
    a = {"rows": np.ascontiguousarray(inp["rows"][0]), "v": G2.fr_pack(inp["v_vec"]), "right": G2.fr_pack(inp["right_vec"]), "left": G2.fr_pack(inp["left_vec"]),
         "vmv": np.full(105, SENTINEL, dtype=np.uint64)}
    p = {k: v.ctypes.data_as(C.POINTER(C.c_uint64)) for k, v in a.items()}
    h = C.c_void_p(1)
    rc = zl._lib.zg_dory_open_key_begin(key_handle, p["rows"], None, C.c_size_t(a["rows"].shape[0]), p["v"], C.c_size_t(a["v"].shape[0]), p["right"], p["left"],
                                        C.c_uint32(nu), C.c_uint32(sigma), p["vmv"], C.byref(h))
    return rc, h.value, bool((a["vmv"] == SENTINEL).all())


def test_begin_refuses_and_writes_nothing(zl, engine):
    inp = _inputs(2, 3, 61)
    key = _key(zl, inp)  # 8 G1 and 4 G2 generators
    refused = (zl.ERR_INVALID, None, True)
    assert _raw_key_begin(zl, None, inp, 2, 3) == refused        # a NULL key
    assert _raw_key_begin(zl, key._h, inp, 3, 2) == refused      # nu > sigma
    assert _raw_key_begin(zl, key._h, inp, 2, 21) == refused     # sigma > 20
    assert _raw_key_begin(zl, key._h, inp, 2, 4) == refused      # n_g1 = 8 < 2^sigma
    assert _raw_key_begin(zl, key._h, inp, 3, 3) == refused      # n_g2 = 4 < 2^nu
    with pytest.raises(zl.ZgError) as err:
        zl.DoryOpenSession.begin_key(None, inp["rows"], G2.fr_pack(inp["v_vec"]), G2.fr_pack(inp["right_vec"]), G2.fr_pack(inp["left_vec"]), 2, 3)
    assert err.value.code == zl.ERR_INVALID
    # the key is still usable: the same arguments, whole, give the model's proof
    ses = _begin_key(zl, key, inp)
    got = _run(ses, _words(K.open_challenges(3)))
    ses.close()
    key.free()
    assert K.same_records(got, _model(("refusals", 2, 3), inp))


def test_run_only_right_after_begin_and_nothing_after_it(zl, engine):
    inp = _inputs(1, 2, 62)
    want = _model(("order", 1, 2), inp)
    words = _words(K.open_challenges(2))
    key = _key(zl, inp)
    a = _begin_key(zl, key, inp)
    first = a.first_message()
    with pytest.raises(zl.ZgError) as err:
        a.run(words)
    assert err.value.code == zl.ERR_INVALID and len(a) == 4
    # the refused call changed nothing: the session goes on call by call to the model's proof
    second = a.second_message(words[0], words[1])
    a.fold(words[2], words[3])
    with pytest.raises(zl.ZgError):
        a.run(words)  # nor in a later round
    rest_first, rest_second = a.first_message(), a.second_message(words[4], words[5])
    a.fold(words[6], words[7])
    final = a.final(words[8], words[9])
    assert K.same_records({"vmv": a.vmv, "first": [first, rest_first], "second": [second, rest_second], "final": final}, want)
    with pytest.raises(zl.ZgError):
        a.run(words)
    a.close()
    b = _begin_key(zl, key, inp)
    assert K.same_records(_run(b, words), want)
    one = G2.fr_pack([1])[0]
    for bad in (b.first_message, lambda: b.second_message(one, one), lambda: b.fold(one, one), lambda: b.final(one, one), lambda: b.run(words)):
        with pytest.raises(zl.ZgError) as err:
            bad()
        assert err.value.code == zl.ERR_INVALID
    assert len(b) == 1
    b.close()
    key.free()


def test_a_key_with_an_open_session_is_not_freed(zl, engine):
    inp = _inputs(1, 1, 63)
    key = _key(zl, inp)
    ses = _begin_key(zl, key, inp)
    with pytest.raises(zl.ZgError) as err:
        key.free()
    assert err.value.code == zl.ERR_INVALID and key.lens() == (2, 2)
    got = _run(ses, _words(K.open_challenges(1)))  # key and session are still whole
    assert K.same_records(got, _model(("free", 1, 1), inp))
    ses.close()
    key.free()
    assert key._h is None


# ---------------------------------------------------------------- 6. the key is only read
def test_commitments_over_the_key_are_unchanged_by_openings_and_two_sessions_share_it(zl, engine):
    inp_a = _inputs(2, 3, 71)
    inp_b = dict(_inputs(2, 3, 72, n_rows=2))
    for name in ("a", "b", "g1_vec", "g2_vec", "g2_pts"):
        inp_b[name] = inp_a[name]  # one key, two openings
    rng = random.Random(73)
    polys = [(zl.DORY_POLY_FR, G2.fr_pack([rng.randrange(R) for _ in range(32)]), None, 0, 0),
             (zl.DORY_POLY_U64, np.array([rng.randrange(1 << 64) for _ in range(32)], dtype=np.uint64), None, 0, 0)]
    key = _key(zl, inp_a)
    before = zl.dory_commit_batch(key, polys)
    a, b = _begin_key(zl, key, inp_a), _begin_key(zl, key, inp_b)  # open at once, driven in turn
    words = _words(K.open_challenges(3))
    fa, fb = a.first_message(), b.first_message()
    got_b = _open_run(zl, key, inp_b, words)
    during = zl.dory_commit_batch(key, polys)
    sa, sb = a.second_message(words[0], words[1]), b.second_message(words[0], words[1])
    a.close()
    b.close()
    got_a = _open_run(zl, key, inp_a, words)
    after = zl.dory_commit_batch(key, polys)
    key.free()
    want_a, want_b = _model(("shared", "a"), inp_a), _model(("shared", "b"), inp_b)
    assert np.array_equal(before, during) and np.array_equal(before, after)
    assert np.array_equal(fa, want_a["first"][0]) and np.array_equal(fb, want_b["first"][0])
    assert np.array_equal(sa, want_a["second"][0]) and np.array_equal(sb, want_b["second"][0])
    assert K.same_records(got_a, want_a) and K.same_records(got_b, want_b)


# ---------------------------------------------------------------- 7. the ABI
def test_feature_bit(zl):
    from zolt_amd import _abi
    assert zl.abi_features() & 512 and _abi.ZG_FEATURE_DORY_OPEN_KEY == 512
    assert zl.abi_version() == (1, 11)
