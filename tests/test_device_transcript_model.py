"""Fiat-Shamir lane functions without a GPU: the Blake2b transcript and the batched-sumcheck round step of zolt_amd/csrc/blake2b.hip.h compiled
for the host (tests/cpp/blake2b_host.cpp) against the model (tests/fs_model.py: hashlib and Python integers) — Blake2b-256 around every block
boundary, every transcript operation, the reference's own transcript log, the 125-bit mask, and the round step on random values and on the
rounds the reference printed for Stages 2 and 3 — once as built, once as a stand-alone program under -fsanitize=address,undefined. The
model alone is held against the reference's log, its printed rounds and api.Blake2bTranscript without a compiler, and the header is
compiled (not run) for gfx950.

    python -m pytest tests/test_device_transcript_model.py -q --durations=0"""
import json
import os
import random
import struct

import pytest

from tests import fs_model as M

ROOT = M.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _need_hipcc():
    if not os.path.exists(M.HIPCC):
        pytest.skip("hipcc is absent: the host harness compiles the kernels' own HIP header")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    _need_hipcc()
    return M.compile_host(str(tmp_path_factory.mktemp("blake2b_host") / "blake2b_host"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    _need_hipcc()
    return M.compile_host(str(tmp_path_factory.mktemp("blake2b_host_san") / "blake2b_host_san"),
                          extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def le(hexstr):
    return int.from_bytes(bytes.fromhex(hexstr), "little")


# ---- the model alone (no compiler)
def test_model_on_the_reference_log_and_against_the_host_mirror():
    from zolt_amd import api
    g = json.load(open(os.path.join(GOLDEN, "blake2b_transcript_preamble.json")))
    t = M.Transcript(g["label"].encode())
    assert t.state.hex() == g["initial_state_hex"]
    for o in g["ops"]:
        if "state_before_prefix" in o:
            assert t.state.hex().startswith(o["state_before_prefix"])
        t.append_u64(o["value"]) if o["op"] == "appendU64" else t.append_bytes(bytes.fromhex(o["hex"]))
        if "state_after_prefix" in o:
            assert t.state.hex().startswith(o["state_after_prefix"])
    assert t.state.hex().startswith(g["state_prefix_after_all_ops"])
    h, t = api.Blake2bTranscript(b"Jolt"), M.Transcript(b"Jolt")
    for k in range(4):  # the two readings of the 16 challenge bytes differ in byte order
        h.appendScalar(api.fr_from_int(k + 7))
        t.append_scalar(k + 7)
        assert [int(x) for x in h.challengeScalarFull()] == M.limbs(t.challenge_scalar_full())
        assert [int(x) for x in h.challengeScalar()] == t.challenge_scalar_words()
        assert (h.state, h.n_rounds) == (t.state, t.n_rounds)


def test_model_on_the_captured_rounds():
    _, recs = _stage_records()
    assert len(recs) >= 24 + 8
    for claim, c0, c2, c3, r, nxt in recs:
        assert M.next_claim(claim, c0, c2, c3, r) == nxt and M.limbs(r)[:2] == [0, 0]


def test_header_compiles_for_gfx950(tmp_path):
    """compiled only: the lane functions are verified on the host, and this keeps a host-only change from going unnoticed"""
    import subprocess
    _need_hipcc()
    subprocess.run([M.HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    "-c", os.path.join(ROOT, "tests", "cpp", "blake2b_device_compile.hip"), "-o", str(tmp_path / "blake2b_device.o")], check=True, capture_output=True, text=True)


# ---- Blake2b-256
def _hashes(exe):
    msgs = [M.message(n) for n in M.LENGTHS] + [bytes(128), b"\xff" * 129]
    got = M.host_hashes(exe, msgs)
    for m, g in zip(msgs, got):
        assert g == M.blake(m), len(m)
    return got


def test_blake2b_at_every_block_boundary(exe):
    """0, 1, 63 .. 4096 bytes: a message of exactly 128 (256, 4096) bytes ends in a FULL block that is compressed as the final one"""
    _hashes(exe)


# ---- the transcript
def _script():
    """every operation, the one-block (64-byte payload) and two-block (65) inputs, and the counter across 255 -> 256 and 65535 -> 65536"""
    rnd = random.Random(11)
    sc = [rnd.randrange(M.R_MOD) for _ in range(4)] + [0, 1, M.R_MOD - 1]
    s = [("init", b"Jolt"), ("u64", struct.pack("<Q", 4096)), ("message", b"UniPoly_begin"), ("message", b""), ("message", b"x" * 32)]
    s += [("bytes", M.message(n, 9)) for n in (0, 1, 31, 32, 63, 64, 65, 127, 128, 192, 193, 448, 4096)]
    s += [("scalar", struct.pack("<4Q", *M.limbs(v))) for v in sc]
    s += [("challenge", b""), ("challenge_full", b""), ("u64", struct.pack("<Q", 2**64 - 1)), ("challenge", b"")]
    for n0 in (254, 65534):
        s += [("import", M.blake(b"state %d" % n0) + struct.pack("<I", n0)), ("u64", struct.pack("<Q", 7)), ("bytes", b"abc"), ("challenge", b""),
              ("scalar", struct.pack("<4Q", *M.limbs(5)))]
    s += [("init", b""), ("init", b"a"), ("init", b"b" * 31), ("init", b"c" * 32), ("challenge_full", b"")]
    s += [("init", b"d" * 40), ("message", b"e" * 40), ("challenge", b"")]  # too long: cut to 32 bytes, never a wrapped padding count
    return s


def _model_script(script):
    t, out = M.Transcript(b""), []
    for op, p in script:
        res = [0, 0, 0, 0]
        if op == "init":
            t = M.Transcript(p[:32])
        elif op == "import":
            t = M.Transcript(state=p[:32], n_rounds=struct.unpack("<I", p[32:])[0])
        elif op == "bytes":
            t.append_bytes(p)
        elif op == "message":
            t.append_message(p[:32])
        elif op == "u64":
            t.append_u64(struct.unpack("<Q", p)[0])
        elif op == "scalar":
            t.append_scalar(M.unlimbs(struct.unpack("<4Q", p)))
        elif op == "challenge":
            res = t.challenge_scalar_words()
        else:
            res = M.limbs(t.challenge_scalar_full())
        out.append((res, t.state, t.n_rounds))
    return out


def _transcript(exe):
    script = _script()
    got, want = M.host_script(exe, script), _model_script(script)
    for (op, p), g, w in zip(script, got, want):
        assert g == w, (op, len(p))
    rounds = [g[2] for g in got]
    assert 256 in rounds and 65536 in rounds and 65537 in rounds
    return got


def test_every_transcript_operation(exe):
    _transcript(exe)


def test_the_reference_transcript_log(exe):
    """tests/golden/blake2b_transcript_preamble.json: the states the reference printed for its preamble"""
    g = json.load(open(os.path.join(GOLDEN, "blake2b_transcript_preamble.json")))
    script = [("init", g["label"].encode())]
    for o in g["ops"]:
        script.append(("u64", struct.pack("<Q", o["value"])) if o["op"] == "appendU64" else ("bytes", bytes.fromhex(o["hex"])))
    got = M.host_script(exe, script)
    assert got[0][1].hex() == g["initial_state_hex"]
    for k, o in enumerate(g["ops"]):
        if "state_after_prefix" in o:
            assert got[k][1].hex().startswith(o["state_before_prefix"]) and got[k + 1][1].hex().startswith(o["state_after_prefix"]), k
    assert got[-1][1].hex().startswith(g["state_prefix_after_all_ops"])


def test_64_challenges_limb_for_limb_and_the_mask_at_work(exe):
    script = [("init", b"Jolt")] + [("challenge", b"")] * 64
    got = M.host_script(exe, script)[1:]
    t = M.Transcript(b"Jolt")
    masked = 0
    for g in got:
        before = M.Transcript(state=t.state, n_rounds=t.n_rounds).challenge_u128()
        masked += before >> 125 != 0
        w = t.challenge_scalar_words()
        assert g[0] == w and w[:2] == [0, 0] and w[3] < 1 << 61 and g[1] == t.state
    assert masked >= 32, masked


# ---- the round step
def _random_batches():
    rnd = random.Random(5)
    f = lambda: rnd.randrange(M.R_MOD)  # noqa: E731
    out = []
    for rule in (0, 1):
        for sample in (1, 2):
            inst = [{"num_rounds": n, "kind": k, "claim": f(), "coeff": f()} for n, k in ((5, M.EVALS_ALL), (4, M.DERIVE_1), (2, M.DERIVE_13), (5, M.QUADRATIC))]
            out.append((inst, rule, sample, [[[f() for _ in range(4)] for _ in inst] for _ in range(5)]))
    out.append(([{"num_rounds": 1, "kind": M.DERIVE_13, "claim": f(), "coeff": f()}], 0, 1, [[[f() for _ in range(4)]]]))
    out.append(([{"num_rounds": 3, "kind": k % 4, "claim": f(), "coeff": f()} for k in range(8)], 1, 2, [[[f() for _ in range(4)] for _ in range(8)] for _ in range(3)]))
    return out


def _round_steps(exe):
    results = []
    for inst, rule, setup, sums in _random_batches():
        b, t = M.Batch(inst, rule), M.Transcript(b"rounds")
        got = M.host_rounds(exe, b, t, setup, sums)
        b.setup(t, setup == 2)
        for j, (S, state, n_rounds, log) in enumerate(got):
            if j:
                comp, rw = b.step(t, sums[j - 1])
                assert log == sum((M.limbs(v) for v in comp), []) + rw, j
                assert list(S["r"]) == rw
            assert list(S["claim"]) == M.limbs(b.claim) and state == t.state and n_rounds == t.n_rounds and int(S["round"]) == b.round, j
            for n, i in enumerate(b.inst):
                assert list(S["inst_claim"][n]) == M.limbs(i["claim"]) and list(S["coeff"][n]) == M.limbs(i["coeff"]), (j, n)
        results.append([(S.tobytes(), st) for S, st, _, _ in got])
    return results


def test_round_step_on_random_values(exe):
    """the four kinds, instances that join late under both inactive rules, given and sampled coefficients, claims that are NOT the sums"""
    _round_steps(exe)


def _stage_records():
    s2 = json.load(open(os.path.join(GOLDEN, "stage2_batched_rounds.json")))
    s3 = json.load(open(os.path.join(GOLDEN, "stage3_batched_rounds.json")))
    recs = [(le(r["current_claim"]), le(r["c0"]), le(r["c2"]), le(r["c3"]), le(r["challenge"]), le(r["next_claim"])) for r in s2["rounds"]]
    claim = sum(int(c, 16) * le(v) for c, v in zip(s3["batching_coeffs_be"], s3["input_claims"])) % M.R_MOD  # equal round counts: no power of two
    for r in s3["rounds"]:
        recs.append((claim, le(r["c0"]), le(r["c2"]), le(r["c3"]), le(r["challenge"]), le(r["next_claim"])))
        claim = le(r["next_claim"])
    return s2, recs


def _captured(exe):
    s2, recs = _stage_records()
    assert len(recs) >= 24 + 8
    for claim, c0, c2, c3, r, nxt in recs:
        assert M.next_claim(claim, c0, c2, c3, r) == nxt  # the model on the reference's own numbers
        assert M.limbs(r)[:2] == [0, 0]                   # a challenge's Montgomery words are the raw limbs [0, 0, lo, hi]
    got = M.host_next_claims(exe, [(c, c0, c2, c3, M.limbs(r)) for c, c0, c2, c3, r, _ in recs])
    assert got == [nxt for *_, nxt in recs]
    # setupBatching's combined claim from the captured claims, round counts and coefficients
    inst = [{"num_rounds": n, "kind": M.EVALS_ALL, "claim": le(c), "coeff": le(k)} for n, c, k in zip(s2["num_rounds"], s2["input_claims"], s2["batching_coeffs"])]
    S = M.host_rounds(exe, M.Batch(inst), M.Transcript(b"Jolt"), 1, [])[0][0]
    assert list(S["claim"]) == M.limbs(le(s2["initial_batched_claim"]))
    return got


def test_round_step_on_the_captured_stage2_and_stage3_rounds(exe):
    """claim, c0 / c2 / c3, challenge -> next claim as the reference printed them, c1 taken from the claim"""
    _captured(exe)


def test_the_same_program_under_asan_and_ubsan(exe, exe_san):
    assert _hashes(exe_san) == _hashes(exe)
    assert _transcript(exe_san) == _transcript(exe)
    assert _round_steps(exe_san) == _round_steps(exe)
    assert _captured(exe_san) == _captured(exe)
