"""The lane functions of the Dory commitment kernels (zolt_amd/csrc/dory_commit.hip.h) on the CPU: tests/cpp/dory_commit_host.cpp compiles
the kernels' own header for the host (hipcc --offload-host-only, ZG_F29_SERIAL: the compiler forms of the products) and runs the digit
decode, the table build, a lane's row sum, the kernel's tree order and the Horner combine; the expected points are big-integer multiples
of the generator (tests/pairing_model.py).

    python -m pytest tests/test_dory_commit_host.py -q --durations=0        # about fifteen seconds, the compile included"""
import os
import shutil
import subprocess

import pytest

from tests import pairing_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP header")

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dory_commit_host") / "dory_commit_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-DZG_F29_SERIAL", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "dory_commit_host.cpp"), "-o", path], check=True, capture_output=True, text=True)
    return path


def _words(v):
    v = v * pm.MONT % pm.P
    return " ".join(f"{(v >> (64 * i)) & M64:x}" for i in range(4))


def _run(exe, scalars, queries):
    """scalars: a_c (0 = an identity generator); queries: (words, shift, bits, lanes, nvirt, entries, signs or None)
    -> [(digits, point or None)]"""
    text = [f"{len(scalars):x}"]
    for a in scalars:
        p = pm.g1_mul(pm.G1_GEN, a % R) if a % R else None
        text.append("1 " + _words(0) + " " + _words(0) if p is None else "0 " + _words(p[0]) + " " + _words(p[1]))
    for words, shift, bits, lanes, nvirt, entries, signs in queries:
        text.append(f"{words:x} {shift:x} {bits:x} {lanes:x} {nvirt:x} {1 if signs is not None else 0:x} {len(entries):x}")
        for i, e in enumerate(entries):
            text.append(f"{e & M64:x} {e >> 64:x} {signs[i] if signs is not None else 0:x}")
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True)
    lines = res.stdout.split("\n")
    out = []
    inv = pow(pm.MONT, -1, pm.P)
    for q in range(len(queries)):
        d, p = lines[2 * q].split(), lines[2 * q + 1].split()
        assert d[0] == "D" and p[0] == "P"
        w = [int(t, 16) for t in p[1:]]
        x = sum(w[1 + i] << (64 * i) for i in range(4)) * inv % pm.P
        y = sum(w[5 + i] << (64 * i) for i in range(4)) * inv % pm.P
        assert w[0] in (0, 1) and (w[0] == 0 or (x, y) == (0, 0))  # the identity is written x = y = 0
        out.append(([int(t, 16) for t in d[1:]], None if w[0] else (x, y)))
    return out


def _want(scalars, queries):
    out = []
    for words, shift, bits, lanes, nvirt, entries, signs in queries:
        digits = [(e & M64) & 255 if nvirt == 8 else (e >> shift) & ((1 << bits) - 1) for e in entries]
        vals = [(e & M64) if nvirt == 8 else d for e, d in zip(entries, digits)]
        s = sum((-v if signs is not None and signs[i] else v) * scalars[i] for i, v in enumerate(vals)) % R
        out.append((digits, pm.g1_mul(pm.G1_GEN, s) if s else None))
    return out


def _check(exe, scalars, queries):
    got, want = _run(exe, scalars, queries), _want(scalars, queries)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, (q, queries[q][:5], g, w)


def test_digit_decode_and_row_sums_on_a_generic_key(exe):
    import random
    rng = random.Random(7)
    scalars = [rng.randrange(1, R) for _ in range(16)]
    scalars[5] = 0  # an identity generator contributes nothing, whatever its digit
    e128 = [rng.getrandbits(128) for _ in range(16)]
    e64 = [rng.getrandbits(64) for _ in range(16)]
    sparse = [rng.getrandbits(128) if i % 5 == 0 else 0 for i in range(16)]
    queries = [(2, 60, 8, 4, 1, e128, None),        # an 8-bit field that straddles the two words of a 128-bit entry
               (2, 57, 8, 1, 1, e128, None), (2, 63, 2, 2, 1, e128, None),
               (2, 124, 4, 8, 1, e128, None),        # the top nibble: InstructionRa[0]
               (2, 120, 8, 16, 1, e128, None), (2, 0, 4, 4, 1, e128, None), (2, 64, 8, 4, 1, e128, None), (2, 56, 8, 4, 1, e128, None),
               (1, 60, 4, 2, 1, e64, None), (1, 56, 8, 1, 1, e64, None), (1, 0, 1, 4, 1, e64, None), (1, 13, 7, 8, 1, e64[:11], None),
               (2, 124, 4, 4, 1, sparse, None), (1, 0, 8, 4, 1, [0] * 9, None), (1, 3, 5, 64, 1, e64[:3], None)]
    _check(exe, scalars, queries)


def test_u64_bytes_signs_and_horner(exe):
    import random
    rng = random.Random(8)
    scalars = [rng.randrange(1, R) for _ in range(8)]
    words = [M64, 255 << 56, 0, 1, rng.getrandbits(64), 1 << 63, 0x0100, rng.getrandbits(64)]  # byte 7 of 2^64 - 1; only byte 7 set
    signs = [1, 0, 1, 1, 0, 1, 0, 1]  # (a negative zero among them)
    _check(exe, scalars, [(1, 0, 0, 1, 8, words, None), (1, 0, 0, 2, 8, words, signs), (1, 0, 0, 8, 8, words, signs), (1, 0, 0, 4, 8, [0] * 8, [1] * 8),
                          (1, 0, 0, 1, 8, words[:1], [1])])


def test_partial_sums_that_meet_the_next_table_entry(exe):
    """every generator the same point: a lane's accumulator equals the next row (the doubling) or its negative (the identity), in the
    lane loop (one lane) and in the tree (lanes that each hold the same point)"""
    scalars = [1] * 8
    ones = [1] * 8
    queries = [(1, 0, 8, 1, 1, ones, None),                                  # G + G: the doubling inside the lane loop, then 2G + G ...
               (1, 0, 8, 1, 1, [1, 1, 2, 4, 8, 16, 32, 64], None),           # acc = 2G meets T[2] = 2G, 4G meets 4G, ...
               (1, 0, 8, 2, 1, ones, None), (1, 0, 8, 8, 1, ones, None),      # the same inside the tree
               (1, 0, 8, 4, 1, [3, 1, 2, 2, 5, 1, 3, 3], None),
               (1, 0, 0, 1, 8, ones, [0, 1, 0, 1, 0, 1, 0, 1]),               # G - G: the identity inside the lane loop, then a fresh start
               (1, 0, 0, 2, 8, ones, [0, 1, 0, 1, 0, 1, 0, 1]),               # lanes hold 4G and -4G: the identity in the tree
               (1, 0, 0, 8, 8, [2, 2, 1, 1, 7, 7, 9, 9], [0, 1, 1, 0, 0, 1, 1, 0]),
               (1, 0, 0, 1, 8, [1, 1, 2, 4], [0, 0, 0, 1]),                   # G + G = 2G, + 2G = 4G, - 4G = identity
               (1, 0, 0, 1, 8, [M64, M64, 1 << 56, 1 << 56], [0, 1, 0, 0])]   # the Horner doublings from byte 7 with cancelling low bytes
    _check(exe, scalars, queries)
    # related generators with different multiples: g1 = 2 g0, so T[0][2] = T[1][1] and T[0][4] = T[1][2]
    _check(exe, [1, 2, 4, R - 1], [(1, 0, 8, 1, 1, [2, 1, 1, 8], None), (1, 0, 8, 2, 1, [4, 2, 3, 12], None), (1, 0, 8, 4, 1, [6, 3, 0, 12], None),
                                    (1, 0, 8, 1, 1, [5, 0, 0, 5], None)])
