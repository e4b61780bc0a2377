"""The pairing as one lane of the device computes it (zolt_amd/csrc/fp12.hip.h, pairing.hip.h) on the CPU: tests/cpp/pairing_host.cpp
compiles the kernels' own headers for the host (hipcc --offload-host-only) and runs them on records; tests/pairing_model.py is the checker.
What only the device has — the kernels' indexing, the product tree, the entry points — is tests/test_gpu_pairing.py's.

    python -m pytest tests/test_pairing_host.py -q --durations=0        # a few seconds, the compile included"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import g2_model as G2
from tests import pairing_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")
P, R = M.P, M.R
OP_MUL, OP_SQR, OP_INV, OP_CONJ, OP_FROB1, OP_FROB2, OP_FROB3, OP_EXP_X = range(17, 25)
OP_MILLER, OP_FINAL_EXP, OP_MUL_BY_034 = 100, 101, 102


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairing_host") / "pairing_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pairing_host.cpp"), "-o", out],
                   check=True, capture_output=True, text=True)
    return out


def _run(exe, op, a, b=None):
    """a, b: (n, 48) uint64 operands -> [Fp12] results"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 48)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 48)
    rec = np.concatenate([a, b], axis=1)
    res = subprocess.run([exe], input=b"%d %d\n" % (op, a.shape[0]) + rec.tobytes(), capture_output=True, check=True)
    return M.gt_unpack(np.frombuffer(res.stdout, dtype=np.uint64).reshape(-1, 48))


def _inputs():
    rng = random.Random(12)
    edge = [M.ZERO, M.ONE, tuple([(P - 1, P - 1)] * 6)]
    for k in range(6):
        for c in ((1, 0), (0, 1), (rng.randrange(P), rng.randrange(P))):
            f = [(0, 0)] * 6
            f[k] = c
            edge.append(tuple(f))
    rand = lambda: tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))  # noqa: E731
    a = edge + [rand() for _ in range(40)]
    b = [rand() for _ in edge] + edge + [rand() for _ in range(40 - len(edge))]
    return a, b


def test_tower_ops(exe):
    a, b = _inputs()
    pa, pb = M.gt_pack(a), M.gt_pack(b)
    assert _run(exe, OP_MUL, pa, pb) == [M.mul(u, v) for u, v in zip(a, b)]
    assert _run(exe, OP_SQR, pa) == [M.sqr(u) for u in a]
    inv = _run(exe, OP_INV, pa)
    assert inv == [M.inv(u) for u in a] and inv[0] == M.ZERO
    assert _run(exe, OP_CONJ, pa) == [M.conj(u) for u in a]
    for n, op in ((1, OP_FROB1), (2, OP_FROB2), (3, OP_FROB3)):
        assert _run(exe, op, pa) == [M.frobenius(u, n) for u in a], n
    assert _run(exe, OP_EXP_X, pa[:6]) == [M.exp_by_x(u) for u in a[:6]]


def test_mul_by_034(exe):
    a, b = _inputs()
    want = [M.mul_by_034(u, v[0], v[2], v[4]) for u, v in zip(a, b)]  # b's first three Fp2 in memory: the coefficients of w^0, w^2, w^4
    assert _run(exe, OP_MUL_BY_034, M.gt_pack(a), M.gt_pack(b)) == want


def test_miller_loop_and_final_exponentiation(exe):
    rng = random.Random(3)
    ps = [M.G1_GEN] + [M.g1_mul(M.G1_GEN, rng.randrange(1, R)) for _ in range(3)]
    qs = [G2.G] + [G2.scalar_mul(G2.G, rng.randrange(1, R)) for _ in range(3)]
    rec = np.zeros((4, 48), dtype=np.uint64)
    rec[:, :8] = M.g1_pack(ps)[0]
    rec[:, 8:24] = G2.pack(qs)[0]
    got = _run(exe, OP_MILLER, rec)
    want = [M.miller_loop(p, q) for p, q in zip(ps, qs)]
    assert got == want  # the unreduced value: the same step formulas and digits
    fe = _run(exe, OP_FINAL_EXP, M.gt_pack(want + [M.ZERO, M.ONE]))
    assert fe == [M.final_exponentiation(m) for m in want] + [M.ONE, M.ONE]
    assert M.to_bytes(fe[0])[:16].hex() == "950e879d73631f5eb5788589eb5f7ef8"  # tests/golden/pairing_generator_jolt.json
