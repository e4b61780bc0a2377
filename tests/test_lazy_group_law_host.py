"""The lazy-limb group law of the MSM (zolt_amd/csrc/fp29.hip.h, g1_29.hip.h) on the CPU: tests/cpp/lazy_g1_host.cpp compiles the kernels'
own headers for the host (hipcc --offload-host-only, ZG_F29_SERIAL: the compiler forms of the products) and runs the record format of
zg_selftest_lazy_g1 over stdin / stdout. The vectors, the model and the checker are tests/lazy_model.py — the ones the device test
(tests/test_gpu_lazy_group_law.py) uses, so this file pins them where no GPU exists. Every op except the inline-assembly product forms and
the four-lane ops.

    python -m pytest tests/test_lazy_group_law_host.py -q --durations=0        # about ten seconds, the compile included"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lazy_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

SEED = 20260


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lazy_g1_host") / "lazy_g1_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-DZG_F29_SERIAL", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lazy_g1_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)

    def run(op, items):
        res = subprocess.run([exe], input=f"{op} {len(items)}\n".encode() + lm.pack(items).tobytes(), capture_output=True, check=True)
        return np.frombuffer(res.stdout, dtype=np.uint32).reshape(len(items), lm.OUT_WORDS)

    return run


def _family(harness, op, n, need):
    items = lm.records_for(op, SEED + op, n)
    assert len(items) == n
    lm.assert_in_class(op, items)
    kinds = {it[0] for it in items}
    assert all(any(k.startswith(w) for k in kinds) for w in need), (sorted(kinds), need)
    out = harness(op, items)
    mx = lm.check(op, items, out, device=False)
    print(f"{lm.OP_NAMES[op]}: {n} records, largest outputs / p: {dict(mx)}")
    return items, out


def test_madd(harness):
    """xyzz29_madd_nz + xyzz29_madd_except: both signs, acc == +-P for every representative of acc.x, forced limb patterns, run-start y"""
    _family(harness, lm.MADD, 512, ["regular+", "regular-", "double+", "double-", "infinity+", "infinity-", "run-start", "forced-x-double", "forced-x-infinity",
                                    "forced-y", "forced-zz", "forced-zzz", "forced-y-2p"])


def test_start(harness):
    _family(harness, lm.START, 256, ["regular++", "regular--", "double+-", "double-+", "infinity++", "infinity-+"])


def test_add(harness):
    _family(harness, lm.ADD, 512, ["regular", "double", "double-same", "infinity", "identity-a", "identity-b", "identity-both", "forced-x-double", "forced-zzz"])


def test_dbl_and_jdbl(harness):
    _family(harness, lm.DBL, 256, ["regular", "identity", "forced-x", "forced-y"])
    _family(harness, lm.JDBL, 256, ["zero", "top", "forced-x", "forced-y", "forced-z"])


def test_prod_compiler_forms(harness):
    _family(harness, lm.PROD, 1024, ["worst", "forced", "top-exact", "rand"])


def test_lin(harness):
    """the biased subtractions, the small multiples, f29_to_fp and the zero test, each alone on raw limbs"""
    items, out = _family(harness, lm.LIN, 2048, ["zero-0p", "zero-16p", "zero-17p", "near-0p-raised", "near-7p", "sub-extreme", "x3-extreme", "to-fp-edge", "random"])
    # the zero test said yes to k * p, k = 0..16, and to nothing else (the checker asserted each; this counts them)
    yes = [it[0] for it, o in zip(items, out) if o[144]]
    assert sorted(set(yes) - {"to-fp-edge"}) == sorted(f"zero-{k}p" for k in range(17)), sorted(set(yes))  # (0, p and 15p are to-fp edges too)
    # records on which a zero test that forgets the carry between limbs answers differently: a raised limb under k = 0
    raised = [it for it in items if it[0] == "near-0p-raised"]
    assert len(raised) >= 20 and all(int(it[1][:9].max()) >= 1 << 29 for it in raised)


def test_the_checker_can_fail(harness):
    """one limb, one flag, one lane off: the checker says so (a checker that accepts everything would pass every test above)"""
    items = lm.records_for(lm.MADD, SEED, 64)
    out = harness(lm.MADD, items).copy()
    lm.check(lm.MADD, items, out, device=False)
    reg = next(i for i, it in enumerate(items) if lm.branch(it[0]) == "regular")
    exc = next(i for i, it in enumerate(items) if lm.branch(it[0]) == "double")
    for row, word, delta in ((reg, 0, 1), (reg, 9 + 3, 1), (reg, 18, 1), (reg, 8, 1 << 20), (exc, 144, 1), (exc, 145, 1), (reg, 144, 2)):
        bad = out.copy()
        bad[row, word] ^= np.uint32(delta)
        with pytest.raises(AssertionError):
            lm.check(lm.MADD, items, bad, device=False)


def test_the_model_is_bn254_g1():
    """the checker's own group law against closed forms: the generator's order, a point of the chain, associativity"""
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    assert lm.on_curve(lm.G) and lm.val(lm.limbs(lm.ACC_X - 1)) == lm.ACC_X - 1

    def mul(p, k):
        acc = None
        for bit in bin(k)[2:]:
            acc = lm.double(acc)
            if bit == "1":
                acc = lm.add(acc, p)
        return acc

    assert mul(lm.G, r) is None and mul(lm.G, r - 1) == lm.neg(lm.G)
    g = lm.Gen(1)
    a, b, c = g.point(), g.point(), g.point()
    assert a == mul(lm.G, 4) and lm.add(lm.add(a, b), c) == lm.add(a, lm.add(b, c)) and lm.on_curve(lm.add(a, b))
    assert lm.add(a, lm.neg(a)) is None and lm.add(a, a) == lm.double(a)
    # fp29.hip.h's constants restated from p: ONE = 2^261 mod p, and 2^261 / p (the 168.9 of the product bound, rounded down)
    assert lm.limbs(lm.MONT % lm.P)[0] == 0x157ccc21 and lm.MONT // lm.P >= 168
