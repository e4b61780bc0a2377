"""The sumcheck kernels' lazy Fr arithmetic (the Fr side of zolt_amd/csrc/fp29.hip.h) and their lazy 288-bit sums (acc9.hip.h) on the CPU,
function by function on raw limbs: tests/cpp/lazy_fr_host.cpp compiles the kernels' own headers for the host (hipcc --offload-host-only,
ZG_F29_SERIAL) and runs the record format of zg_selftest_lazy_fr over stdin / stdout — once as built, once more under
-fsanitize=address,undefined (a stand-alone program). The vectors, the model and the checker are tests/lazy_fr_model.py — the ones the
device test (tests/test_gpu_lazy_fr.py) uses, so this file pins them where no GPU exists. Every op except the block reduction.

    python -m pytest tests/test_lazy_fr_host.py -q -s --durations=0        # about twenty seconds, the two compiles included"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lazy_fr_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

def _compile(exe, extra=()):
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-DZG_F29_SERIAL", "-std=c++17", "-O1", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "lazy_fr_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)

    def run(op, items):
        res = subprocess.run([exe], input=f"{op} {len(items)}\n".encode() + fm.pack(items).tobytes(), capture_output=True)
        assert res.returncode == 0, (res.returncode, res.stderr.decode()[-2000:])
        return np.frombuffer(res.stdout, dtype=np.uint32).reshape(len(items), fm.OUT_WORDS)

    return run


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("lazy_fr_host") / "lazy_fr_host"))


@needs_hipcc
def test_mul(harness):
    """f29t_mul<Fr29> on raw limbs: a = A r - 1 against 32 (r - 1) for A = 1, 2, 4, the same integers with limbs raised to 2^30 - 1, k r,
    single limbs, eq_spartan_kernel's W = AB - 32 c + 64 r and psc_expr_kernel's pair sums at the top of their classes"""
    _, _, mx = fm.family(harness, fm.MUL)
    assert max(v for k, v in mx.items() if k.startswith("mul ")) < fm.OUT_MAX and mx["column bits"] <= 64


@needs_hipcc
def test_mul_short(harness):
    """f29t_mul_short<Fr29, 5> up to b = 2^145 - 1 and <Fr29, 3> up to b = 2^64 - 1; the limbs of b past NB are not read"""
    fm.family(harness, fm.MUL_SHORT5)
    fm.family(harness, fm.MUL_SHORT3)


@needs_hipcc
def test_canonical_entry_points(harness):
    """fr_mul29 with a prescaled factor, fr_mul29v, frmul_prepare / frmul_apply on both paths, fr29_in_shift, fr_from_u64_29, fr_from_mont29
    and the product by R2PRE: bit-equal to x y R^-1 mod r and to fe_mul; the narrow path is taken exactly when the low 128 bits are zero"""
    items, out, _ = fm.family(harness, fm.CANON)
    narrow = {it[0] for it, o in zip(items, out) if o[145]}
    assert {"y-zero", "rand-narrow", "narrow-H-1"} <= narrow and not any(k.startswith("one-low-word") or k in ("rand", "y-one-mont") for k in narrow), sorted(narrow)


@needs_hipcc
def test_sum64(harness):
    """acc29_add x count, acc29_reduce: up to FR29_ACC_MAX = 64 values of 2 r - 1"""
    _, _, mx = fm.family(harness, fm.SUM64)
    assert mx["sum64 in"] > fm.SUM_MAX - 1e-6  # the top of the class was reached


@needs_hipcc
def test_sum32(harness):
    """ChainAcc4: a carry pass every four additions, the in-loop flush at 64 followed by up to four more additions, the single-value flush"""
    fm.family(harness, fm.SUM32)


@needs_hipcc
def test_carry(harness):
    fm.family(harness, fm.CARRY)


@needs_hipcc
def test_acc9(harness):
    """acc9_reduce at k r + {-1, 0, 1, r/2, r - 1} up to k = floor(2^284 / r) and at 2^284 - 1; acc9_add / add_if / add_acc carrying through
    every limb into the ninth"""
    _, _, mx = fm.family(harness, fm.ACC9)
    assert mx["acc9 bits"] == 284


@needs_hipcc
def test_every_op_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined: a shift past a word's width, a signed overflow or
    an index past an array in the shipped functions ends the run with a report"""
    run = _compile(str(tmp_path / "lazy_fr_host_san"), extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for op in sorted(fm.N):
        items = fm.records_for(op, fm.SEED + op, 256)
        fm.check(op, items, run(op, items))


@needs_hipcc
def test_the_checker_can_fail(harness):
    """one limb, one flag, the narrow bit off: the checker says so (a checker that accepts everything would pass every test above)"""
    flips = {
        fm.MUL: [(0, 1), (8, 1), (9, 1), (16, 1 << 31)],
        fm.MUL_SHORT5: [(3, 1), (10, 2)],
        fm.CANON: [(0, 1), (9 + 7, 1), (18, 4), (27 + 8, 1), (36, 1), (45, 1), (63, 1), (72, 1), (145, 1)],
        fm.SUM64: [(0, 1), (7, 1 << 28), (145, 64 ^ 128)],
        fm.SUM32: [(0, 1), (9, 1), (18, 1), (27 + 7, 1), (144, 1), (145, 64 ^ 128)],
        fm.CARRY: [(0, 1), (8, 1)],
        fm.ACC9: [(0, 1), (7, 1), (9 + 8, 1), (18, 1), (27, 1), (36 + 8, 1)],
    }
    for op, cases in flips.items():
        items = fm.records_for(op, fm.SEED, 64)
        out = harness(op, items)
        fm.check(op, items, out)
        for word, delta in cases:
            for row in (0, 63):
                bad = out.copy()
                bad[row, word] ^= np.uint32(delta)
                with pytest.raises(AssertionError):
                    fm.check(op, items, bad)
    # an operand outside its class is refused before anything is compared
    items = fm.records_for(fm.MUL, fm.SEED, 8)
    kind, row, meta = items[0]
    row = row.copy()
    row[0] |= 1 << 30
    with pytest.raises(AssertionError):
        fm.assert_in_class(fm.MUL, [(kind, row, meta)])
    with pytest.raises(AssertionError):
        fm.acc9_reduce_model((1 << 286) - 1)  # outside S < 2^284: the quotient estimate no longer fits


def _source_array(text, name):
    return [[int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", body)] for body in re.findall(name + r"\[9\]\s*=\s*\{([^}]*)\}", text)]


def test_the_models_constants_are_what_r_derives_and_what_the_sources_hold():
    r = fm.R
    assert fm.val(fm.R29) == r and fm.wval([0xf0000001, 0x43e1f593, 0x79b97091, 0x2833e848]) == r % (1 << 128)
    assert fm.NINV == -pow(r, -1, 1 << 29) % (1 << 29)
    assert fm.C261 == fm.limbs((1 << 261) % r)
    assert fm.K343 == fm.limbs((1 << 343) % r)
    assert fm.R2PRE == fm.limbs(32 * ((1 << 512) % r) % r)  # the canonical 32 R^2 mod r: any representative below 32 r would do
    assert fm.MAGIC == (1 << 64) // -(-r // (1 << 224)) and -(-r // (1 << 224)) == 811880051
    # 64 r with limbs 0..7 raised by 2^30, the excess borrowed from the next limb: (bias - b) cannot underflow limb-wise for exact b
    assert fm.val(fm.BIAS64R) == 64 * r and all(x >= 1 << 30 for x in fm.BIAS64R[:8])
    assert fm.BIAS64R == [x + (1 << 30) - (2 if i else 0) for i, x in enumerate(fm.limbs(64 * r)[:8])] + [(64 * r >> 232) - 2]
    assert fm.H_MAX << 128 < r < (fm.H_MAX + 1) << 128 and fm.K_MAX == (1 << 284) // r
    # 2^261 / r, rounded down: the 168.9 of the product bound
    assert fm.MUL_DEN <= fm.Fraction(1 << 261, r)
    # ... and the sources hold the same numbers (C261 twice)
    fp29, poly, acc9 = (open(os.path.join(CSRC, f)).read() for f in ("fp29.hip.h", "poly.hip", "acc9.hip.h"))
    assert _source_array(fp29, "C261") == [fm.C261, fm.C261] and _source_array(fp29, "K343") == [fm.K343]
    assert _source_array(fp29, "R2PRE") == [fm.R2PRE] and _source_array(poly, "BIAS64R") == [fm.BIAS64R]
    assert fm.R29 in _source_array(fp29, r"P")
    assert re.findall(r"NINV = (0x[0-9a-f]+)u;\s*// -r\^-1", fp29) == [hex(fm.NINV).replace("0x", "0x0")]
    assert [int(x, 16) for x in re.findall(r"MAGIC = (0x[0-9a-f]+)ull", acc9)] == [fm.MAGIC]
    assert [int(x) for x in re.findall(r"FR29_ACC_MAX = (\d+);", fp29)] == [fm.FR29_ACC_MAX]
