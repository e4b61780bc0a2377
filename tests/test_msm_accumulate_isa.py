"""Static guard on the instruction mix of the MSM accumulate loop (no GPU needed: hipcc cross-compiles for gfx950).

The mixed addition's ten products run in groups of independent ones (fp29.hip.h: f29_mul_x2 ...), one multiply-add chain
per column, seeded with its carry. Written one product at a time, hipcc splits every column into two chains and joins them
with a v_lshl_add_u64 (144 of them per addition). This test keeps a compiler upgrade from bringing those joins back
unnoticed, and keeps the kernel inside two waves per SIMD without scratch.

Two device-only compiles of msm.hip: the regular one (registers, scratch) and one with ZG_EXP_NOSLOW, which drops the
exceptional-case branch, so that the loop's blocks of field products are exactly the fast path.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
KERNEL = "_ZN2zg27msm_accumulate_chunk_kernelILb0EEEvPKjS2_S2_S2_PKcjjPc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def _compile(tmp, name, flags):
    out = os.path.join(tmp, name + ".s")
    cmd = [_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I" + CSRC, *flags,
           os.path.join(CSRC, "msm.hip"), "-o", out]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT), out


def _blocks(asm):
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.amdhsa_kernel " + KERNEL))
    blocks, cur = [], []
    for l in lines[start + 1:end]:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            blocks.append(cur)
            cur = []
            continue
        s = l.strip()
        if s and not s.startswith((";", ".")):
            cur.append(re.sub(r"_e(32|64)$", "", s.split()[0]))
    blocks.append(cur)
    return [collections.Counter(b) for b in blocks]


def _meta(asm, key):
    m = re.search(r"\.set " + re.escape(KERNEL) + r"\." + key + r", (\d+)", asm)
    assert m, key
    return int(m.group(1))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not _hipcc():
        pytest.skip("hipcc not found")
    tmp = str(tmp_path_factory.mktemp("isa"))
    jobs = {"regular": _compile(tmp, "regular", []), "noslow": _compile(tmp, "noslow", ["-DZG_EXP_NOSLOW"])}
    res = {}
    for k, (p, out) in jobs.items():
        log = p.communicate(timeout=900)[0].decode(errors="replace")
        assert p.returncode == 0, log[-4000:]
        with open(out) as f:
            res[k] = f.read()
    return res


def test_accumulate_registers_and_scratch(isa):
    asm = isa["regular"]
    assert _meta(asm, "num_vgpr") + _meta(asm, "num_agpr") <= 256  # two waves per SIMD
    assert _meta(asm, "private_seg_size") == 0  # no spills


def test_accumulate_fast_path_mix(isa):
    prod = [b for b in _blocks(isa["noslow"]) if b["v_mad_u64_u32"] >= 100]  # the blocks of field products
    tot = sum(prod, collections.Counter())
    # ten products per mixed addition: 2 x 162 (U2, S2) + 2 x 126 (PP, R^2) + 4 x 162 (PPP, Q, ZZ3, ZZZ3) + 243 (Y3)
    assert tot["v_mad_u64_u32"] == 1467, dict(tot)
    assert tot["v_lshl_add_u64"] <= 4, dict(tot)  # chain joins: 144 in the one-product-at-a-time schedule
    valu = sum(v for k, v in tot.items() if k.startswith("v_"))
    # issue slots of the fast path (VALU + s_nop): 2274 in the one-product-at-a-time schedule
    assert valu + tot["s_nop"] <= 2220, dict(tot)
