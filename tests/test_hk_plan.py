"""The level plan of HyperKZG.open (zolt_amd/csrc/hk_plan.h) on the CPU: plain g++ compiles tests/cpp/hk_plan_check.cpp against the
header (no GPU needed).

- invariants over a grid of table sizes (0 .. 2^24, powers of two and not), points of 0 .. 34 variables (more than the fold can reach
  included), SRS lengths that clamp no, some or all commits, the three ZG_HK_FUSE_LONG modes, with and without helper streams: the
  folded levels are the reference loop's; every level has one destination, the one the loop chose before the plan existed; the
  regions of the arena are disjoint and inside it, and no fold writes past its region; a matrix's rows are consecutive levels, none
  longer than the first, their live lengths never growing; a matrix has at least two rows, the long one only with helper streams, mode 2's
  lone first level only with three long levels; what is zeroed is the matrices exactly; the arena is no larger than the two buffers it replaces;
- the plans of the benchmark's opening (2^20 evaluations on a 2^20-point SRS) in the three modes and of two clamped openings, pinned.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "hk_plan_check.cpp")

# Written out by hand from the loop as it stood before the plan: (n_evals, num_vars, SRS, mode) with helper streams ->
# the short matrix (first level + rows x row length @ arena offset), the long matrix, the levels with a buffer of their own
# (level @ offset : entries written), the long rows' live lengths, the arena.
# 2^20 on 2^20: the long levels 2^19 .. 2^15 are levels 0 .. 4, the fifteen short ones (16384 .. 1) follow; the matrices come first in
# the arena (15 * 16384 = 245760 entries of short rows), then the own buffers.
# 2^18 on 2^17: three long rows of at most 2^17. 2^19 on 2^17 in mode 2: the lone first level folds 2^18 pairs and commits 2^17 of them.
PINNED = [
    ((1 << 20, 20, 1 << 20, 0), "computed=20 small=5+15x16384@0 long=- own=0@245760:524288,1@770048:262144,2@1032192:131072,3@1163264:65536,4@1228800:32768 "
                                "rowlens=- arena=1261568"),
    ((1 << 20, 20, 1 << 20, 1), "computed=20 small=5+15x16384@0 long=0+5x524288@245760 own=- rowlens=524288,262144,131072,65536,32768 arena=2867200"),
    ((1 << 20, 20, 1 << 20, 2), "computed=20 small=5+15x16384@0 long=1+4x262144@245760 own=0@1294336:524288 rowlens=262144,131072,65536,32768 arena=1818624"),
    ((1 << 18, 18, 1 << 17, 1), "computed=18 small=3+15x16384@0 long=0+3x131072@245760 own=- rowlens=131072,65536,32768 arena=638976"),
    ((1 << 19, 19, 1 << 17, 2), "computed=19 small=4+15x16384@0 long=1+3x131072@245760 own=0@638976:262144 rowlens=131072,65536,32768 arena=901120"),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    out = str(tmp_path_factory.mktemp("hk_plan") / "hk_plan_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, DRIVER, "-o", out])
    return out


def _run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_plan_invariants(driver):
    out = _run(driver, "grid")
    assert out.startswith("grid ok"), out


def test_plan_invariants_under_sanitizers(tmp_path):
    """the same grid with the checker (a program of its own, host code only) built with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "hk_plan_check_san")
    subprocess.check_call([os.environ.get("CXX") or shutil.which("g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC, DRIVER, "-o", exe])
    assert _run(exe, "grid").startswith("grid ok")


@pytest.mark.parametrize("case,want", PINNED, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)
def test_plans_pinned(driver, case, want):
    assert _run(driver, "plan", *case, 1).strip() == want


def test_without_helper_streams_nothing_long_is_fused(driver):
    """no stream group: the long levels keep their own buffers in every mode, and the short matrix stays"""
    want = PINNED[0][1]
    for mode in (0, 1, 2):
        assert _run(driver, "plan", 1 << 20, 20, 1 << 20, mode, 0).strip() == want
