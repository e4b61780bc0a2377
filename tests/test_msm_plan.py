"""The MSM planner (zolt_amd/csrc/msm_plan.h) on the CPU: plain g++ compiles tests/cpp/msm_plan_check.cpp against the header, and the
driver runs under several switch sets (no GPU needed).

- invariants over a grid of handles (1 .. 2^27 bases, auto and forced window bits / levels, one-shot configs), their launches and point
  slices, and fused batches of 1 .. 32 vectors, wide or narrow: an LDS sort's counters fit 128 KiB; a two-pass plan has fb + rb = 31, a row
  reference that fits rb bits, at most 3000 coarse bins, at most 32 windows and at least ZG_MSM_FINE_BITS_MIN fine bits; every fused set
  sorts in LDS or in two passes; the workspace sizes cover every launch of the set;
- the round-6 fault: the long levels of HyperKZG.open on wide-window handles (tests/test_gpu_api_mirror.py::test_hyperkzg_open_long_levels)
  are fused into a two-pass set by default and not fused at all when the two-pass sort is off or refused;
- default plans of table and one-shot handles at 2^10 .. 2^24 bases, pinned.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "msm_plan_check.cpp")

SWITCH_SETS = [{}, {"ZG_MSM_TWO_PASS_SORT": "0"}, {"ZG_MSM_LDS_SORT": "0"}, {"ZG_MSM_FINE_BITS": "3", "ZG_MSM_FINE_BITS_MIN": "2"},
               {"ZG_MSM_FINE_BITS": "5", "ZG_MSM_FINE_BITS_MIN": "2"}, {"ZG_MSM_FINE_BITS_MIN": "8"}, {"ZG_MSM_TWO_PASS_SPAN": "256"},
               {"ZG_MSM_TWO_PASS_SPAN": "8192"}]

# parent-commit plans: bases, expected_uses, then c, W, L, G, sort (0 global-atomic, 1 LDS, 2 two-pass), fine bits, coarse bins,
# sort blocks, accumulate chunks
DEFAULT_PLANS = """
10 0 c=7 W=37 L=37 G=1 sort=1 fb=0 NCB=0 nblk=4 NT=4096
10 1 c=7 W=37 L=1 G=37 sort=1 fb=0 NCB=0 nblk=4 NT=4096
11 0 c=8 W=32 L=32 G=1 sort=1 fb=0 NCB=0 nblk=8 NT=4096
11 1 c=8 W=32 L=1 G=32 sort=1 fb=0 NCB=0 nblk=8 NT=4096
12 0 c=8 W=32 L=32 G=1 sort=1 fb=0 NCB=0 nblk=16 NT=8192
12 1 c=8 W=32 L=1 G=32 sort=1 fb=0 NCB=0 nblk=16 NT=8192
13 0 c=10 W=26 L=26 G=1 sort=1 fb=0 NCB=0 nblk=32 NT=16384
13 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=8 NT=16384
14 0 c=10 W=26 L=26 G=1 sort=1 fb=0 NCB=0 nblk=64 NT=32768
14 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=16 NT=32768
15 0 c=16 W=16 L=16 G=1 sort=2 fb=7 NCB=256 nblk=16 NT=32768
15 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=32 NT=65536
16 0 c=16 W=16 L=16 G=1 sort=2 fb=7 NCB=256 nblk=32 NT=65536
16 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=64 NT=131072
17 0 c=16 W=16 L=16 G=1 sort=2 fb=7 NCB=256 nblk=64 NT=131072
17 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=128 NT=131072
18 0 c=16 W=16 L=16 G=1 sort=2 fb=7 NCB=256 nblk=128 NT=131072
18 1 c=13 W=20 L=1 G=20 sort=2 fb=7 NCB=640 nblk=256 NT=131072
19 0 c=16 W=16 L=16 G=1 sort=2 fb=7 NCB=256 nblk=256 NT=131072
19 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=512 NT=131072
20 0 c=17 W=15 L=15 G=1 sort=2 fb=7 NCB=512 nblk=512 NT=131072
20 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=1024 NT=131072
21 0 c=17 W=15 L=15 G=1 sort=2 fb=6 NCB=1024 nblk=1024 NT=131072
21 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=2048 NT=131072
22 0 c=17 W=15 L=15 G=1 sort=2 fb=5 NCB=2048 nblk=2048 NT=131072
22 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=4096 NT=131072
23 0 c=16 W=16 L=16 G=1 sort=1 fb=0 NCB=0 nblk=256 NT=131072
23 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=8192 NT=131072
24 0 c=16 W=16 L=16 G=1 sort=1 fb=0 NCB=0 nblk=256 NT=131072
24 1 c=15 W=17 L=1 G=17 sort=2 fb=7 NCB=2176 nblk=16384 NT=131072
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    out = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, DRIVER, "-o", out])
    return out


def _run(driver, switches, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZG_")}  # only the switches under test
    env.update(switches)
    r = subprocess.run([driver, *map(str, args)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("switches", SWITCH_SETS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_plan_invariants(driver, switches):
    out = _run(driver, switches, "grid")
    assert out.startswith("grid ok"), out


# (SRS bases, row length, rows) of the fused long levels in test_hyperkzg_open_long_levels
LONG_LEVELS = [(1 << 17, 1 << 16, 2), (1 << 17, 1 << 17, 3), (1 << 18, 1 << 17, 3), (1 << 18, 1 << 16, 2)]


def test_long_levels_are_what_the_open_plans(tmp_path):
    """LONG_LEVELS against the level plan (zolt_amd/csrc/hk_plan.h, tests/cpp/hk_plan_check.cpp) of that test's (v, SRS bases, mode) cases
    with a fused long matrix"""
    import re
    out = str(tmp_path / "hk_plan_check")
    subprocess.check_call([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "hk_plan_check.cpp"), "-o", out])
    planned = set()
    for v, srs, mode in [(17, 1 << 17, 2), (18, 1 << 17, 2), (18, 1 << 18, 2), (18, 1 << 17, 1), (17, 1 << 17, 1), (18, 1 << 18, 1)]:
        rows, length = re.search(r" long=\d+\+(\d+)x(\d+)@", _run(out, {}, "plan", 1 << v, v, srs, mode, 1)).groups()
        planned.add((srs, int(length), int(rows)))
    assert planned == set(LONG_LEVELS)


@pytest.mark.parametrize("hn,n,k", LONG_LEVELS)
def test_round6_long_levels(driver, hn, n, k):
    assert _run(driver, {}, "fuse", hn, n, k, 1).split() == [str(k), "2"]  # fused, two-pass sort
    for off in ({"ZG_MSM_TWO_PASS_SORT": "0"}, {"ZG_MSM_FINE_BITS_MIN": "8"}):
        assert _run(driver, off, "fuse", hn, n, k, 1).split() == ["0", "-1"], off  # not fused: no LDS scatter over 2^16+ counters


def test_default_plans_pinned(driver):
    assert _run(driver, {}, "table").split("\n") == DEFAULT_PLANS.strip().split("\n") + [""]
