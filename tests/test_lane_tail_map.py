"""The index map of the lane-form row / column sums (zolt_amd/csrc/msm_lane_map.h) and the planner's tail rule (msm_plan.h: plan_tail) on
the CPU: plain g++ compiles tests/cpp/lane_tail_map_check.cpp against the headers with the address and undefined-behaviour sanitizers
and runs it (no GPU needed). For 6 x 6, 6 x 8 and 8 x 8 buckets the driver replays every thread of every stage: each bucket index
1 .. 2^(lb+hb) - 1 is read exactly once by the row pass and once by the column pass, every LDS slot is written once before the next
stage reads it and never while another unit reads it, and every row / column sum lands once in its rc slot."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "lane_tail_map_check.cpp")


def test_lane_tail_map(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    out = str(tmp_path / "lane_tail_map_check")
    # -Wno-unused-function: the planner header's other static functions are not called here. The sanitizer runtimes are linked
    # statically: the program stands alone, whatever else the environment loads into a process
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + CSRC, DRIVER, "-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZG_")}  # the driver sets the switches itself
    r = subprocess.run([out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "lane map ok", r.stdout + r.stderr
