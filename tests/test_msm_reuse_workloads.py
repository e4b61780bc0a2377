"""The workloads of the MSM workspace-reuse walk (tests/msm_reuse_workloads.py) on the CPU, so that the device test that uses them
(tests/test_gpu_msm_workspace_reuse.py) stands on checked ground:

- closed form: for every workload over 2^10 bases, with and without infinity flags, (sum s_i k_i) * G equals the pinned oracle's MSM
  over the same bases, flags and scalars, byte for byte — generator, bases and closed form are held to the oracle without a device;
- census: with the plan of every configuration taken from the planner (tests/cpp/msm_plan_check.cpp, mode `plan`, under the
  configuration's switches), each workload leaves in a workspace what its table entry claims. These are conditions on the inputs, not
  measurements: if a configuration's size stops meeting them the test fails and the size has to change;
- walk: all_pairs_order(m) takes each of the m^2 ordered pairs exactly once, m = 2 .. 12.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import msm_reuse_workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "msm_plan_check.cpp")


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    out = str(tmp_path_factory.mktemp("msm_reuse") / "msm_plan_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, DRIVER, "-o", out])
    return out


def _plan(driver, conf, m=None):
    """the planner's line for the configuration's handle and a launch of m scalars on it, as a dict of integers"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZG_")}  # only the configuration's switches
    env.update(conf["env"])
    cfg = conf["cfg"]
    args = [conf["N"], cfg.get("window_bits", 0), cfg.get("precompute_levels", 0), cfg.get("expected_uses", 0)] + ([m] if m is not None else [])
    r = subprocess.run([driver, "plan", *map(str, args)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "flags"])
def test_closed_form_equals_the_oracle(ob, flagged):
    N, c = 1 << 10, 7
    xy = W.bases(ob.g1_gen_multiples(N // 2), N)
    flags = W.default_flags(N) if flagged else None
    ks = W.base_multipliers(N, flags)
    assert sum(W.base_multipliers(N)) == 0
    identities = 0
    for wl in W.workloads(N, c, extra=(("R200", "U", 100, 200), ("PBITS", "BITS", 0, 300))):
        name, off, n, ints = wl
        want = W.result_record(W.closed_form(ks, wl))
        got, ginf = ob.msm_g1(xy[off:off + n], None if flags is None else flags[off:off + n], W.fr_mont(ints))
        assert ginf == want[8] and np.array_equal(got, want[:8]), name
        identities += int(want[8])
    assert identities == (1 if flagged else 2)  # Z, and CANCEL where no flag breaks a pair


def test_bases_of_an_odd_handle(ob):
    """5003 bases (the sliced configuration): 2501 positive multiples, 2502 negative ones; CANCEL leaves the unpaired base out"""
    N = 5003
    gm = ob.g1_gen_multiples(N - N // 2)
    xy, ks = W.bases(gm, N), W.base_multipliers(N)
    assert ks[:3] == [1, 2, 3] and ks[N // 2 - 1] == N // 2 and ks[N // 2] == -1 and ks[-1] == -(N - N // 2)
    assert np.array_equal(xy[:N // 2], gm[:N // 2]) and np.array_equal(xy[N // 2:, :4], gm[:, :4])
    assert np.array_equal(xy[N // 2:, 4:], ob.f_neg(ob.FP, gm[:, 4:]))
    cancel = [wl for wl in W.workloads(N, 8) if wl[0] == "CANCEL"][0]
    assert W.closed_form(ks, cancel) is None and cancel[3][-1] == 0


def _launches(driver, conf, wl):
    """the launches one MSM over `wl` makes on the configuration's handle: [(the launch's part of the workload, its accumulate chunks)]"""
    name, off, n, ints = wl
    p = _plan(driver, conf, n)
    out = []
    for j in range(p["S"]):
        a = j * p["per"]
        cnt = min(p["per"], n - a)
        q = p if p["S"] == 1 else _plan(driver, conf, cnt)  # (a slice is shorter than two spans: a launch of its own)
        assert q["S"] == 1 and q["per"] == cnt
        out.append(((name, off + a, cnt, ints[a:a + cnt]), q["launch_NT"]))
    return p["S"], out


@pytest.mark.parametrize("name", list(W.CONFIGS))
def test_census_of_every_configuration(driver, name):
    conf = W.CONFIGS[name]
    p = _plan(driver, conf)
    print(name, p)
    assert {k: p[k] for k in conf["plan"]} == conf["plan"], p
    c, G, NB, NK = p["c"], p["G"], p["NB"], p["NK"]
    heavy_over = 8 if p["tail"] == 1 else 8 * p["GS"]  # msm_bucket_combine_lane_kernel / msm_bucket_combine_kernel
    seen = {"empty": 0, "light": 0, "heavy": 0, "huge": 0}
    for wl in W.workloads(conf["N"], c, extra=conf["extra"]):
        S, launches = _launches(driver, conf, wl)
        if wl[0] in conf.get("slices", {}):
            assert S == conf["slices"][wl[0]], (wl[0], S)
        elif "slices" not in conf:
            assert S == 1
        cs = [W.census(part, c, nt, G=G, heavy_over=heavy_over) for part, nt in launches]
        for x in cs:
            assert x["NK"] == NK and x["empty"] + x["light"] + x["heavy"] + x["huge"] == NK
            assert all(nt >= 1024 and x["total"] <= x["C"] * nt for _, nt in launches)
            for k in seen:
                seen[k] += x[k]
        tot = {k: sum(x[k] for x in cs) for k in seen}
        runs = [r for x in cs for r in x["runs"]]
        print(f"  {wl[0]:7s} off={wl[1]} n={wl[2]} launches={S} entries={sum(x['total'] for x in cs)} " + " ".join(f"{k}={v}" for k, v in tot.items())
              + f" most_partials={max([r[2] for r in runs] or [0])}")
        if wl[0] in ("Z", "PZ"):
            assert not runs
        elif wl[0] == "ONE":
            assert len(runs) == 1 and runs[0][1:] == (1, 1)
        elif wl[0] == "BITS":
            assert len({r[0] for r in runs}) == 1  # one bucket: digit 1 of window 0
            if conf["bits_huge"]:
                assert tot["huge"] >= 1
            else:
                assert tot["heavy"] == S and max(n for _, _, n, _ in [l[0] for l in launches]) <= W.HUGE_PARTIALS
        elif wl[0] == "BYTE":
            reachable = NB >= 256 and wl[2] // 256 > heavy_over
            assert conf["byte_heavy"] == reachable, (NB, wl[2], heavy_over)
            if conf["byte_heavy"]:
                assert tot["heavy"] >= 100 and tot["huge"] == 0 and tot["empty"] >= NK - 255
            elif NB >= 256:  # 16 quads a bucket: all of BYTE's buckets are light
                assert tot["heavy"] == 0 and tot["huge"] == 0 and tot["light"] >= 200
            else:  # c = 8: 129 .. 255 are negative digits, their carries pile into the bucket of digit 1 — one long run beside light ones
                assert tot["light"] >= 100 and tot["heavy"] + tot["huge"] == S
        elif wl[0] == "U":
            assert all(x["total"] > x["NK"] or x["empty"] < x["NK"] // 2 for x in cs)
        elif wl[0] == "SUB":
            assert S == 1 and launches[0][1] < p["NT"]  # fewer chunks than the workspace holds
    # every class of bucket occurs on this configuration (a slice of the sliced handle has 2048 chunks in all: none of its buckets is huge)
    assert all(v for k, v in seen.items() if k != "huge" or conf["bits_huge"]), seen


@pytest.mark.parametrize("name", list(W.CONFIGS))
def test_only_the_empty_and_the_cancelling_workloads_give_the_identity(name):
    """(EQ would on an even handle if it took every base: the k_i sum to zero)"""
    conf = W.CONFIGS[name]
    ks = W.base_multipliers(conf["N"])
    wls = W.workloads(conf["N"], conf["plan"]["c"], extra=conf["extra"])
    assert [w[0] for w in wls if W.closed_form(ks, w) is None] == [w[0] for w in wls if w[0] in ("Z", "CANCEL", "PZ")]


def test_byte_is_heavy_where_it_can_be():
    assert sorted(k for k, v in W.CONFIGS.items() if v["byte_heavy"]) == ["lane-tail-13", "lane-tail-15", "tableless", "two-pass"]


@pytest.mark.parametrize("m", range(2, 13))
def test_walk_takes_every_ordered_pair_once(m):
    walk = W.all_pairs_order(m)
    assert len(walk) == m * m + 1 and walk[0] == walk[-1] and set(walk) == set(range(m))
    pairs = list(zip(walk, walk[1:]))
    assert len(set(pairs)) == m * m == len(pairs)
