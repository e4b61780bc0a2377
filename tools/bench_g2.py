#!/usr/bin/env python3
"""G2 entry points against their G1 yardsticks (needs a GPU). Writes profiles/g2_bench.json.

Host-pointer call time: a host clock around the synchronous call (it ends in a stream synchronise inside the library) — warm-up, `--reps`
repeats, median and the min / max spread. Kernel-only time comes from a separate profiler run per size, never from the same run:

    python tools/bench_g2.py --out profiles/g2_bench.json                                        # call times, ratios
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/n1024 -- python tools/bench_g2.py --sizes 1024 --reps 5 --profiled DIR/n1024
    python tools/bench_g2.py --merge DIR --out profiles/g2_bench.json                            # adds kernel_ms from DIR/n*/

Columns at every n: each new entry point; the parent commit's G1 entry point that does the same job at the same n
(zg_g1_scalar_mul_batch, zg_g1_fixed_base_mul_batch, zg_msm_g1 on a table-less handle, expected_uses = 1) and the ratio G2 / G1; and
msm_g2 against n x (scalar_mul_batch per-element time), which is what the reference's msmG2 loop costs in this library's own units."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the kernels one call of an entry point launches (stable names, for the profiler's per-kernel statistics)
KERNELS = {
    "g2_scalar_mul_batch": ["scalar_mul_kernel<G2>"],
    "g2_fixed_base_mul_batch": ["g2_fb_window_bases_kernel", "g2_fb_rows_kernel", "g2_fb_mul_kernel"],
    "g2_axpy_batch": ["axpy_kernel<G2>"],
    "g2_affine_add_batch": ["g2_affine_add_kernel"],
    "g2_is_on_curve_batch": ["on_curve_kernel<G2>"],
    "msm_g2": ["g2_msm_digits_kernel", "g2_msm_bucket_kernel", "g2_msm_bitsum_kernel", "g2_msm_final_kernel"],
    "g1_axpy_batch": ["axpy_kernel<G1>"],
    "g1_scalar_mul_batch": ["scalar_mul_kernel<G1>"],
    "g1_fixed_base_mul_batch": ["fb_window_bases_kernel", "fb_table_rows_kernel", "fb_mul_kernel"],
    "g1_affine_add_batch": ["g1_affine_add_kernel"],
    "msm_g1_tableless": ["msm_"],  # every kernel of the G1 MSM launch set (prefix match)
}
PAIRS = [("g2_scalar_mul_batch", "g1_scalar_mul_batch"), ("g2_fixed_base_mul_batch", "g1_fixed_base_mul_batch"), ("g2_axpy_batch", "g1_axpy_batch"),
         ("g2_affine_add_batch", "g1_affine_add_batch"), ("msm_g2", "msm_g1_tableless")]


def fr_random(rng, n):
    from zolt_amd import lib
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] >>= np.uint64(2)  # below the modulus
    return lib.field_op(lib.FR, lib.OP_TO_MONT, raw)


def run(sizes, reps, warmup):
    from zolt_amd import api, lib
    lib.init()
    rng = np.random.default_rng(7)
    out = {}
    for n in sizes:
        sc, ks = fr_random(rng, n), fr_random(rng, n)
        s1 = sc[0]
        g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), ks)
        g2b = lib.g2_fixed_base_mul_batch(api.g2_generator(), sc)
        g1 = lib.g1_fixed_base_mul_batch(api.generator(), ks)
        g1b = lib.g1_fixed_base_mul_batch(api.generator(), sc)
        h = lib.Bases.upload(g1[0], g1[1], expected_uses=1)
        d_xy, d_sc, d_out = lib.DeviceBuffer.from_host(g2[0]), lib.DeviceBuffer.from_host(sc), lib.DeviceBuffer(17 * 8)
        calls = {
            "g2_is_on_curve_batch": lambda: lib.g2_is_on_curve_batch(g2[0], g2[1]),
            "g2_affine_add_batch": lambda: lib.g2_affine_add_batch(g2[0], g2[1], g2b[0], g2b[1]),
            "g2_scalar_mul_batch": lambda: lib.g2_scalar_mul_batch(g2[0], g2[1], sc),
            "g2_fixed_base_mul_batch": lambda: lib.g2_fixed_base_mul_batch(api.g2_generator(), sc),
            "g2_axpy_batch": lambda: lib.g2_axpy_batch(g2[0], g2[1], g2b[0], g2b[1], s1),
            "g1_axpy_batch": lambda: lib.g1_axpy_batch(g1[0], g1[1], g1b[0], g1b[1], s1),
            "msm_g2": lambda: lib.msm_g2(g2[0], g2[1], sc),
            "msm_g2_dev": lambda: (lib.msm_g2_dev(d_xy.ptr, 0, d_sc.ptr, n, d_out.ptr), lib.sync()),
            "g1_affine_add_batch": lambda: lib.g1_affine_add_batch(g1[0], g1[1], g1b[0], g1b[1]),
            "g1_scalar_mul_batch": lambda: lib.g1_scalar_mul_batch(g1[0], g1[1], sc),
            "g1_fixed_base_mul_batch": lambda: lib.g1_fixed_base_mul_batch(api.generator(), sc),
            "msm_g1_tableless": lambda: h.msm(sc),
        }
        row = {}
        for name, fn in calls.items():
            for _ in range(warmup):
                fn()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            row[name] = {"call_ms_median": statistics.median(ts), "call_ms_min": min(ts), "call_ms_max": max(ts), "calls": warmup + reps}
        # same answers from both MSM entry points before any number is kept
        rec = d_out.to_host()
        want = lib.msm_g2(g2[0], g2[1], sc)
        assert np.array_equal(rec[:16], want[0]) and int(rec[16]) == want[1]
        h.free()
        for b in (d_xy, d_sc, d_out):
            b.free()
        out[str(n)] = row
    return out


def ratios(res, key):
    for n, row in res.items():
        r = {}
        for a, b in PAIRS:
            if key in row.get(a, {}) and key in row.get(b, {}) and row[b][key]:
                r[f"{a}/{b}"] = row[a][key] / row[b][key]
        if key in row.get("msm_g2", {}) and key in row.get("g2_scalar_mul_batch", {}):
            # n scalar multiplications at the batch kernel's per-element cost = one launch of the batch: the reference's msmG2 loop in our units
            r["n*scalar_mul_per_element/msm_g2"] = row["g2_scalar_mul_batch"][key] / row["msm_g2"][key]
        row["ratios_" + key] = r


def merge(res, prof_dir):
    """kernel_ms per call from DIR/n<size>/**/*kernel_stats.csv and the call counts the profiled run left in DIR/n<size>/calls.json"""
    for n, row in res.items():
        d = os.path.join(prof_dir, f"n{n}")
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats or not os.path.exists(os.path.join(d, "calls.json")):
            continue
        calls = json.load(open(os.path.join(d, "calls.json")))
        total = {}
        for f in stats:
            for r in csv.DictReader(open(f)):
                name = r["Name"].split("(")[0].replace("void ", "").replace("zg::", "").strip()  # points.hip's kernels are told apart by their group
                total[name] = total.get(name, 0.0) + float(r["TotalDurationNs"])
        for entry, kernels in KERNELS.items():
            if entry not in row:
                continue
            ns = sum(v for k, v in total.items() if any(k == p or (p.endswith("_") and k.startswith(p)) for p in kernels))
            n_calls = calls.get(entry, 0) + (calls.get("msm_g2_dev", 0) if entry == "msm_g2" else 0)
            n_calls += calls.get("_setup_" + entry, 0)
            if ns and n_calls:
                row[entry]["kernel_ms"] = ns / n_calls / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profiled", default=None, help="directory of the profiler run this process is part of: leaves calls.json there")
    ap.add_argument("--merge", default=None, help="directory with n<size>/ profiler outputs: adds kernel_ms to --out")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.merge:
        doc = json.load(open(a.out))
        merge(doc["sizes"], a.merge)
        ratios(doc["sizes"], "kernel_ms")
        json.dump(doc, open(a.out, "w"), indent=1)
        print(json.dumps({n: r.get("ratios_kernel_ms") for n, r in doc["sizes"].items()}))
        return
    res = run(sizes, a.reps, a.warmup)
    if a.profiled:
        os.makedirs(a.profiled, exist_ok=True)
        for n, row in res.items():
            calls = {k: v["calls"] for k, v in row.items()}
            calls["_setup_g2_fixed_base_mul_batch"], calls["_setup_g1_fixed_base_mul_batch"] = 2, 2
            calls["msm_g2"] += 1  # the cross-check call
            json.dump(calls, open(os.path.join(a.profiled, "calls.json"), "w"))
        return
    ratios(res, "call_ms_median")
    doc = {"what": "tools/bench_g2.py on one MI355X: host-pointer call times (ms; median, min, max of --reps synchronous calls after warm-up); kernel_ms, where "
                   "present, is kernel time per call from a separate rocprofv3 --kernel-trace --stats run of the same calls",
           "reps": a.reps, "warmup": a.warmup, "sizes": res}
    if a.out:
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({n: r["ratios_call_ms_median"] for n, r in res.items()}))


if __name__ == "__main__":
    main()
