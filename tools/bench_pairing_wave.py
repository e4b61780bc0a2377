#!/usr/bin/env python3
"""The two pairing engines (include/zolt_gpu.h, "Pairings (engine)") on the same inputs, in one process on one MI355X (needs one):
LANE, a lane per Miller loop and per final exponentiation, and WAVE, a wavefront per each. Conventions of tools/bench_pairing.py:
host-pointer calls that end in a device synchronise, `--warmup` calls, then the median, min and max of `--reps` timed ones.

Rows: zg_final_exponentiation_batch of 1 and 6 elements; zg_miller_loop_batch and zg_multi_pairing (k = 1) at n = 1, 2^6, 2^10, 2^12,
2^16; a round's six products of 2^9 pairs as one call; one Dory opening at sigma = nu = 6 and 8 through the session with fixed
challenges (tools/bench_dory_open.py), with its per-round split; verifier setup at K = 6; the reference's commitment list at T = 2^14.

Every row's outputs are compared byte for byte between the engines; the tool exits non-zero on a mismatch. A row PASSES where WAVE's
max is below LANE's min; the row at n = 2^16 has no bar and only reports which engine wins.

    python tools/bench_pairing_wave.py --out profiles/pairing_wave_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ZG_DORY_COMMIT_TIMES"] = "0"  # tools/bench_dory_commit.py turns the stage clock on when imported: not for these figures

NO_BAR = 1 << 16


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "calls": warmup + reps}


def flat(x):
    """every array of a result, in order, as one list"""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return [np.asarray(x)]


def both(lib, fn, reps, warmup, bar=True):
    """fn under each engine: its outputs compared, then timed -> the row"""
    outs, row = {}, {}
    for name, eng in (("lane", lib.PAIRING_ENGINE_LANE), ("wave", lib.PAIRING_ENGINE_WAVE)):
        with lib.pairing_engine(eng):
            outs[name] = flat(fn())
            row[name] = timed(fn, reps, warmup)
    row["same_bytes"] = len(outs["lane"]) == len(outs["wave"]) and all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(outs["lane"], outs["wave"]))
    row["lane/wave"] = row["lane"]["ms_median"] / row["wave"]["ms_median"]
    row["bar"] = bar
    row["wave_max_below_lane_min"] = row["wave"]["ms_max"] < row["lane"]["ms_min"]
    return row


def run(reps, warmup, each=None):
    from tools import bench_dory_commit, bench_dory_open, bench_dory_vsetup, bench_pairing
    from zolt_amd import api, lib
    lib.init()
    rng = np.random.default_rng(11)
    sizes = [1, 1 << 6, 1 << 10, 1 << 12, 1 << 16]
    top = max(sizes)
    g1 = lib.g1_fixed_base_mul_batch(api.generator(), bench_pairing.fr_random(rng, top))
    g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), bench_pairing.fr_random(rng, top))
    rows = {}

    def keep(name, row):
        rows[name] = row
        if each:
            each(rows)

    with lib.pairing_engine(lib.PAIRING_ENGINE_LANE):
        m6 = lib.miller_loop_batch(g1[0][:6], None, g2[0][:6], None)
    for n in (1, 6):
        keep(f"final_exponentiation_batch[{n}]", both(lib, lambda: lib.final_exponentiation_batch(m6[:n]), reps, warmup))
    for n in sizes:
        a, ai, b, bi = g1[0][:n], g1[1][:n], g2[0][:n], g2[1][:n]
        keep(f"miller_loop_batch[{n}]", both(lib, lambda: lib.miller_loop_batch(a, ai, b, bi), reps, warmup, bar=n < NO_BAR))
        keep(f"multi_pairing_k1[{n}]", both(lib, lambda: lib.multi_pairing(a, ai, b, bi), reps, warmup, bar=n < NO_BAR))
    n6 = 6 * 512
    a, ai, b, bi = g1[0][:n6], g1[1][:n6], g2[0][:n6], g2[1][:n6]
    seg = [512 * j for j in range(7)]
    keep("round_six_products_of_512", both(lib, lambda: lib.multi_pairing(a, ai, b, bi, seg), reps, warmup))
    for sigma in (6, 8):
        inp = bench_dory_open.make_inputs(sigma, sigma, seed=7000 + sigma)
        row = both(lib, lambda: bench_dory_open.session_open(inp), reps, warmup)
        for name, eng in (("lane", lib.PAIRING_ENGINE_LANE), ("wave", lib.PAIRING_ENGINE_WAVE)):  # one further opening, every step waited for
            with lib.pairing_engine(eng):
                sp = bench_dory_open.Splits()
                bench_dory_open.session_open(inp, sp)
                row[name]["per_round_ms"] = {k: v / sigma for k, v in sp.ms.items() if k not in ("begin", "final_and_close")}
        keep(f"dory_opening[sigma=nu={sigma}]", row)
    K = 6
    vg1, vg2 = bench_dory_vsetup.make_generators(K, seed=40 + K)
    keep(f"dory_verifier_setup_points[K={K}]", both(lib, lambda: lib.dory_verifier_setup_points(vg1[0], vg1[1], vg2[0], vg2[1]), reps, warmup))
    T = 1 << 14
    log_t = T.bit_length() - 1
    params = api.Dory.setup(log_t + 1)
    key = api.Dory.key(params)
    cols = bench_dory_commit.columns(T, True, seed=1000 + log_t)
    keep(f"dory_commit_trace_columns[T={T}]", both(lib, lambda: api.Dory.commitTraceColumns(key, *cols), reps, warmup))
    key.free()
    params.deinit()
    return rows


def verdict(rows):
    bad = [k for k, r in rows.items() if not r["same_bytes"]]
    missed = [k for k, r in rows.items() if r["bar"] and not r["wave_max_below_lane_min"]]
    return bad, missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {"what": "tools/bench_pairing_wave.py on one MI355X: host-pointer call times (ms; median, min, max of --reps synchronous calls after "
                   "--warmup) of the lane and the wave pairing engine on the same inputs, outputs compared byte for byte",
           "reps": a.reps, "warmup": a.warmup}

    def each(rows):
        doc["rows"] = rows
        if a.out:
            json.dump(doc, open(a.out, "w"), indent=1)

    rows = run(a.reps, a.warmup, each)
    bad, missed = verdict(rows)
    doc.update({"rows": rows, "mismatched_rows": bad, "rows_that_miss_the_bar": missed})
    if a.out:
        json.dump(doc, open(a.out, "w"), indent=1)
    for k, r in rows.items():
        print(f"{k:42s} lane {r['lane']['ms_median']:9.3f} ({r['lane']['ms_min']:.3f}-{r['lane']['ms_max']:.3f})  wave {r['wave']['ms_median']:9.3f} "
              f"({r['wave']['ms_min']:.3f}-{r['wave']['ms_max']:.3f})  x{r['lane/wave']:.2f} {'' if r['bar'] else '(no bar) '}"
              f"{'ok' if r['wave_max_below_lane_min'] else 'MISS' if r['bar'] else ''}{'' if r['same_bytes'] else '  MISMATCH'}")
    print(json.dumps({"mismatched_rows": bad, "rows_that_miss_the_bar": missed}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
