#!/usr/bin/env python3
"""The pairing entry points on one GPU (needs one). Writes profiles/pairing_bench.json.

Host-pointer call time: a host clock around the synchronous call (it ends in a stream synchronise inside the library) — `--warmup` calls,
then `--reps` timed ones: median and the min / max spread.

    python tools/bench_pairing.py --out profiles/pairing_bench.json

Measured: zg_miller_loop_batch, zg_pairing_batch and zg_multi_pairing (k = 1) at every n of --sizes; a reduce-and-fold round's six
products (six segments of 2^9 pairs) as ONE zg_multi_pairing call and as six calls; zg_final_exponentiation_batch of one element (the
one-lane tail of every multi-pairing, for its share); and zg_g2_scalar_mul_batch at n = 2^10 in the same process as the yardstick: a
Miller loop is about as many Fp products in one lane as a G2 scalar multiplication."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fr_random(rng, n):
    from zolt_amd import lib
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] >>= np.uint64(2)  # below the modulus
    return lib.field_op(lib.FR, lib.OP_TO_MONT, raw)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"call_ms_median": statistics.median(ts), "call_ms_min": min(ts), "call_ms_max": max(ts), "calls": warmup + reps}


def run(sizes, reps, warmup):
    from zolt_amd import api, lib
    lib.init()
    rng = np.random.default_rng(11)
    top = max(sizes + [6 * 512])
    g1 = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, top))
    g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), fr_random(rng, top))
    out = {"sizes": {}}
    for n in sizes:
        a, ai, b, bi = g1[0][:n], g1[1][:n], g2[0][:n], g2[1][:n]
        row = {
            "miller_loop_batch": timed(lambda: lib.miller_loop_batch(a, ai, b, bi), reps, warmup),
            "pairing_batch": timed(lambda: lib.pairing_batch(a, ai, b, bi), reps, warmup),
            "multi_pairing_k1": timed(lambda: lib.multi_pairing(a, ai, b, bi), reps, warmup),
        }
        # the entry points agree before any number is kept
        assert np.array_equal(lib.pairing_batch(a[:2], ai[:2], b[:2], bi[:2]), lib.final_exponentiation_batch(lib.miller_loop_batch(a[:2], ai[:2], b[:2], bi[:2])))
        out["sizes"][str(n)] = row
    # one round's six products: six segments of 2^9 pairs
    n6 = 6 * 512
    a, ai, b, bi = g1[0][:n6], g1[1][:n6], g2[0][:n6], g2[1][:n6]
    seg = [512 * j for j in range(7)]
    one = lib.multi_pairing(a, ai, b, bi, seg)
    six = np.stack([lib.multi_pairing(a[512 * j:512 * j + 512], ai[512 * j:512 * j + 512], b[512 * j:512 * j + 512], bi[512 * j:512 * j + 512])[0]
                    for j in range(6)])
    assert np.array_equal(one, six)
    out["round_six_products"] = {
        "one_call_k6": timed(lambda: lib.multi_pairing(a, ai, b, bi, seg), reps, warmup),
        "six_calls_k1": timed(lambda: [lib.multi_pairing(a[512 * j:512 * j + 512], ai[512 * j:512 * j + 512], b[512 * j:512 * j + 512],
                                                         bi[512 * j:512 * j + 512]) for j in range(6)], reps, warmup),
    }
    m1 = lib.miller_loop_batch(g1[0][:1], None, g2[0][:1], None)
    out["final_exponentiation_n1"] = timed(lambda: lib.final_exponentiation_batch(m1), reps, warmup)
    sc = fr_random(rng, 1024)
    out["yardstick_g2_scalar_mul_batch_1024"] = timed(lambda: lib.g2_scalar_mul_batch(g2[0][:1024], g2[1][:1024], sc), reps, warmup)
    return out


def ratios(res):
    y = res["yardstick_g2_scalar_mul_batch_1024"]["call_ms_median"]
    fe = res["final_exponentiation_n1"]["call_ms_median"]
    r = {"six_calls/one_call": res["round_six_products"]["six_calls_k1"]["call_ms_median"] / res["round_six_products"]["one_call_k6"]["call_ms_median"]}
    for n, row in res["sizes"].items():
        r[f"miller_loop_batch[{n}]/g2_scalar_mul_batch[1024]"] = row["miller_loop_batch"]["call_ms_median"] / y
        r[f"final_exponentiation_n1/multi_pairing_k1[{n}]"] = fe / row["multi_pairing_k1"]["call_ms_median"]
    res["ratios_call_ms_median"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run([int(s) for s in a.sizes.split(",")], a.reps, a.warmup)
    ratios(res)
    doc = {"what": "tools/bench_pairing.py on one MI355X: host-pointer call times (ms; median, min, max of --reps synchronous calls after --warmup)",
           "reps": a.reps, "warmup": a.warmup}
    doc.update(res)
    if a.out:
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(res["ratios_call_ms_median"]))


if __name__ == "__main__":
    main()
