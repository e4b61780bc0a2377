#!/usr/bin/env python3
"""The Dory verifier setup (DoryVerifierSetup.fromSRS's 3 * 2^K - 2 pairings, src/zkvm/preprocessing.zig:889-973) on one GPU (needs one),
three ways, at n_g1 = n_g2 = 2^K:

  key        zg_dory_verifier_setup over a resident key (the key's creation is not in the figure: it serves the commitments)
  points     zg_dory_verifier_setup_points from host generators
  composed   the same values from the parent commit's entry points: the host slices the generators into the explicit pair list of all
             3K + 1 products and makes ONE zg_multi_pairing call over it — the strongest composition the per-call ABI offers. Its chi
             values still lack their running product: `composed_with_chi` adds the K Fp12 products, one zg_field_op call each.

All routes give the same words (checked before any number is kept). Times are a host clock around calls that end in a device synchronise:
`--warmup` calls, then `--reps` timed ones, in one process; median, min and max.

    python tools/bench_dory_vsetup.py --out profiles/dory_vsetup_bench.json
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


def fr_random(rng, n):
    from zolt_amd import lib
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    raw[:, 3] >>= np.uint64(2)  # below the modulus
    return lib.field_op(lib.FR, lib.OP_TO_MONT, raw)


def make_generators(K, seed):
    from zolt_amd import api, lib
    rng = np.random.default_rng(seed)
    g1 = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, 1 << K))
    g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), fr_random(rng, 1 << K))
    return (np.ascontiguousarray(g1[0]).reshape(-1, 8), np.asarray(g1[1], dtype=np.uint8)), (np.ascontiguousarray(g2[0]).reshape(-1, 16), np.asarray(g2[1], dtype=np.uint8))


def composed(g1, g2, K, with_chi):
    """the explicit pair list — diagonal levels, then g1[h..2h) x g2[0..h), then g1[0..h) x g2[h..2h) per level — and one multi-pairing"""
    from zolt_amd import lib
    N = 1 << K
    i1, i2, seg = [np.arange(N)], [np.arange(N)], [0, 1] + [2 << k for k in range(K)]
    for fam in (0, 1):
        for k in range(1, K + 1):
            h = 1 << (k - 1)
            i1.append(np.arange(h, 2 * h) if fam == 0 else np.arange(h))
            i2.append(np.arange(h) if fam == 0 else np.arange(h, 2 * h))
            seg.append(seg[-1] + h)
    i1, i2 = np.concatenate(i1), np.concatenate(i2)
    gt = lib.multi_pairing(g1[0][i1], g1[1][i1], g2[0][i2], g2[1][i2], np.array(seg, dtype=np.uint64))
    chi, d1r, d2r = gt[:K + 1].copy(), gt[K:2 * K + 1].copy(), gt[2 * K:3 * K + 1].copy()
    d1r[0] = d2r[0] = ONE
    if with_chi:
        for k in range(1, K + 1):
            chi[k] = lib.field_op(lib.FP, lib.OP_FP12_MUL, chi[k - 1].reshape(12, 4), chi[k].reshape(12, 4)).reshape(48)
    return chi, d1r, d2r


ONE = None


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "calls": warmup + reps}


def run(Ks, reps, warmup, each=None):
    global ONE
    from zolt_amd import api, lib
    lib.init()
    ONE = api.gtOne()
    out = {}
    for K in Ks:
        g1, g2 = make_generators(K, seed=200 + K)
        key = lib.DoryKey.create(g1, g2)
        want = lib.dory_verifier_setup(key)
        for got in (lib.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1]), composed(g1, g2, K, True)):
            assert all(np.array_equal(a, b) for a, b in zip(want, got)), K  # the routes agree before any number is kept
        row = {"pairs": 3 * (1 << K) - 2, "products": 3 * K + 1,
               "key": timed(lambda: lib.dory_verifier_setup(key), reps, warmup),
               "points": timed(lambda: lib.dory_verifier_setup_points(g1[0], g1[1], g2[0], g2[1]), reps, warmup),
               "composed": timed(lambda: composed(g1, g2, K, False), reps, warmup),
               "composed_with_chi": timed(lambda: composed(g1, g2, K, True), reps, warmup)}
        key.free()
        for name in ("points", "composed", "composed_with_chi"):
            row[name + "/key"] = row[name]["ms_median"] / row["key"]["ms_median"]
        out[str(K)] = row
        if each:
            each(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="4,6,8,10")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def each(res):
        doc = {"what": "tools/bench_dory_vsetup.py on one MI355X: every chi and delta of a Dory key with n_g1 = n_g2 = 2^K; ms of a host clock "
                       "around synchronous calls: median, min, max of --reps calls after --warmup; composed = the parent commit's "
                       "zg_multi_pairing over the explicitly sliced pair list, 3K + 1 segments in one call (its chi values without their "
                       "running product; composed_with_chi adds K zg_field_op Fp12 products)", "reps": a.reps, "warmup": a.warmup, "K": res}
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        k, r = list(res.items())[-1]
        print(f"K {k}: key {r['key']['ms_median']:.2f} ms, points {r['points']['ms_median']:.2f} ms, composed {r['composed']['ms_median']:.2f} ms, "
              f"composed_with_chi {r['composed_with_chi']['ms_median']:.2f} ms", file=sys.stderr, flush=True)

    res = run([int(s) for s in a.ks.split(",")], a.reps, a.warmup, each)
    print(json.dumps({k: {n: r[n]["ms_median"] for n in ("key", "points", "composed", "composed_with_chi")} for k, r in res.items()}))


if __name__ == "__main__":
    main()
