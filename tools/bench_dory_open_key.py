#!/usr/bin/env python3
"""The opening the prover calls (DoryCommitmentScheme.open's device side, begin to final) on one GPU (needs one), three ways:

  (i)   begin_stepwise      zg_dory_open_begin + the stepwise calls: the generators uploaded and an MSM handle built at begin, two host
                            synchronisations a round. Runs only where nu = sigma (that begin takes 2^sigma generators a side).
  (ii)  key_stepwise        zg_dory_open_key_begin + the stepwise calls: the generators and the handle are the resident key's. The same
                            kernels as (iii) under today's synchronisation pattern: the baseline of (iii).
  (iii) key_run             zg_dory_open_key_begin + zg_dory_open_run: every round enqueued back to back, one synchronisation.

at (nu, sigma) = (6, 6), (7, 8), (10, 10), (11, 12), under the pairing engine of the environment (ZG_PAIRING_ENGINE). The challenges are
fixed pseudo-random scalars. All routes of a size produce the same message records, compared byte for byte before any number is kept.
Times are a host clock around calls that end in a device synchronise: `--warmup` whole openings, then `--reps` timed ones, and the
whole thing `--sittings` times over so that the run-to-run spread shows; per sitting median, min and max, and the split of an opening
into begin and the rest. The key is made once per size and is in no figure.

    python tools/bench_dory_open_key.py --out profiles/dory_open_key_bench.json
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

from tools.bench_dory_open import fr_random  # noqa: E402

SIZES = [(6, 6), (7, 8), (10, 10), (11, 12)]


def make_inputs(nu, sigma, seed):
    from zolt_amd import api, lib
    rng = np.random.default_rng(seed)
    n, n_left = 1 << sigma, 1 << nu
    g1 = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, n))
    g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), fr_random(rng, n_left))
    rows = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, n_left))
    ch = fr_random(rng, 2 * sigma + 1)
    words = np.stack([ch, lib.field_op(lib.FR, lib.OP_INV, ch)], axis=1).reshape(-1, 4)  # c, c_inv, ...
    return {"g1_vec": g1, "g2_vec": g2, "rows": rows, "v_vec": fr_random(rng, n), "right_vec": fr_random(rng, n), "left_vec": fr_random(rng, n_left),
            "nu": nu, "sigma": sigma, "words": np.ascontiguousarray(words)}


def _begin(inp, key):
    from zolt_amd import lib
    if key is None:
        return lib.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"])
    return lib.DoryOpenSession.begin_key(key, inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"])


def open_once(inp, key, run):
    """-> (records as one array, ms of begin, ms of the rounds and the final message)"""
    w, sigma = inp["words"], inp["sigma"]
    t0 = time.perf_counter()
    ses = _begin(inp, key)
    t1 = time.perf_counter()
    if run:
        first, second, final = ses.run(w)
    else:
        first, second = [], []
        for t in range(sigma):
            first.append(ses.first_message())
            second.append(ses.second_message(w[4 * t], w[4 * t + 1]))
            ses.fold(w[4 * t + 2], w[4 * t + 3])
        final = ses.final(w[4 * sigma], w[4 * sigma + 1])
    t2 = time.perf_counter()
    ses.close()
    rec = np.concatenate([ses.vmv] + [np.asarray(m).reshape(-1) for m in first] + [np.asarray(m).reshape(-1) for m in second] + [final])
    return rec, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sittings", type=int, default=3)
    ap.add_argument("--sizes", default=None, help="e.g. 6,6;7,8")
    args = ap.parse_args()
    from zolt_amd import lib
    lib.init()
    sizes = SIZES if not args.sizes else [tuple(int(x) for x in s.split(",")) for s in args.sizes.split(";")]
    result = {"tool": "tools/bench_dory_open_key.py", "pairing_engine": lib.pairing_engine_get(), "warmup": args.warmup, "reps": args.reps,
              "sittings": args.sittings, "sizes": []}
    for nu, sigma in sizes:
        inp = make_inputs(nu, sigma, seed=1000 * nu + sigma)
        key = lib.DoryKey.create(inp["g1_vec"], inp["g2_vec"])
        routes = {"key_stepwise": (key, False), "key_run": (key, True)}
        if nu == sigma:
            routes = {"begin_stepwise": (None, False), **routes}
        ref = None
        for name, (k, run) in routes.items():  # the same bytes, before any number is kept
            rec = open_once(inp, k, run)[0]
            if ref is None:
                ref = rec
            if not np.array_equal(rec, ref):
                raise SystemExit(f"(nu, sigma) = ({nu}, {sigma}): {name} differs from {next(iter(routes))}")
        entry = {"nu": nu, "sigma": sigma, "host_synchronisations": {"begin_stepwise": 2 * sigma + 2, "key_stepwise": 2 * sigma + 2, "key_run": 2},
                 "records_equal": True, "routes": {name: [] for name in routes}}
        for _ in range(args.sittings):
            for name, (k, run) in routes.items():
                for _ in range(args.warmup):
                    open_once(inp, k, run)
                runs = [open_once(inp, k, run)[1:] for _ in range(args.reps)]
                entry["routes"][name].append({"whole": stats([b + r for b, r in runs]), "begin": stats([b for b, _ in runs]), "rounds_and_final": stats([r for _, r in runs])})
        med = {name: [s["whole"]["median_ms"] for s in entry["routes"][name]] for name in routes}
        entry["whole_median_ms_per_sitting"] = med
        entry["run_over_key_stepwise"] = round(statistics.median(med["key_run"]) / statistics.median(med["key_stepwise"]), 4)
        # faster beyond the spread: the slowest sitting of (iii) under the fastest sitting of (ii)
        entry["run_faster_beyond_spread"] = max(med["key_run"]) < min(med["key_stepwise"])
        if nu == sigma:
            entry["key_stepwise_over_begin_stepwise"] = round(statistics.median(med["key_stepwise"]) / statistics.median(med["begin_stepwise"]), 4)
        key.free()
        result["sizes"].append(entry)
        print(json.dumps({k: entry[k] for k in entry if k != "routes"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
