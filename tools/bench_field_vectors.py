#!/usr/bin/env python3
"""The section "field vectors (device)" (include/zolt_gpu.h) timed, for Fr and Fp, in one process on the same inputs. Every figure is wall
time of the whole call, after warm-up, repeated: median, minimum and maximum in milliseconds. A _dev figure includes a zg_sync() where the
call itself is asynchronous.

  batch_inverse_host   zg_field_batch_inverse (host pointers)  vs  zg_field_op(ZG_OP_INV) — the entry point and kernel as they were
                       before this section, one Fermat exponentiation per element — on the same input; outputs compared byte for byte
  batch_inverse_dev    zg_field_batch_inverse_dev  vs  zg_field_op_dev(ZG_OP_INV) on resident data; outputs compared byte for byte
  inner_product_dev, horner_dev, dense_evaluate_dev (Fr)   resident data, with the bytes they read per second; compared with the host forms

"faster" in the summary means faster by more than the max - min spread of either figure.

    python tools/bench_field_vectors.py --out profiles/field_vectors_bench.json [--sizes 16,20,22] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zolt_amd import lib  # noqa: E402

NAMES = {lib.FR: "fr", lib.FP: "fp"}


def timed(fn, reps, warmup=1):
    out = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            out.append(dt)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def compare(old, new):
    """ratio of the medians, and whether `new` is faster by more than the spread of either figure"""
    spread = max(old["max_ms"] - old["min_ms"], new["max_ms"] - new["min_ms"])
    return {"ratio_old_over_new": old["median_ms"] / new["median_ms"], "spread_ms": spread,
            "faster_beyond_spread": bool(old["median_ms"] - new["median_ms"] > spread)}


def elements(field, n, seed):
    """n canonical Montgomery elements, a zero every 1000th"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a = lib.field_op(field, lib.OP_TO_MONT, raw)
    a[::1000] = 0
    return a


def with_rate(t, nbytes):
    t["GB_per_s"] = nbytes / (t["median_ms"] * 1e-3) / 1e9
    return t


def bench(field, log_n, reps):
    n = 1 << log_n
    a, b = elements(field, n, 7 + field), elements(field, n, 11 + field)
    res = {}
    keep = {}
    # both host-pointer forms write into an output that exists and has been touched: a fresh 32 MB array per call is pinned page by page
    # by the HIP runtime, now and then for tens of milliseconds, and that would be the figure
    out_old, out_new = np.zeros_like(a), np.zeros_like(a)
    p_a, p_old, p_new = a.ctypes.data, out_old.ctypes.data, out_new.ctypes.data

    def op_inv_host():
        assert lib._lib.zg_field_op(field, lib.OP_INV, p_a, None, p_old, n) == 0, lib.last_error()

    def batch_inv_host():
        assert lib._lib.zg_field_batch_inverse(field, p_a, p_new, n) == 0, lib.last_error()

    old, new = timed(op_inv_host, reps, warmup=2), timed(batch_inv_host, reps, warmup=2)
    assert out_old.tobytes() == out_new.tobytes(), "zg_field_batch_inverse and ZG_OP_INV disagree"
    keep["old"] = out_old
    res["batch_inverse_host"] = {"field_op_inv": old, "batch_inverse": new, **compare(old, new)}

    d_a, d_b = lib.DeviceBuffer.from_host(a), lib.DeviceBuffer.from_host(b)
    d_o, d_n = lib.DeviceBuffer(n * 32), lib.DeviceBuffer(n * 32)

    def op_inv_dev():
        lib.field_op_dev(field, lib.OP_INV, d_a.ptr, 0, d_o.ptr, n)
        lib.sync()

    def batch_inv_dev():
        lib.field_batch_inverse_dev(field, d_a.ptr, d_n.ptr, n)
        lib.sync()

    old, new = timed(op_inv_dev, reps), with_rate(timed(batch_inv_dev, reps), 64 * n)
    assert d_o.to_host().tobytes() == d_n.to_host().tobytes() == keep["old"].tobytes(), "the device forms disagree"
    res["batch_inverse_dev"] = {"field_op_dev_inv": old, "batch_inverse_dev": new, **compare(old, new)}

    res["inner_product_dev"] = with_rate(timed(lambda: keep.__setitem__("ip", lib.field_inner_product_dev(field, d_a.ptr, d_b.ptr, n)), reps), 64 * n)
    assert keep["ip"].tobytes() == lib.field_inner_product(field, a, b).tobytes(), "inner product: host and device forms disagree"
    x = b[1]
    res["horner_dev"] = with_rate(timed(lambda: keep.__setitem__("h", lib.field_horner_dev(field, d_a.ptr, n, x)), reps), 32 * n)
    assert keep["h"].tobytes() == lib.field_horner(field, a, x).tobytes(), "Horner: host and device forms disagree"
    if field == lib.FR:
        point = b[2:2 + log_n]
        res["dense_evaluate_dev"] = with_rate(timed(lambda: keep.__setitem__("e", lib.fr_dense_evaluate_dev(d_a.ptr, point)), reps), 96 * n)
        assert keep["e"].tobytes() == lib.fr_dense_evaluate(a, point).tobytes(), "dense evaluation: host and device forms disagree"
    for buf in (d_a, d_b, d_o, d_n):
        buf.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    lib.init(0)
    out = {"tool": "tools/bench_field_vectors.py", "version": lib.version(), "elements_per_lane": lib.FV_E, "tile": lib.FV_TILE,
           "timing": "wall time of the whole call (a zg_sync() included where the call is asynchronous), 1 warm-up (2 for the host-pointer forms, into "
                     "outputs that exist), median / min / max of reps",
           "bytes": "batch inverse: 64 per element (read and write); inner product: 64; Horner: 32; dense evaluation: 96 (the eq table written, then both read)"}
    for field in (lib.FR, lib.FP):
        out[NAMES[field]] = {}
        for s in [int(v) for v in args.sizes.split(",") if v]:
            out[NAMES[field]][f"2^{s}"] = bench(field, s, args.reps)
            print(NAMES[field], s, json.dumps(out[NAMES[field]][f"2^{s}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
