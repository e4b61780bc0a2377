#!/usr/bin/env python3
"""Key files to usable handles: "Points from bytes" (zg_*_from_bytes) against the composition the mirrors had before, in one process on the
same bytes. Every figure is wall time of the whole call (bytes in host memory to a handle or to points in host memory), after warm-up,
repeated: median, minimum and maximum in milliseconds.

  g1_be_load     n BE records of a raw SRS: wire.srs_from_raw  vs  wire.srs_g1_from_raw followed by Bases.upload; the handles are compared
                 by one MSM
  dory_srs       the Jolt Dory SRS at max_num_vars: Dory.loadFromFile  vs  the records converted through zg_field_op(TO_MONT) followed by
                 DoryKey.create; the keys are compared by one commitment
  decompress     n compressed records a group through g1 / g2_points_from_bytes (no earlier path exists on the device: the figure stands alone)

    python tools/bench_point_bytes.py --out profiles/point_bytes_bench.json [--sizes 16,20,22] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zolt_amd import api, lib  # noqa: E402

P = api.P_MOD
HALF = [((P - 1) // 2 >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]


def timed(fn, reps, warmup=1, after=None):
    out = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if after:
            after(r)
        if k >= warmup:
            out.append(dt)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def above_half(canon):
    """canon (n, 4) canonical limbs -> bool (n,): the value is > (p - 1) / 2, i.e. not "positive\""""
    gt = np.zeros(canon.shape[0], dtype=bool)
    eq = np.ones(canon.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        gt |= eq & (canon[:, i] > np.uint64(HALF[i]))
        eq &= canon[:, i] == np.uint64(HALF[i])
    return gt


def g1_points(n):
    tau = api.fr_from_int(0x1234567 + n)
    b, xy, inf = lib.Bases.hyperkzg_setup(api.generator(), tau, n, expected_uses=1)
    b.free()
    return xy, inf


def compress(canon_x, canon_y_sign, words):
    rec = np.ascontiguousarray(canon_x).view(np.uint8).reshape(-1, 8 * words).copy()
    rec[:, -1] |= np.where(canon_y_sign, 0x80, 0).astype(np.uint8)
    return rec.tobytes()


def bench_g1_load(log_n, reps):
    n = 1 << log_n
    xy, inf = g1_points(n)
    raw = api.srs_g1_to_raw(xy, inf)
    sc = np.ascontiguousarray(xy[:, :4] & np.uint64((1 << 60) - 1))  # any scalars below r
    res = {}

    def old():
        pxy, pinf, _ = api.srs_g1_from_raw(raw)
        return lib.Bases.upload(pxy, pinf)

    def new():
        return api.srs_from_raw(raw)["bases"]

    for name, fn in (("today", old), ("from_bytes", new)):
        res[name] = timed(fn, reps, after=lambda h: (res.setdefault(name + "_msm", [int(w) for w in h.msm(sc)[0]]), h.free()))
    assert res.pop("today_msm") == res.pop("from_bytes_msm"), "the two handles disagree"
    res["ratio_today_over_from_bytes"] = res["today"]["median_ms"] / res["from_bytes"]["median_ms"]
    return res


def bench_dory_srs(max_num_vars, reps):
    params = api.Dory.setup(max_num_vars)
    g1, g2 = params.g1_vec, params.g2_vec
    le = lambda xy: lib.field_op(lib.FP, lib.OP_FROM_MONT, np.ascontiguousarray(xy).reshape(-1, 4)).tobytes()  # noqa: E731
    blob = (b"JOLT_DORY_SRS_V1" + max_num_vars.to_bytes(8, "little") + g1[0].shape[0].to_bytes(8, "little") + le(g1[0]) + g2[0].shape[0].to_bytes(8, "little")
            + le(g2[0]) + bytes(192))
    params.deinit()
    evals = np.ascontiguousarray(g1[0][:, :4] & np.uint64((1 << 60) - 1))[:1 << min(max_num_vars, 8)]
    res = {}

    def old():
        _, b1, b2, _, _ = api.Dory.parseSrsContainer(blob)
        pts = []
        for b, words in ((b1, 8), (b2, 16)):
            raw = np.frombuffer(b, dtype=np.uint64).reshape(-1, 4).copy()
            raw[words // 4 - 1::words // 4, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
            pts.append((lib.field_op(lib.FP, lib.OP_TO_MONT, raw).reshape(-1, words), None))
        return lib.DoryKey.create(*pts)

    def new():
        return api.Dory.loadFromFile(blob)

    for name, fn in (("today", old), ("from_bytes", new)):
        res[name] = timed(fn, reps, after=lambda k: (res.setdefault(name + "_gt", [int(w) for w in lib.dory_commit_batch(k, [(lib.DORY_POLY_FR, evals, None, 0, 0)])[0]]),
                                                     k.free()))
    assert res.pop("today_gt") == res.pop("from_bytes_gt"), "the two keys disagree"
    res["ratio_today_over_from_bytes"] = res["today"]["median_ms"] / res["from_bytes"]["median_ms"]
    return res


def bench_decompress(log_n, reps):
    n = 1 << log_n
    xy, _ = g1_points(n)
    canon = lib.field_op(lib.FP, lib.OP_FROM_MONT, xy.reshape(-1, 4)).reshape(n, 2, 4)
    rec1 = compress(canon[:, 0], above_half(canon[:, 1]), 4)
    sc = np.ascontiguousarray(xy[:, :4] & np.uint64((1 << 60) - 1))
    g2xy, _ = lib.g2_fixed_base_mul_batch(api.g2_generator(), sc)
    c2 = lib.field_op(lib.FP, lib.OP_FROM_MONT, g2xy.reshape(-1, 4)).reshape(n, 4, 4)
    c1_zero = ~c2[:, 3].any(axis=1)
    rec2 = compress(c2[:, :2].reshape(n, 8), np.where(c1_zero, above_half(c2[:, 2]), above_half(c2[:, 3])), 8)
    res = {"g1": timed(lambda: lib.g1_points_from_bytes(rec1, lib.POINT_BYTES_ARK_COMPRESSED), reps),
           "g2": timed(lambda: lib.g2_points_from_bytes(rec2, lib.POINT_BYTES_ARK_COMPRESSED), reps)}
    assert np.array_equal(lib.g1_points_from_bytes(rec1, lib.POINT_BYTES_ARK_COMPRESSED)[0], xy), "G1 decompression does not return the points"
    assert np.array_equal(lib.g2_points_from_bytes(rec2, lib.POINT_BYTES_ARK_COMPRESSED)[0], g2xy), "G2 decompression does not return the points"
    for g in ("g1", "g2"):
        res[g]["us_per_point"] = res[g]["median_ms"] * 1e3 / n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--dory", default="16,20")
    ap.add_argument("--decompress", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lib.init(0)
    out = {"tool": "tools/bench_point_bytes.py", "version": lib.version(), "timing": "wall time of the whole call, 1 warm-up, median / min / max of reps",
           "g1_be_load": {}, "dory_srs": {}, "decompress": {}}
    for s in [int(v) for v in args.sizes.split(",") if v]:
        out["g1_be_load"][f"2^{s}"] = bench_g1_load(s, args.reps)
        print("g1_be_load", s, json.dumps(out["g1_be_load"][f"2^{s}"]), flush=True)
    for s in [int(v) for v in args.dory.split(",") if v]:
        out["dory_srs"][f"max_num_vars={s}"] = bench_dory_srs(s, args.reps)
        print("dory_srs", s, json.dumps(out["dory_srs"][f"max_num_vars={s}"]), flush=True)
    for s in [int(v) for v in args.decompress.split(",") if v]:
        out["decompress"][f"2^{s}"] = bench_decompress(s, args.reps)
        print("decompress", s, json.dumps(out["decompress"][f"2^{s}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
