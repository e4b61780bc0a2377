#!/usr/bin/env python3
"""One whole Dory opening (openWithTranscript's device side, begin to final) on one GPU (needs one), two ways:

  session    the resident reduce-and-fold session (zg_dory_open_*: lib.DoryOpenSession)
  per_call   the same proof composed from the per-call entry points — api.Dory.multiPairBatch, msmG2, applyFirstChallenge, foldVectors,
             initV2 and Bases.upload(expected_uses=1).msm — which upload and download the vectors around every step

The transcript is replaced by fixed pseudo-random challenges, so the host hash is in neither figure. Both routes produce the same message
records (checked before any number is kept). Times are a host clock around calls that end in a device synchronise: `--warmup` whole
openings, then `--reps` timed ones; median, min and max. A further pass per size splits a round into first message, update + second
message, and fold (the session's fold is asynchronous: the split pass waits for it, the whole-opening figure does not).

    python tools/bench_dory_open.py --out profiles/dory_open_bench.json
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


def make_inputs(nu, sigma, seed, n_rows=None):
    """generators, row commitments and scalar vectors of an opening, made on the device from a seed; challenges[r] = (beta, beta_inv,
    alpha, alpha_inv), then (gamma, gamma_inv)"""
    from zolt_amd import api, lib
    rng = np.random.default_rng(seed)
    n, n_left = 1 << sigma, 1 << nu
    n_rows = n_left if n_rows is None else n_rows
    g1 = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, n))
    g2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), fr_random(rng, n))
    rows = lib.g1_fixed_base_mul_batch(api.generator(), fr_random(rng, n_rows))
    ch = fr_random(rng, 2 * sigma + 1)
    ch_inv = lib.field_op(lib.FR, lib.OP_INV, ch)
    return {"g1_vec": g1, "g2_vec": g2, "rows": rows, "v_vec": fr_random(rng, n), "right_vec": fr_random(rng, n), "left_vec": fr_random(rng, n_left),
            "nu": nu, "sigma": sigma, "challenges": [(ch[2 * r], ch_inv[2 * r], ch[2 * r + 1], ch_inv[2 * r + 1]) for r in range(sigma)],
            "gamma": (ch[2 * sigma], ch_inv[2 * sigma])}


class Splits:
    """host-clock time per step kind, summed over the rounds of one opening"""

    def __init__(self):
        self.ms = {}

    def add(self, key, t0):
        self.ms[key] = self.ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3


def session_open(inp, splits=None):
    """-> (vmv, firsts, seconds, final) message records. With `splits` every fold is waited for, so its time is its own."""
    from zolt_amd import lib
    t0 = time.perf_counter()
    ses = lib.DoryOpenSession.begin(inp["g1_vec"], inp["g2_vec"], inp["rows"], inp["v_vec"], inp["right_vec"], inp["left_vec"], inp["nu"], inp["sigma"])
    if splits:
        splits.add("begin", t0)
    firsts, seconds = [], []
    for beta, beta_inv, alpha, alpha_inv in inp["challenges"]:
        t0 = time.perf_counter()
        firsts.append(ses.first_message())
        if splits:
            splits.add("first_message", t0)
        t0 = time.perf_counter()
        seconds.append(ses.second_message(beta, beta_inv))
        if splits:
            splits.add("update_and_second_message", t0)
        t0 = time.perf_counter()
        ses.fold(alpha, alpha_inv)
        if splits:
            ses.wait()
            splits.add("fold", t0)
    t0 = time.perf_counter()
    final = ses.final(*inp["gamma"])
    vmv = ses.vmv
    ses.close()
    if splits:
        splits.add("final_and_close", t0)
    return vmv, firsts, seconds, final


def _g1_rec(p):
    out = np.zeros(9, dtype=np.uint64)
    if p[1]:
        out[8] = 1
    else:
        out[:8] = p[0]
    return out


def _g2_rec(p):
    return np.concatenate([np.asarray(p[0], dtype=np.uint64).reshape(16), np.array([int(p[1])], dtype=np.uint64)])


def _g1_msm(xy, inf, sc):
    """MSM.compute over a temporary: a handle per call, as a host without resident vectors has to"""
    from zolt_amd import lib
    h = lib.Bases.upload(xy, inf, expected_uses=1)
    try:
        return h.msm(sc)
    finally:
        h.free()


def per_call_open(inp, splits=None):
    """the same opening from the per-call entry points -> the same four results"""
    from zolt_amd import api, lib
    D = api.Dory
    nu, sigma = inp["nu"], inp["sigma"]
    n, n_left = 1 << sigma, 1 << nu
    g1 = (np.asarray(inp["g1_vec"][0])[:n], np.asarray(inp["g1_vec"][1])[:n])
    g2 = (np.asarray(inp["g2_vec"][0])[:n], np.asarray(inp["g2_vec"][1])[:n])
    t0 = time.perf_counter()
    k = min(np.asarray(inp["rows"][0]).shape[0], n)
    v1 = (np.zeros((n, 8), dtype=np.uint64), np.ones(n, dtype=np.uint8))
    v1[0][:k], v1[1][:k] = np.asarray(inp["rows"][0])[:k], np.asarray(inp["rows"][1])[:k]
    v_vec = np.asarray(inp["v_vec"]).reshape(-1, 4)
    nv = v_vec.shape[0]
    t_v = _g1_msm(v1[0][:nv], v1[1][:nv], v_vec)
    gamma1_v = _g1_msm(g1[0][:nv], g1[1][:nv], v_vec)
    g2_0 = (g2[0][:1], g2[1][:1])
    one = lambda p: (np.asarray(p[0]).reshape(1, 8), np.array([p[1]], dtype=np.uint8))  # noqa: E731
    c_d2 = D.multiPairBatch([(one(t_v), g2_0), (one(gamma1_v), g2_0)])
    e1 = _g1_msm(v1[0][:n_left], v1[1][:n_left], inp["left_vec"])
    vmv = np.concatenate([c_d2.reshape(-1), _g1_rec(e1)])
    v2 = D.initV2(g2[0][0], v_vec, n) if not g2[1][0] else (np.tile(api.g2_identity(), (n, 1)), np.ones(n, dtype=np.uint8))
    s1 = np.asarray(inp["right_vec"]).reshape(-1, 4).copy()
    s2 = np.zeros((n, 4), dtype=np.uint64)
    s2[:n_left] = inp["left_vec"]
    if splits:
        splits.add("begin", t0)
    firsts, seconds = [], []
    cur = n
    for beta, beta_inv, alpha, alpha_inv in inp["challenges"]:
        n2 = cur // 2
        sl = lambda v, a, b: (v[0][a:b], v[1][a:b])  # noqa: E731
        t0 = time.perf_counter()
        d = D.multiPairBatch([(sl(v1, 0, n2), sl(g2, 0, n2)), (sl(v1, n2, cur), sl(g2, 0, n2)), (sl(g1, 0, n2), sl(v2, 0, n2)), (sl(g1, 0, n2), sl(v2, n2, cur))])
        e1_beta = _g1_msm(g1[0][:cur], g1[1][:cur], s2[:cur])
        e2_beta = D.msmG2(sl(g2, 0, cur), s1[:cur])
        firsts.append(np.concatenate([d.reshape(-1), _g1_rec(e1_beta), _g2_rec(e2_beta)]))
        if splits:
            splits.add("first_message", t0)
        t0 = time.perf_counter()
        v1, v2 = D.applyFirstChallenge(sl(v1, 0, cur), sl(v2, 0, cur), g1, g2, beta, beta_inv)
        cc = D.multiPairBatch([(sl(v1, 0, n2), sl(v2, n2, cur)), (sl(v1, n2, cur), sl(v2, 0, n2))])
        e1_plus = _g1_msm(v1[0][:n2], v1[1][:n2], s2[n2:cur])
        e1_minus = _g1_msm(v1[0][n2:cur], v1[1][n2:cur], s2[:n2])
        e2_plus = D.msmG2(sl(v2, n2, cur), s1[:n2])
        e2_minus = D.msmG2(sl(v2, 0, n2), s1[n2:cur])
        seconds.append(np.concatenate([cc.reshape(-1), _g1_rec(e1_plus), _g1_rec(e1_minus), _g2_rec(e2_plus), _g2_rec(e2_minus)]))
        if splits:
            splits.add("update_and_second_message", t0)
        t0 = time.perf_counter()
        v1, v2, s1, s2 = D.foldVectors(sl(v1, 0, cur), sl(v2, 0, cur), s1[:cur], s2[:cur], alpha, alpha_inv)
        if splits:
            splits.add("fold", t0)
        cur = n2
    t0 = time.perf_counter()
    gamma, gamma_inv = inp["gamma"]
    gs1 = lib.field_op(lib.FR, lib.OP_MUL, np.asarray(gamma).reshape(1, 4), s1[:1])
    gs2 = lib.field_op(lib.FR, lib.OP_MUL, np.asarray(gamma_inv).reshape(1, 4), s2[:1])
    h1 = lib.g1_fixed_base_mul_batch(api.generator(), gs1)
    f1 = lib.g1_affine_add_batch(v1[0][:1], v1[1][:1], h1[0], h1[1])
    h2 = lib.g2_fixed_base_mul_batch(api.g2_generator(), gs2)
    f2 = lib.g2_affine_add_batch(v2[0][:1], v2[1][:1], h2[0], h2[1])
    final = np.concatenate([_g1_rec((f1[0][0], int(f1[1][0]))), _g2_rec((f2[0][0], int(f2[1][0])))])
    if splits:
        splits.add("final_and_close", t0)
    return vmv, firsts, seconds, final


def same_messages(a, b):
    return (np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
            and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3]))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "openings": warmup + reps}


def run(sigmas, reps, warmup, each=None):
    """-> {sigma: row}; `each(rows so far)` after every size, so a long run leaves what it has measured"""
    from zolt_amd import lib
    lib.init()
    out = {}
    for sigma in sigmas:
        inp = make_inputs(sigma, sigma, seed=100 + sigma)
        assert same_messages(session_open(inp), per_call_open(inp)), sigma  # the two routes agree before any number is kept
        row = {"session": timed(lambda: session_open(inp), reps, warmup), "per_call": timed(lambda: per_call_open(inp), reps, warmup)}
        row["per_call/session"] = row["per_call"]["ms_median"] / row["session"]["ms_median"]
        for name, fn in (("session", session_open), ("per_call", per_call_open)):
            sp = Splits()
            fn(inp, sp)
            row[name]["split_ms_one_opening"] = sp.ms
            row[name]["split_ms_per_round"] = {k: sp.ms[k] / sigma for k in ("first_message", "update_and_second_message", "fold")}
        out[str(sigma)] = row
        if each:
            each(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigmas", default="6,8,10,12")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    def each(res):
        doc = {"what": "tools/bench_dory_open.py on one MI355X: one whole Dory opening at sigma = nu, fixed challenges (no transcript); ms of a "
                       "host clock around synchronous calls: median, min, max of --reps openings after --warmup; per_call = the parent "
                       "commit's entry points", "reps": a.reps, "warmup": a.warmup, "sigma": res}
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        s, r = list(res.items())[-1]
        print(f"sigma {s}: session {r['session']['ms_median']:.2f} ms, per_call {r['per_call']['ms_median']:.2f} ms", file=sys.stderr, flush=True)

    res = run([int(s) for s in a.sigmas.split(",")], a.reps, a.warmup, each)
    print(json.dumps({s: {"session_ms": r["session"]["ms_median"], "per_call_ms": r["per_call"]["ms_median"], "per_call/session": r["per_call/session"]}
                      for s, r in res.items()}))


if __name__ == "__main__":
    main()
