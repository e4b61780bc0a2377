"""Every host-pointer entry point that stages through csrc/common.hip.h's Staging, called from four host threads at once under
ZG_POOL_DEBUG=1: each result against oracle.binding, and no pool block written after it was freed. The shapes are the smallest that reach
each branch of the wrappers (empty inputs, one element, the single-slab / partials split of the column sums, the no-round sumcheck, one
and several MSM vectors). Entry points without a zolt_amd.lib wrapper are not called here. One child process: the debug mode is read from
the environment once."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, sys, threading
import numpy as np
sys.path.insert(0, %r)
import torch
from zolt_amd import lib
from oracle import binding as ob
lib.init(0)
P = ob._R_P
N_BASES = 300
gm = ob.g1_gen_multiples(N_BASES)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, (int, bool)):
        return a == b
    return np.array_equal(np.asarray(a), np.asarray(b))


def cases(seed, h):
    # (name, the call through zolt_amd.lib, the oracle's answer) for one thread, which uploads h["bases"] (300 points) and h["srs"] (64)
    rng = np.random.default_rng(seed)
    fr = lambda *shape: ob.f_to_mont(ob.FR, rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64))
    out = []
    add = lambda name, call, want: out.append((name, call, want))
    for v in (0, 1, 9):
        r = fr(v)
        add("eq_table v=%%d" %% v, lambda r=r: lib.fr_eq_table(r), ob.fr_eq_table(r))
        add("eq_plus_one_table v=%%d" %% v, lambda r=r: lib.fr_eq_plus_one_table(r), ob.eq_plus_one_table(r))
        add("lt_table v=%%d" %% v, lambda r=r: lib.fr_lt_table(r), ob.lt_table(r))
        add("eq_prefix_tables v=%%d" %% v, lambda r=r: lib.fr_eq_prefix_tables(r), ob.fr_eq_prefix_tables(r))
    for n in (2, 1024):
        t, r = fr(n), fr(1)[0]
        add("bind_low len=%%d" %% n, lambda t=t, r=r: lib.fr_bind_low(t, r), ob.fr_bind_low(t, r))
        add("bind_high len=%%d" %% n, lambda t=t, r=r: lib.fr_bind_high(t, r), ob.fr_bind_high(t, r))
    for v in (0, 9):
        e, p = fr(1 << v), fr(v)
        add("dense_evaluate v=%%d" %% v, lambda e=e, p=p: lib.fr_dense_evaluate(e, p), ob.fr_dense_evaluate(e, p))
    r6 = fr(6)
    eq6 = ob.fr_eq_table(r6)
    for n_rows in (0, 40, 64):
        w = fr(max(n_rows, 1), 3)[:n_rows]
        want = np.stack([ob.fr_sum_halves(np.concatenate([ob.f_mul(ob.FR, eq6[:n_rows], w[:, i]), np.zeros((128 - n_rows, 4), dtype=np.uint64)]))[0]
                         for i in range(3)])
        add("rows_mle n_rows=%%d" %% n_rows, lambda w=w: lib.fr_rows_mle(w, r6), want)
    # rows_affine: two tables of two interleaved maps over ten rows of five columns, padded to sixteen
    k, ntab, g, n_rows, n_pad = 5, 2, 2, 10, 16
    rows = fr(n_rows, k)
    coeff_int = [[int(rng.integers(0, 1 << 62)) ** 4 %% P if rng.random() < 0.6 else 0 for _ in range(k + 1)] for _ in range(ntab * g)]
    coeff_int[0] = [0] * (k + 1)
    coeffs = np.stack([np.stack([ob.fr_from_int(x) for x in row]) for row in coeff_int])
    want = [np.zeros((n_pad * g, 4), dtype=np.uint64) for _ in range(ntab)]
    for c in range(ntab * g):
        acc = np.repeat(coeffs[c, k].reshape(1, 4), n_rows, axis=0)
        for col in range(k):
            if coeff_int[c][col]:
                acc = ob._fadd(acc, ob._fmul(rows[:, col], coeffs[c, col]))
        want[c // g][c %% g:n_rows * g:g] = acc
    add("rows_affine", lambda: lib.fr_rows_affine(rows, coeffs, ntab, g, n_pad), want)
    # rows_affine_prodsum: three pairs of maps over twenty rows of six columns, weight interleave two
    k2, n2, npairs, g2 = 6, 20, 3, 2
    rows_int = [[int(x) for x in rng.integers(0, 1 << 62, size=k2)] for _ in range(n2)]
    ps_int = [[int(rng.integers(0, 1 << 62)) ** 4 %% P if rng.random() < 0.7 else 0 for _ in range(k2 + 1)] for _ in range(2 * npairs)]
    w_int = [int.from_bytes(rng.bytes(32), "little") %% P for _ in range(n2 * g2)]
    mont = lambda vals: np.stack([ob.fr_from_int(x) for x in vals])
    ps_rows, ps_w, ps_coeffs = mont([x for r in rows_int for x in r]), mont(w_int), mont([x for r in ps_int for x in r])
    want = []
    for p in range(npairs):
        a, b = ps_int[2 * p], ps_int[2 * p + 1]
        tot = 0
        for i in range(n2):
            av = a[k2] + sum(a[c] * rows_int[i][c] for c in range(k2))
            bv = b[k2] + sum(b[c] * rows_int[i][c] for c in range(k2))
            tot += w_int[i * g2 + p %% g2] * av * bv
        want.append(ob.fr_from_int(tot))

    def prodsum():
        d_rows, d_w = lib.DeviceBuffer.from_host(ps_rows), lib.DeviceBuffer.from_host(ps_w)
        got = lib.fr_rows_affine_prodsum_dev(d_rows.ptr, n2, k2, ps_coeffs, npairs, d_w.ptr, g2)
        d_rows.free()
        d_w.free()
        return got
    add("rows_affine_prodsum", prodsum, np.stack(want))
    for rws in (1, 37):
        for m in (1, 4):
            t, w = fr(rws * 300), fr(m, rws)
            add("weighted_colsum rows=%%d m=%%d" %% (rws, m), lambda t=t, w=w, rws=rws: lib.fr_weighted_colsum(t, rws, 300, w), ob.weighted_colsum(t, rws, 300, w))
    for n in (1, 777):
        q = [fr(n) for _ in range(4)]
        add("spartan_combine n=%%d" %% n, lambda q=q: lib.fr_spartan_combine(*q), ob.fr_spartan_combine(*q))
    for n in (1, 300):
        a, s = fr(n), fr(1)[0]
        add("fr_scale n=%%d" %% n, lambda a=a, s=s: lib.fr_scale(a, s), ob.fr_poly_scale(a, s))
    for n in (1, 1024):
        e = fr(n)
        wc, wr, wch, wfin, wok = ob.run_sumcheck(e)

        def sumcheck(e=e):
            res = lib.run_sumcheck(e)
            return [res["claim"], res["rounds"], res["final_point"], res["final_eval"], res["result"]]
        add("run_sumcheck len=%%d" %% n, sumcheck, [wc, wr, wch, wfin, wok == 1])
    for n in (0, 100):
        vals, idx = fr(n), rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64)
        add("bit_split_sums n=%%d" %% n, lambda vals=vals, idx=idx: lib.fr_bit_split_sums(vals, idx, 3), ob.lasso_address_sums(vals, idx, 3))
    srs_xy, no_inf = gm[:64], np.zeros(64, dtype=np.uint8)
    for v in (0, 6):
        e, p, val = fr(1 << v), fr(v), fr(1)[0]
        add("hyperkzg_open v=%%d" %% v, lambda e=e, p=p, val=val: lib.hyperkzg_open(h["srs"], e, p, val), ob.hyperkzg_open(srs_xy, no_inf, e, p, val))
    polys, p = [fr(64), fr(32)], fr(6)
    add("hyperkzg_batch_open k=2", lambda: lib.hyperkzg_batch_open(h["srs"], polys, p), ob.hyperkzg_batch_open(srs_xy, no_inf, polys, p))
    for k in (1, 3):
        for n in (0, 300):
            b = [fr(n) for _ in range(k)]
            add("msm_g1_batch k=%%d n=%%d" %% (k, n), lambda b=b, n=n: h["bases"].msm_batch(b, n=n), ob.msm_g1_batch(gm, None, b))
    for n in (0, 300):
        words = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        add("msm_g1_u64 n=%%d" %% n, lambda words=words, n=n: h["bases"].msm_u64(words, n=n), ob.msm_g1(gm[:n], None, ob.f_from_u64(ob.FR, words)))
    a, b = fr(5), fr(5)
    add("field_op sqr", lambda: lib.field_op(lib.FR, lib.OP_SQR, a), ob.f_sqr(ob.FR, a))
    add("field_op mul", lambda: lib.field_op(lib.FR, lib.OP_MUL, a, b), ob.f_mul(ob.FR, a, b))
    return out


handles = [{} for _ in range(4)]
todo = [cases(100 + i, handles[i]) for i in range(4)]  # inputs and the oracle's answers, once, before the threads start
bad = [[] for _ in range(4)]
ran = [0] * 4


def work(i):
    # the bases are uploaded and freed around everything else: the handles' blocks come from the same pool
    handles[i]["bases"], handles[i]["srs"] = lib.Bases.upload(gm), lib.Bases.upload(gm[:64])
    for name, call, want in todo[i]:
        if not same(call(), want):
            bad[i].append(name)
        ran[i] += 1
    handles[i]["bases"].free()
    handles[i]["srs"].free()


ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
[t.start() for t in ts]
[t.join() for t in ts]
print(json.dumps({"bad": bad, "ran": ran, "stats": lib.pool_debug_stats()}))
"""


def test_every_staged_entry_point_from_four_threads_matches_the_oracle_and_frees_only_idle_blocks():
    env = dict(os.environ)
    env.pop("ZG_DEV_ALLOC_CACHE_MB", None)  # (0 = the pool keeps nothing: there is no reuse to check)
    env["ZG_POOL_DEBUG"] = "1"
    res = subprocess.run([sys.executable, "-c", SCRIPT % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1500:])
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["bad"] == [[], [], [], []], out["bad"]
    assert out["ran"] == [46] * 4, out["ran"]
    st = out["stats"]
    assert st["mode"] == 1 and st["hits"] == 0 and st["blocks_verified"] > 0, st
