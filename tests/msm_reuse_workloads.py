"""Workloads for the MSM workspace-reuse tests (tests/test_gpu_msm_workspace_reuse.py), their closed forms, and a CPU census of what each
one leaves in a workspace. Plain Python and numpy: nothing here needs a device.

Bases. A handle of N bases holds k_i * G with k_i = i + 1 for i < N/2 and k_i = -(i - N/2 + 1) for the rest: the first N/2 generator
multiples followed by the same points with y negated. Every MSM over them is (sum s_i k_i mod r) * G (oracle/pymodel.py:
msm_generator_multiples), whatever the scalars; a base flagged as the point at infinity counts with k_i = 0.

Workloads. Each is (name, off, n, scalars as canonical integers) over bases[off, off + n), for a window width c (W = ceil(255 / c)
windows). What each leaves in, or needs from, the workspace of the launch before it:

  U       uniform full-width scalars over the whole range: every array of the workspace fully populated
  Z       all zero: nothing is sorted, every bucket is empty, the result is the identity
  ONE     zero except scalar 1 at the last base: exactly one non-empty bucket holding one partial sum
  TOP     t << (c * (W - 1)) with t < 8 (and below r): only the top window is populated, a handful of long runs
  BITS    0 / 1, three ones in four: one bucket takes every entry, more than HUGE_PARTIALS of them from 4096 scalars on
  BYTE    below 256: at most 255 non-empty buckets of n / 256 entries each, the rest empty
  EQ      one full-width value repeated over all bases but the last: one long run per window
  NEG     r - small: the low windows are all ones, i.e. negative digits that carry into the next window
  CANCEL  s_i = s_{i + N/2}, uniform: a point and its negative meet in every bucket, so every bucket's total is the identity
  SUB     uniform over 37 bases near the end of the handle: far fewer entries than the workspace was sized for, and fewer chunks
  PREFIX  uniform over bases [0, 3000): served by the side table of a handle that has one

`extra` adds further ranges: (name, kind, off, n) with kind one of the names above, drawn over that range.
"""
import functools

import numpy as np

from oracle import pymodel as pm

HUGE_PARTIALS = 2048  # zolt_amd/csrc/msm.hip
KINDS = ("U", "Z", "ONE", "TOP", "BITS", "BYTE", "EQ", "NEG", "CANCEL", "SUB", "PREFIX")
SUB_POINTS = 37
PREFIX_POINTS = 3000


def base_multipliers(N, flags=None):
    """k_i of the N bases (an odd N has one more negative than positive); a flagged base counts with 0"""
    h = N // 2
    ks = [i + 1 for i in range(h)] + [-(i + 1) for i in range(N - h)]
    if flags is not None:
        ks = [0 if f else k for k, f in zip(ks, flags)]
    return ks


def bases(gm, N):
    """(N, 8) uint64 Montgomery coordinates of the bases from gm[i] = (i + 1) * G (at least N - N // 2 rows)"""
    h = N // 2
    neg = np.ascontiguousarray(gm[:N - h], dtype=np.uint64).copy()
    pos = neg[:h].copy()
    for i in range(N - h):  # -y in Montgomery form is p - y (y != 0 on this curve)
        neg[i, 4:] = pm.limbs(pm.P_MOD - pm.from_limbs(neg[i, 4:]))
    return np.concatenate([pos, neg])


def default_flags(N):
    """an infinity-flag vector that marks a few bases of both halves, the last but one and one inside SUB's range among them"""
    f = np.zeros(N, dtype=np.uint8)
    f[5::389] = 1
    f[N - 2] = 1
    f[_sub_off(N) + 3] = 1
    return f


def _sub_off(N):
    return N - SUB_POINTS - 3


def _uniform(rng, n):
    raw = rng.integers(0, 1 << 63, size=(n, 5), dtype=np.uint64)
    return [(int(a) | int(b) << 63 | int(c) << 126 | int(d) << 189 | int(e) << 252) % pm.R_MOD for a, b, c, d, e in raw]


def _draw(kind, rng, n, c):
    """n scalars of `kind` as canonical integers"""
    W = (255 + c - 1) // c
    if kind in ("U", "SUB", "PREFIX"):
        return _uniform(rng, n)
    if kind == "Z":
        return [0] * n
    if kind == "ONE":
        return [0] * (n - 1) + [1]
    if kind == "TOP":
        shift = c * (W - 1)
        return [int(t) << shift for t in rng.integers(0, min(8, pm.R_MOD >> shift), size=n)]
    if kind == "BITS":  # three ones in four: 4096 scalars already put more than HUGE_PARTIALS entries into the bucket of digit 1
        return [int(v != 0) for v in rng.integers(0, 4, size=n)]
    if kind == "BYTE":
        return [int(v) for v in rng.integers(0, 256, size=n)]
    if kind == "EQ":
        return _uniform(rng, 1) * n
    if kind == "NEG":
        return [pm.R_MOD - int(v) for v in rng.integers(1, 1 << 20, size=n)]
    assert kind == "CANCEL"
    s = _uniform(rng, n // 2)
    return s + s + [0] * (n - 2 * (n // 2))  # (an odd handle's last base has no partner)


@functools.lru_cache(maxsize=None)
def workloads(N, c, seed=2024, extra=()):
    """the eleven workloads of a handle of N bases with c-bit windows, then one per entry of `extra`: [(name, off, n, ints)]"""
    out = []
    for j, kind in enumerate(KINDS):
        rng = np.random.default_rng([seed, N, c, j])
        if kind == "SUB":
            off, n = _sub_off(N), SUB_POINTS
        elif kind == "PREFIX":
            off, n = 0, min(PREFIX_POINTS, N)
        elif kind == "EQ":
            off, n = 0, N - 1 - N % 2  # the k_i of an even handle sum to zero, and so would EQ's result: stop one base short of that
        else:
            off, n = 0, N
        out.append((kind, off, n, tuple(_draw(kind, rng, n, c))))
    for j, (name, kind, off, n) in enumerate(extra):
        assert kind != "CANCEL" and off + n <= N
        out.append((name, off, n, tuple(_draw(kind, np.random.default_rng([seed, N, c, 100 + j]), n, c))))
    return out


def vector(kind, n, c, seed):
    """one scalar vector of `kind` (not CANCEL) over bases [0, n), as a workload: the rows of a batch"""
    assert kind != "CANCEL"
    return (kind, 0, n, tuple(_draw(kind, np.random.default_rng([seed, n, c]), n, c)))


def closed_form(ks, workload):
    """the affine result (x, y) as canonical integers, or None for the identity"""
    _, off, n, ints = workload
    return pm.msm_generator_multiples(ks[off:off + n], ints)


def fr_mont(ints):
    """(n, 4) uint64 Montgomery limbs of canonical scalars"""
    return np.array([pm.limbs(v * pm.MONT_R % pm.R_MOD) for v in ints], dtype=np.uint64).reshape(-1, 4)


def result_record(point):
    """the nine words an MSM hands back for an affine point: Montgomery x, y and the infinity flag (identity: zeros, flag 1)"""
    rec = np.zeros(9, dtype=np.uint64)
    if point is None:
        rec[8] = 1
    else:
        rec[:4] = pm.limbs(pm.to_mont(point[0], pm.P_MOD))
        rec[4:8] = pm.limbs(pm.to_mont(point[1], pm.P_MOD))
    return rec


def signed_digits(s, c):
    """the W signed c-bit digits of a canonical scalar as msm_digits_kernel forms them: a window value above 2^(c-1) becomes
    value - 2^c and carries one into the next window"""
    W, NB, out, carry = (255 + c - 1) // c, 1 << (c - 1), [], 0
    for w in range(W):
        v = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if v > NB else 0
        out.append(v - (1 << c) if carry else v)
    return out


def census(workload, c, NT, G=1, heavy_over=8, flags=None):
    """What one launch over `workload` sorts and how its buckets are summed, as the kernels count it: bucket (w % G) * NB + |digit| - 1
    for every non-zero digit of window w; the sorted list of `total` entries is cut into chunks of C = ceil(total / NT) entries (chunk_len),
    and a bucket whose run is [s0, s1) receives (s1 - 1) / C - s0 / C + 1 partial sums. A bucket is empty, light (at most `heavy_over`
    partials: summed by the combine kernel; 8 * GS for the quad form, 8 for the lane form), heavy (up to HUGE_PARTIALS: a wave of
    msm_heavy_kernel) or huge (more: its block trees and arrival counters).

    -> {"NK", "total", "C", "runs": [(bucket, entries, partials)] for the non-empty buckets in sorted order,
        "empty" / "light" / "heavy" / "huge": bucket counts}
    For Z, ONE, BITS and BYTE below 2^(c-1) the digits are the scalars themselves; any other workload goes through signed_digits."""
    _, off, n, ints = workload
    NB = 1 << (c - 1)
    NK = G * NB
    hist = {}
    for i, s in enumerate(ints):
        if s == 0 or (flags is not None and flags[off + i]):
            continue
        for w, d in enumerate([s] if s <= NB else signed_digits(s, c)):
            if d:
                key = (w % G) * NB + abs(d) - 1
                hist[key] = hist.get(key, 0) + 1
    total = sum(hist.values())
    C = max(1, -(-total // NT))
    runs, s0 = [], 0
    out = {"NK": NK, "total": total, "C": C, "empty": NK - len(hist), "light": 0, "heavy": 0, "huge": 0}
    for key in sorted(hist):
        s1 = s0 + hist[key]
        partials = (s1 - 1) // C - s0 // C + 1
        runs.append((key, hist[key], partials))
        out["huge" if partials > HUGE_PARTIALS else "heavy" if partials > heavy_over else "light"] += 1
        s0 = s1
    out["runs"] = runs
    return out


def all_pairs_order(m):
    """A closed walk over 0 .. m-1 that takes every ordered pair (a, b), a == b included, exactly once as two consecutive items: an
    Eulerian circuit of the complete directed graph with loops (every vertex has m edges in and m out), m * m + 1 items long."""
    nxt = [0] * m  # the next unused successor of each vertex; successors are tried in the order v, v + 1, ... (mod m)
    stack, walk = [0], []
    while stack:  # Hierholzer
        v = stack[-1]
        if nxt[v] < m:
            stack.append((v + nxt[v]) % m)
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk


# The configurations of the reuse walk: bases, the zg_msm_config of the upload, the switches (set before the upload and kept for every
# launch: ZG_MSM_LANES is read at upload; ZG_MSM_LDS_SORT and ZG_MSM_LANE_TAIL by the planner, i.e. at upload and when a fused set or
# a slice is planned; ZG_MSM_TABLE_SPAN_* at upload, where they size the slice buffers, and at every launch), further ranges, and the
# plan the handle must get: sort 0 global atomics / 1 LDS / 2 two passes, tail 0 quad / 1 lane, G bucket groups.
# byte_heavy: BYTE's buckets are heavy. That needs 256 <= 2^(c-1) and more than `heavy_over` partials from n / 256 entries a bucket —
# out of reach at c = 8 and where the combine pass takes 16 quads a bucket (heavy from 129 partials: one-lane, six-lanes); TOP and EQ
# supply those configurations' heavy buckets. bits_huge: BITS's bucket is huge; no slice of the sliced handle has 2048 entries.
CONFIGS = {
    "one-lane": dict(N=1 << 13, cfg={}, env={"ZG_MSM_LANES": "1"}, extra=(), plan=dict(c=10, sort=1, tail=0, G=1), byte_heavy=False, bits_huge=True),
    "six-lanes": dict(N=1 << 13, cfg={}, env={}, extra=(), plan=dict(c=10, sort=1, tail=0, G=1), byte_heavy=False, bits_huge=True),
    # the side table's own workspace sees PREFIX and the two further prefixes: dense, skewed and empty in turn
    "two-pass": dict(N=40000, cfg={"window_bits": 16}, env={"ZG_MSM_LANES": "1"}, extra=(("PBITS", "BITS", 0, 3000), ("PZ", "Z", 0, 2999)),
                     plan=dict(c=16, sort=2, tail=0, G=1), byte_heavy=True, bits_huge=True),
    "atomic": dict(N=6000, cfg={}, env={"ZG_MSM_LANES": "1", "ZG_MSM_LDS_SORT": "0"}, extra=(), plan=dict(c=8, sort=0, tail=0, G=1),
                   byte_heavy=False, bits_huge=True),
    "lane-tail-13": dict(N=1 << 12, cfg={"window_bits": 13}, env={"ZG_MSM_LANES": "1", "ZG_MSM_LANE_TAIL": "1"}, extra=(),
                         plan=dict(c=13, sort=1, tail=1, G=1), byte_heavy=True, bits_huge=True),
    "lane-tail-15": dict(N=1 << 15, cfg={"window_bits": 15}, env={"ZG_MSM_LANES": "1", "ZG_MSM_LANE_TAIL": "1"}, extra=(),
                         plan=dict(c=15, sort=2, tail=1, G=1), byte_heavy=True, bits_huge=True),
    "tableless": dict(N=1 << 13, cfg={"expected_uses": 1}, env={}, extra=(), plan=dict(c=13, sort=2, tail=0, G=20), byte_heavy=True, bits_huge=True),
    # 5003 bases in slices of at least 700 points: the whole range takes 8 slices, PREFIX 5, R1400 2, R1399 and SUB 1
    "sliced": dict(N=5003, cfg={}, env={"ZG_MSM_LANES": "1", "ZG_MSM_TABLE_SPAN_MB": "1", "ZG_MSM_TABLE_SPAN_MIN_POINTS": "700"},
                   extra=(("R1400", "U", 100, 1400), ("R1399", "U", 200, 1399)), plan=dict(c=8, sort=1, tail=0, G=1), byte_heavy=False,
                   bits_huge=False, slices={"U": 8, "PREFIX": 5, "R1400": 2, "R1399": 1, "SUB": 1}),
}
# every switch a configuration may set: a test clears the others so that its handle gets the plan above whatever the suite runs under
SWITCHES = ("ZG_MSM_LANES", "ZG_MSM_LDS_SORT", "ZG_MSM_LANE_TAIL", "ZG_MSM_TABLE_SPAN_MB", "ZG_MSM_TABLE_SPAN_MIN_POINTS", "ZG_MSM_WINDOW_BITS",
            "ZG_MSM_PRECOMPUTE", "ZG_MSM_TWO_PASS_SORT", "ZG_MSM_CHUNK_THREADS", "ZG_MSM_SIDE_TABLE", "ZG_MSM_REDUCE_2D", "ZG_MSM_FINE_BITS",
            "ZG_MSM_FINE_BITS_MIN", "ZG_MSM_CHUNK_ENTRIES", "ZG_MSM_COMBINE_PER_QUAD")
