"""The short-vector bucket MSM (zolt_amd/csrc/small_msm.hip.h) on its own, over G1 and over G2: zg_selftest_small_msm issues the header's
launch set — digits, a workgroup per window with a lane per bucket, the per-bit tree sums, Horner — exactly as g2.hip and dory.hip do, with
jobs of different lengths in one set, which no caller uses yet. The Fp instantiation is otherwise reached only by a Dory opening session on
random inputs.

The model is the closed form: every base is k_i G (or its negative, or a repeat), so the result is (sum s_i k_i mod r) G, one scalar
multiplication of tests/xyzz_model.py per job; the directed bucket patterns are also run through the reference's loop (a scalarMul and an
add per base: tests/g2_model.py msm, and the same loop over G1). Every comparison is word for word, the identity record included.

    python -m pytest tests/test_gpu_small_msm.py -m gpu -q --durations=0"""
import random

import numpy as np
import pytest

from tests import g2_model as M
from tests import xyzz_model as xm

pytestmark = pytest.mark.gpu
R = xm.R
GROUPS = pytest.mark.parametrize("gid", [xm.G1, xm.G2], ids=["g1", "g2"])
POOL_N = 1000


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


class Pool:
    """k G for |k| <= POOL_N, as points and as the ABI's words; built once per group and never changed"""
    _made = {}

    def __new__(cls, gid):
        if gid not in cls._made:
            self = super().__new__(cls)
            grp = self.grp = xm.GROUPS[gid]
            self.pt = [None]
            for _ in range(POOL_N):
                self.pt.append(grp.add(self.pt[-1], grp.G))
            assert self.pt[POOL_N] == grp.mul(grp.G, POOL_N)
            self.words = np.zeros((2 * POOL_N + 1, 2 * grp.W), dtype=np.uint64)  # row k for k G, row -k (from the end) for -k G
            for k in range(1, POOL_N + 1):
                self.words[k] = grp.affine_words(self.pt[k])
                self.words[-k] = grp.affine_words(grp.neg(self.pt[k]))
            cls._made[gid] = self
        return cls._made[gid]

    def point(self, k):
        return self.pt[k] if k >= 0 else self.grp.neg(self.pt[-k])


def job(gid, entries, zero_flagged=True):
    """entries: [(k, s, flagged)] — base k G (k != 0, |k| <= POOL_N), canonical scalar s, identity flag. -> the arrays of one job and the
    expected record. A flagged base keeps its coordinates unless zero_flagged (on input only the flag counts)"""
    pool = Pool(gid)
    ks = np.array([e[0] for e in entries], dtype=np.int64)
    xy = pool.words[ks] if len(entries) else np.zeros((0, 2 * pool.grp.W), dtype=np.uint64)
    inf = np.array([1 if e[2] else 0 for e in entries], dtype=np.uint8)
    if zero_flagged:
        xy = xy.copy()
        xy[inf == 1] = 0
    total = sum(e[0] * e[1] for e in entries if not e[2]) % R
    want = pool.grp.mul(pool.grp.G, total)
    return (xy, inf if inf.any() else None, M.fr_pack([e[1] for e in entries])), (pool.grp.affine_words(want), 1 if want is None else 0)


def run(zl, gid, jobs):
    """one launch set -> [words + flag] per job"""
    return [list(int(x) for x in xy) + [flag] for xy, flag in zl.selftest_small_msm(gid, [j[0] for j in jobs])]


def expect(jobs):
    return [list(words) + [flag] for _, (words, flag) in jobs]


def loop_reference(gid, entries):
    """the reference's loop: res = res + [s] P over the bases in order"""
    pool, res = Pool(gid), None
    for k, s, flagged in entries:
        p = None if flagged else pool.point(k)
        res = M.add(res, M.scalar_mul(p, s)) if gid == xm.G2 else pool.grp.add(res, pool.grp.mul(p, s))
    return pool.grp.affine_words(res), 1 if res is None else 0


def uniform(rng, n):
    return [(rng.choice((-1, 1)) * rng.randrange(1, POOL_N + 1), rng.randrange(R), False) for _ in range(n)]


@GROUPS
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257, 1000])
def test_lengths(zl, gid, n):
    """around the padding of the digit rows to a multiple of four and around the 256-lane workgroup of the digits kernel"""
    j = job(gid, uniform(random.Random(100 + n), n))
    assert run(zl, gid, [j]) == expect([j])


BYTES_ALL = sum(1 << (8 * w) for w in range(32))


def _scalar_families(rng, n):
    ks = [rng.choice((-1, 1)) * rng.randrange(1, POOL_N + 1) for _ in range(n)]
    fam = {
        "every-byte-equal": [b * BYTES_ALL for b in (rng.randrange(1, 0x30) for _ in range(n))],  # one bucket in all 32 windows; < r: r's top byte is 0x30
        "digits-1-and-255": [sum((rng.choice((1, 255)) if w < 31 else 1) << (8 * w) for w in range(32)) for _ in range(n)],
        "r-minus-1": [R - 1] * n,
        "all-zero": [0] * n,
    }
    for w in (0, 15, 31):
        fam[f"one-byte-window-{w}"] = [rng.randrange(1, 0x30 if w == 31 else 256) << (8 * w) for _ in range(n)]
    out = {name: [(k, s, False) for k, s in zip(ks, ss)] for name, ss in fam.items()}
    # a cancelling vector: every term once more with the opposite base, or with the opposite scalar
    half = uniform(rng, n // 2)
    out["cancelling"] = half + [(-k, s, False) if i % 2 else (k, (R - s) % R, False) for i, (k, s, _) in enumerate(half)]
    rng.shuffle(out["cancelling"])
    return out


FAMILIES = ["every-byte-equal", "digits-1-and-255", "r-minus-1", "all-zero", "one-byte-window-0", "one-byte-window-15", "one-byte-window-31", "cancelling"]


@GROUPS
@pytest.mark.parametrize("family", FAMILIES)
def test_scalar_families(zl, gid, family):
    entries = _scalar_families(random.Random(7), 67)[family]
    j = job(gid, entries)
    if family in ("all-zero", "cancelling"):
        assert j[1] == (Pool(gid).grp.affine_words(None), 1)  # the identity record, as the group's reference writes it
    assert run(zl, gid, [j]) == expect([j])


def _directed(w):
    """bucket patterns built from digits of window w; P = 7 G. Buckets 1 and 3 share bit 0, so the bit-0 tree of smsm_bitsum_kernel adds
    them to each other at its last level. A lone base sits in its bucket as from_affine (zz == 1); two equal bases are a doubling there
    (zz == 4 y^2); a third window keeps most results off the identity"""
    sh, other = 8 * w, 8 * ((w + 5) % 31)
    d = lambda digit: digit << sh  # noqa: E731
    keep = (11, 9 << other, False)
    return {
        "same-sum-same-representative": [(7, d(1), False), (7, d(3), False), keep],
        "same-sum-different-representatives": [(14, d(1), False), (7, d(3), False), (7, d(3), False), keep],
        "opposite-sums-same-representative": [(7, d(1), False), (-7, d(3), False), keep],
        "opposite-sums-different-representatives": [(-14, d(1), False), (7, d(3), False), (7, d(3), False), keep],
        "opposite-sums-alone": [(-14, d(1), False), (7, d(3), False), (7, d(3), False)],  # S_0 cancels, S_1 = 2 P: the window is 4 P
        "window-sums-to-identity": [(7, d(2), False), (-14, d(1), False), keep],  # T_w = 2 S_1 + S_0 = 2 P - 2 P in smsm_final_kernel
        "window-sums-to-identity-in-a-bucket": [(7, d(5), False), (-7, d(5), False), keep],
        "everything-cancels": [(7, d(2), False), (-14, d(1), False)],
        "every-base-flagged": [(k, d(k), True) for k in range(1, 17)],
        "every-fifth-base-flagged": [(k, d(k) + (k << other), k % 5 == 0) for k in range(1, 17)],
    }


@GROUPS
@pytest.mark.parametrize("w", [0, 15, 31])
def test_directed_bucket_patterns(zl, gid, w):
    """the exceptional branches of xyzz_madd and xyzz_add inside the bucket, bit-sum and final kernels, in the lowest window, a middle one
    and the top one; against the closed form and against the reference's loop (n <= 16)"""
    cases = _directed(w)
    for name, entries in cases.items():
        assert len(entries) <= 16
        j = job(gid, entries)
        assert j[1] == loop_reference(gid, entries), name
        assert run(zl, gid, [j]) == expect([j]), name
        if name.startswith("every-fifth"):  # on input only the flag counts: the coordinates under a flag may be anything
            kept = job(gid, entries, zero_flagged=False)
            assert kept[1] == j[1] and run(zl, gid, [kept]) == expect([j]), name
    for name in ("everything-cancels", "every-base-flagged"):
        assert job(gid, cases[name])[1][1] == 1, name


@GROUPS
@pytest.mark.parametrize("lengths", [(5, 0, 257, 4), (1000, 1, 1, 3), (3, 256), (255, 0, 1), (0, 0), (4, 4, 4, 4)], ids=str)
def test_launch_sets_of_unequal_jobs(zl, gid, lengths):
    """2, 3 and 4 jobs of different lengths in one launch set, one scratch sized for the longest: every job is the model's, and word for
    word the same job run alone"""
    rng = random.Random(sum(lengths) + len(lengths))
    jobs = [job(gid, uniform(rng, n)) for n in lengths]
    together = run(zl, gid, jobs)
    assert together == expect(jobs)
    for j, got in zip(jobs, together):
        assert run(zl, gid, [j]) == [got]


def test_bad_arguments_are_error_codes(zl):
    import ctypes as C
    for gid in (xm.G1, xm.G2):
        (xy, _, sc), _ = job(gid, uniform(random.Random(1), 4))
        out = np.zeros(4 * 17, dtype=np.uint64)

        def call(group, n_jobs, n, with_n=True, with_xy=True, with_sc=True, with_out=True, null_xy0=False):
            ns = (C.c_size_t * 4)(*([n] * 4))
            xs = (C.c_void_p * 4)(*([None if null_xy0 else xy.ctypes.data] + [xy.ctypes.data] * 3))
            ss = (C.c_void_p * 4)(*([sc.ctypes.data] * 4))
            return zl._lib.zg_selftest_small_msm(group, n_jobs, ns if with_n else None, xs if with_xy else None, None, ss if with_sc else None,
                                                 out.ctypes.data if with_out else None)

        assert call(gid, 1, 4) == 0
        for bad in (dict(group=-1), dict(group=2), dict(n_jobs=0), dict(n_jobs=5), dict(n_jobs=-1), dict(n=(1 << 16) + 1), dict(with_n=False),
                    dict(with_xy=False), dict(with_sc=False), dict(with_out=False), dict(null_xy0=True)):
            args = dict(group=gid, n_jobs=1, n=4)
            args.update(bad)
            assert call(**args) == zl.ERR_INVALID, bad
