"""Run by tests/test_gpu_launch_shapes.py, one fresh process per switch set (the switches are read once per process): the launch
shapes the prover gets at 2^21 entries and above — workgroup template, rows per workgroup, grid cap, grid-stride trips — forced at
the smallest sizes that still have them, every result bit for bit against the oracle.

    python tests/launch_shapes_check.py SET        (SET: a key of SETS; the parent puts SETS[SET]["env"] into the environment)

Every case first asks the library which shape it would launch (zg_selftest_launch_shape, the functions the launches call) and
compares it with the shape written down here; a switch that was renamed, clamped or cached differently fails there instead of
silently running the default shape. The shapes below are derived from zolt_amd/csrc/{poly,psc,rrw}.hip:

  eq table   rows = 2^(v - 8) rows of 256 entries (expanding kernel: 2^(v - 11) rows of 2048); rows per workgroup =
             min(ceil(rows / min(rows, ZG_EQ_BLOCKS)), 256); template <4> needs 4 rows per workgroup, <2> needs 2. A thread group
             walks its rows two per trip and a remainder row, so an odd count per group runs both.
  Spartan    the same with ZG_SC_SPARTAN_BLOCKS / ZG_SC_SPARTAN_WG.
  fold/sums  workgroups = min(ceil(pairs / threads), ZG_SC_MAX_BLOCKS) (sums: two pairs per thread); trips = pairs / (workgroups x
             pairs per workgroup), ragged when that is no integer. zg_run_sumcheck's launches are clamped to 1024 workgroups.

One child holds one eq set, one Spartan set and one fold set: the three families read disjoint switches.
A set with "pytest" runs existing test nodes of the suite in this process under the switches instead (nothing else holds the GPU)."""
import hashlib
import os
import sys

import numpy as np

# eq: (v, shape with wide challenges, shape with 128-bit challenges); shape = (template WG, rows per workgroup, workgroups, expanding kernel)
# spartan: (v, (template WG, rows per workgroup, workgroups))
# fold: sizes (log2 entries) and, per size, (fold threads, fold workgroups, sums threads, sums workgroups, 256-thread workgroups)
SETS = {
    # <1>, 16 and 32 rows per workgroup, two workgroups: the default shape from v = 21 on (512 workgroups there)
    "eq1x2-sp1x1-sc3x64": {
        "env": {"ZG_EQ_WG": "1", "ZG_EQ_BLOCKS": "2", "ZG_SC_SPARTAN_BLOCKS": "1", "ZG_SC_SPARTAN_WG": "1",
                "ZG_SC_MAX_BLOCKS": "3", "ZG_SC_FOLD_THREADS": "64", "ZG_SC_SUMS_THREADS": "64"},
        "eq": [(13, (1, 16, 2, 0), (1, 16, 2, 0)), (14, (1, 32, 2, 0), (1, 32, 2, 0))],
        "spartan": [(10, (1, 4, 1)), (12, (1, 16, 1)), (17, (1, 256, 2))],
        "fold": {12: (64, 3, 64, 3, 3), 13: (64, 3, 64, 3, 3)}, "fold_min_trips": 3, "fold_ragged": True,
    },
    # <1>, rows capped at EQ_MAX_ROWS = 256: one full workgroup (v = 16) and two (v = 17), the default shape from v = 26 on;
    # the production thread counts (512 fold / 1024 sums) with 16 / 4 trips
    "eq1x1-sp1x2-sc2": {
        "env": {"ZG_EQ_WG": "1", "ZG_EQ_BLOCKS": "1", "ZG_SC_SPARTAN_BLOCKS": "1", "ZG_SC_SPARTAN_WG": "2", "ZG_SC_MAX_BLOCKS": "2"},
        "eq": [(16, (1, 256, 1, 0), (1, 256, 1, 0)), (17, (1, 256, 2, 0), (1, 256, 2, 0))],
        "spartan": [(10, (2, 4, 1)), (12, (2, 16, 1)), (17, (2, 256, 2))],
        "fold": {14: (512, 2, 1024, 2, 2), 15: (512, 2, 1024, 2, 2)}, "fold_min_trips": 2, "fold_ragged": False,
    },
    # <2>, three workgroups, the last one short (4 of 6 rows, 10 of 11), 3 rows per thread group (v = 12) and 6 / 5 (v = 13): the two-row
    # trip and the remainder row in one workgroup; v = 9: one row per workgroup falls back to <1>; v = 11: the last workgroup has 2 of 3 rows
    "eq2x3-sp3x1-sc1x192": {
        "env": {"ZG_EQ_WG": "2", "ZG_EQ_BLOCKS": "3", "ZG_SC_SPARTAN_BLOCKS": "3", "ZG_SC_SPARTAN_WG": "1",
                "ZG_SC_MAX_BLOCKS": "1", "ZG_SC_FOLD_THREADS": "192", "ZG_SC_SUMS_THREADS": "192"},
        "eq": [(9, (1, 1, 2, 0), (1, 1, 2, 0)), (10, (2, 2, 2, 0), (2, 2, 2, 0)), (11, (2, 3, 3, 0), (2, 3, 3, 0)),
               (12, (2, 6, 3, 0), (2, 6, 3, 0)), (13, (2, 11, 3, 0), (2, 11, 3, 0))],
        "spartan": [(10, (1, 2, 2)), (12, (1, 6, 3))],
        "fold": {11: (192, 1, 192, 1, 1)}, "fold_min_trips": 3, "fold_ragged": True,
    },
    # <4> with 6 and 11 rows per workgroup (groups of 2 / 1 and 3 / 2 rows), ragged; <4> asked for with 1, 2 and 3 rows per workgroup
    # falls back to <1>, <2>, <2>. Fold: zg_run_sumcheck's launches clamped to SC_RUN_PAIRS = 1024 workgroups where a session takes 2048
    "eq4x3-sp3x2-scrun": {
        "env": {"ZG_EQ_WG": "4", "ZG_EQ_BLOCKS": "3", "ZG_SC_SPARTAN_BLOCKS": "3", "ZG_SC_SPARTAN_WG": "2",
                "ZG_SC_MAX_BLOCKS": "2048", "ZG_SC_FOLD_THREADS": "64"},
        "eq": [(9, (1, 1, 2, 0), (1, 1, 2, 0)), (10, (2, 2, 2, 0), (2, 2, 2, 0)), (11, (2, 3, 3, 0), (2, 3, 3, 0)),
               (12, (4, 6, 3, 0), (4, 6, 3, 0)), (13, (4, 11, 3, 0), (4, 11, 3, 0))],
        "spartan": [(10, (2, 2, 2)), (12, (2, 6, 3))],
        "run_clamp": 18,
    },
    # eq_expand_kernel<2>, three workgroups of 3 / 6 / 11 rows of 2048 entries, the last one short; wide challenges in the middle of
    # the index take eq_main_kernel<2> at the same sizes (22, 43, 86 rows per workgroup); v = 13 is below the expanding kernel's least size
    "eqx3": {
        "env": {"ZG_EQ_EXPAND": "14", "ZG_EQ_BLOCKS": "3"},
        "eq": [(13, (2, 11, 3, 0), (2, 11, 3, 0)), (14, (2, 22, 3, 0), (2, 3, 3, 1)), (15, (2, 43, 3, 0), (2, 6, 3, 1)),
               (16, (2, 86, 3, 0), (2, 11, 3, 1))],
    },
    # eq_expand_kernel<1>: one row per workgroup
    "eqx64": {
        "env": {"ZG_EQ_EXPAND": "14", "ZG_EQ_BLOCKS": "64"},
        "eq": [(14, (1, 1, 64, 0), (1, 1, 8, 1)), (15, (2, 2, 64, 0), (1, 1, 16, 1))],
    },
    # Stage 4 with one register chunk per thread (the shape of T = 2^20: 4096 and 2048 cycle pairs are at least the 1024 threads asked
    # for) and with two; expression rounds never one lane per (pair, term, point)
    "rrw1024-psc0": {
        "env": {"ZG_RRW_THREADS": "1024", "ZG_PSC_SPREAD_MAX_PAIRS": "0"},
        "rrw": [((4096, 32), 1), ((2048, 32), 1), ((512, 32), 2)], "psc": [(32, (1, 0)), (8192, (32, 0))],
        "pytest": ["test_gpu_stage4.py::test_rounds_against_the_restatement[10-1000-5]", "test_gpu_stage4.py::test_rounds_against_the_restatement[13-8000-1]",
                   "test_gpu_stage4.py::test_original_stage4_prover_against_the_restatement[10-1000]",
                   "test_gpu_stage4.py::test_original_stage4_prover_against_the_restatement[12-4000]",
                   "test_gpu_product_sumcheck.py::test_round_expr_against_big_int_model", "test_gpu_product_sumcheck.py::test_instruction_input_prover[10]"],
    },
    # no cycle fold under the row masks; expression rounds one lane per (pair, term, point) up to 65536 pairs (8192 pairs: 512 workgroups)
    "rrwmask0-psc65536": {
        "env": {"ZG_RRW_MASKED_FOLDS": "0", "ZG_PSC_SPREAD_MAX_PAIRS": "65536"},
        "rrw": [((512, 32), 32)], "psc": [(32, (2, 1)), (8192, (512, 1))],
        "pytest": ["test_gpu_stage4.py::test_rounds_against_the_restatement[6-50-3]", "test_gpu_stage4.py::test_rounds_against_the_restatement[10-1000-5]",
                   "test_gpu_stage4.py::test_original_stage4_prover_against_the_restatement[8-256]",
                   "test_gpu_product_sumcheck.py::test_round_expr_against_big_int_model", "test_gpu_product_sumcheck.py::test_instruction_input_prover[14]"],
    },
    # every cycle fold of phase 1 under the row masks
    "rrwmask30": {
        "env": {"ZG_RRW_MASKED_FOLDS": "30"},
        "rrw": [((512, 32), 32)],
        "pytest": ["test_gpu_stage4.py::test_rounds_against_the_restatement[6-50-3]", "test_gpu_stage4.py::test_rounds_against_the_restatement[10-1000-5]",
                   "test_gpu_stage4.py::test_original_stage4_prover_against_the_restatement[8-256]"],
    },
}

R_TOP = 0x30644E72E131A029  # top u64 limb of r: [0, 0, lo, hi] is a canonical element for hi < R_TOP


def _ok(what):
    print("ok:", what, flush=True)


class Checks:
    def __init__(self):
        from oracle import binding as ob
        from tests import util as U
        from zolt_amd import api, lib
        lib.init()
        self.ob, self.U, self.api, self.lib = ob, U, api, lib

    def rand(self, seed, n):
        return self.ob.f_to_mont(self.ob.FR, self.U.random_raw256(seed, n)) if n else np.zeros((0, 4), dtype=np.uint64)

    def narrow(self, seed, n):
        """n stored elements [0, 0, lo, hi], the form of the reference's 128-bit challenges, with the extremes in front"""
        w = self.U.splitmix64(seed, 2 * max(n, 1)).reshape(-1, 2)[:n]
        out = np.zeros((n, 4), dtype=np.uint64)
        out[:, 2] = w[:, 0]
        out[:, 3] = w[:, 1] & np.uint64((1 << 61) - 1)
        for i, (lo, hi) in enumerate([((1 << 64) - 1, R_TOP - 1), (0, 0), (1, 0), (0, 1 << 60)][:n]):
            out[i, 2], out[i, 3] = lo, hi
        return out

    def shape(self, family, a, b, want, what):
        got = self.lib.launch_shape(family, a, b)[:len(want)]
        assert got == tuple(want), f"{what}: the library would launch {got}, this case is written for {tuple(want)}"

    # ---- eq table
    def eq(self, cases):
        lib, ob = self.lib, self.ob
        for v, wide_shape, narrow_shape in cases:
            for kind, r, want in (("wide", self.rand(100 + v, v), wide_shape), ("128-bit", self.narrow(200 + v, v), narrow_shape)):
                self.shape(lib.SHAPE_EQ_TABLE, v, int(kind == "128-bit"), want, f"eq table v={v} {kind}")
                for scale in (None, self.rand(300 + v, 1)[0]):
                    assert np.array_equal(lib.fr_eq_table(r, scale), ob.fr_eq_table(r, scale)), (v, kind, scale is not None)
                _ok(f"eq table v={v} {kind} challenges, with and without scale, shape {want}")
            if narrow_shape[3]:  # one wide challenge among the three middle variables: not the expanding kernel
                r = self.narrow(200 + v, v)
                r[v - 10] = self.rand(400 + v, 1)[0]
                self.shape(lib.SHAPE_EQ_TABLE, v, 0, wide_shape, f"eq table v={v} mixed")
                assert np.array_equal(lib.fr_eq_table(r), ob.fr_eq_table(r)), (v, "mixed")
                _ok(f"eq table v={v} 128-bit challenges but one in the middle, shape {wide_shape}")

    # ---- fused Spartan open
    def spartan(self, cases):
        lib, ob = self.lib, self.ob
        for v, want in cases:
            n = 1 << v
            self.shape(lib.SHAPE_EQ_SPARTAN, v, 0, want, f"spartan open v={v}")
            az, bz, cz = (self.rand(500 + 3 * v + k, n) for k in range(3))
            d = [lib.DeviceBuffer.from_host(t) for t in (az, bz, cz)]
            for layout in (lib.SC_HIGH_HALF, lib.SC_LOW_PAIR):
                for kind, r in (("wide", self.rand(600 + v, v)), ("128-bit", self.narrow(700 + v, v))):
                    scale = self.rand(800 + v, 1)[0] if kind == "wide" else None
                    table = ob.fr_spartan_combine(ob.fr_eq_table(r, scale), az, bz, cz)
                    s = lib.SumcheckSession.open_spartan_dev(r, d[0].ptr, d[1].ptr, d[2].ptr, layout=layout, scale=scale)
                    assert len(s) == n and np.array_equal(s.read(), table), (v, layout, kind)
                    self.rounds(s, table, layout, self.rand(900 + v, v), 2)
                    s.close()
                _ok(f"spartan open v={v} layout {layout}, wide challenges with scale and 128-bit without, shape {want}")
            for b in d:
                b.free()

    def rounds(self, s, table, layout, chals, n_rounds):
        """a session's round sums and folds against the oracle's, table by table"""
        lib, ob = self.lib, self.ob
        cur = table
        for k in range(n_rounds):
            g0, g1 = s.round_sums()
            w0, w1 = ob.fr_sum_halves(cur) if layout == lib.SC_HIGH_HALF else ob.fr_sum_even_odd(cur)
            assert np.array_equal(g0, w0) and np.array_equal(g1, w1), ("round sums", len(cur), layout, k)
            s.bind(chals[k])
            cur = ob.fr_bind_high(cur, chals[k]) if layout == lib.SC_HIGH_HALF else ob.fr_bind_low(cur, chals[k])
            assert hashlib.sha256(s.read().tobytes()).digest() == hashlib.sha256(cur.tobytes()).digest(), ("fold", len(cur), layout, k)
        return cur

    # ---- fold / sums / the 256-thread pair-sum kernels
    def fold(self, sizes, min_trips, ragged):
        lib, ob, api, U = self.lib, self.ob, self.api, self.U
        for v, (ft, fb, st, sb, pb) in sizes.items():
            n, half = 1 << v, 1 << (v - 1)
            for run in (0, 1):
                self.shape(lib.SHAPE_SC_FOLD, half, run, (ft, fb), f"fold 2^{v} run={run}")
                self.shape(lib.SHAPE_SC_SUMS, half, run, (st, sb), f"sums 2^{v} run={run}")
            for what, elems in (("raf round", half), ("raf claim", n), ("bit split", n - 1097)):
                self.shape(lib.SHAPE_SC_PAIRSUM, elems, 0, (256, pb), f"{what} 2^{v}")
            self.shape(lib.SHAPE_HK_FOLD, half, 0, (256, pb), f"quotient fold 2^{v}")
            # trips of the first launch of each kernel: pairs over (workgroups x pairs per workgroup)
            for what, pairs, per in (("fold", half, fb * ft), ("sums", half, sb * st * 2), ("raf round", half, pb * 256), ("raf claim", n, pb * 256),
                                     ("bit split", n - 1097, pb * 256), ("quotient fold", half, pb * 256)):
                trips = -(-pairs // per)  # (a power-of-two table over a power-of-two grid has no ragged last trip)
                assert trips >= min_trips and (not ragged or pairs % per or not per & (per - 1)), (what, v, pairs, per)
            t = self.rand(1000 + v, n)
            for layout in (lib.SC_HIGH_HALF, lib.SC_LOW_PAIR):
                for kind, ch in (("wide", self.rand(1100 + v, v)), ("128-bit", self.narrow(1200 + v, v))):
                    s = lib.SumcheckSession.open(t, layout)
                    cur = self.rounds(s, t, layout, ch, v)
                    assert np.array_equal(s.final(), cur[0])
                    s.close()
                _ok(f"session 2^{v} layout {layout}: every round's sums and fold, fold {ft} x {fb}, sums {st} x {sb}")
            want = ob.run_sumcheck(t)
            for tail in (n, n // 2, 1):
                os.environ["ZG_SC_TAIL_MAX"] = str(tail)  # read per call
                try:
                    self.run_sumcheck(t, want)
                finally:
                    del os.environ["ZG_SC_TAIL_MAX"]
                _ok(f"zg_run_sumcheck 2^{v} with the LDS tail from {tail} entries")
            self.raf(v, t)
            m = n - 1097  # an odd count
            idx = U.splitmix64(1300 + v, 2 * m).reshape(m, 2)
            for bit in (0, 63, 64, 127):
                g0, g1 = lib.fr_bit_split_sums(t[:m], idx, bit)
                w0, w1 = ob.lasso_address_sums(t[:m], idx, bit)
                assert np.array_equal(g0, w0) and np.array_equal(g1, w1), ("bit split", v, bit)
            _ok(f"zg_fr_bit_split_sums over {m} values, 256 x {pb}")
            self.hyperkzg_open(v, t)

    def run_sumcheck(self, t, want):
        res = self.lib.run_sumcheck(t)
        wc, wr, wch, wfin, wok = want
        assert res["result"] and wok == 1 and np.array_equal(res["claim"], wc) and np.array_equal(res["final_eval"], wfin)
        assert np.array_equal(res["rounds"].reshape(-1, 2, 4), np.asarray(wr).reshape(-1, 2, 4))
        assert np.array_equal(res["final_point"].reshape(-1, 4), np.asarray(wch).reshape(-1, 4))

    def raf(self, log_k, ra):
        """RafEvaluationProver: zg_sumcheck_raf_claim against exact integers, then every zg_sumcheck_raf_round and LOW_PAIR fold against the oracle"""
        api, ob, U = self.api, self.ob, self.U
        start = 0x7FFF8000
        claim = sum(U.fr_to_int(x) * (start + 8 * k) for k, x in enumerate(ra)) % api.R_MOD
        prover = api.RafEvaluationProver(ra, start, log_k)
        assert U.fr_to_int(prover.current_claim) == claim, ("raf claim", log_k)
        cur, bound, wclaim = ra.copy(), np.zeros((0, 4), dtype=np.uint64), api.fr_from_int(claim)
        ch = self.narrow(1400 + log_k, log_k)
        ch[1::2] = self.rand(1500 + log_k, log_k)[1::2]
        for rd in range(log_k):
            got, want = prover.computeRoundPolynomialCubic(), ob.raf_round_cubic(cur, start, bound, log_k, wclaim)
            assert np.array_equal(got, want), ("raf round", log_k, rd)
            prover.updateClaim(got, ch[rd])
            wclaim = ob.raf_update_claim(want, ch[rd])
            prover.bindChallenge(ch[rd])
            cur = ob.fr_bind_low(cur, ch[rd])
            bound = np.concatenate([bound, ch[rd][None, :]])
        assert np.array_equal(prover.getFinalClaim(), cur[0]) and np.array_equal(prover.current_claim, wclaim)
        prover.deinit()
        _ok(f"raf claim and {log_k} raf rounds over 2^{log_k} entries")

    def hyperkzg_open(self, v, ev):
        lib, ob = self.lib, self.ob
        n = 1 << v
        gm, inf = ob.g1_gen_multiples(n), np.zeros(n, dtype=np.uint8)
        pt = self.rand(1600 + v, v)
        zero = np.zeros(4, dtype=np.uint64)
        h = lib.Bases.upload(gm)
        q, qi, fin = lib.hyperkzg_open(h, ev, pt, zero)
        h.free()
        wq, wqi, wfin = ob.hyperkzg_open(gm, inf, ev, pt, zero)
        assert np.array_equal(fin, wfin) and np.array_equal(qi, wqi) and np.array_equal(q, wq), ("hyperkzg open", v)
        _ok(f"zg_hyperkzg_open 2^{v}: {v} quotient commitments and the final evaluation")

    def run_clamp(self, v):
        """zg_run_sumcheck where the grid of a session's launch exceeds the device-resident protocol's 1024 block pairs"""
        lib, ob = self.lib, self.ob
        half = 1 << (v - 1)
        self.shape(lib.SHAPE_SC_FOLD, half, 0, (64, 2048), f"session fold 2^{v}")
        self.shape(lib.SHAPE_SC_FOLD, half, 1, (64, 1024), f"run fold 2^{v}")  # two trips per thread
        self.shape(lib.SHAPE_SC_FOLD, half // 2, 1, (64, 1024), f"run fold 2^{v - 1}")
        t = self.rand(1700 + v, 1 << v)
        self.run_sumcheck(t, ob.run_sumcheck(t))
        _ok(f"zg_run_sumcheck 2^{v}: folds of 64 x 1024 where a session launches 64 x 2048")


def main(name):
    spec = SETS[name]
    for key, val in spec["env"].items():
        assert os.environ.get(key) == val, f"{key} is not {val} in this process's environment"
    if "pytest" in spec:
        try:
            import torch  # noqa: F401  (before libzolt_gpu.so, as tests/conftest.py has it)
        except Exception:
            pass
        from zolt_amd import lib
        for (inner, outer), chunks in spec.get("rrw", []):
            got = lib.launch_shape(lib.SHAPE_RRW, inner, outer)[0]
            assert got == chunks, f"Stage-4 round over {inner} x {outer}: {got} register chunks, written for {chunks}"
            _ok(f"Stage-4 round over {inner} x {outer}: {chunks} register chunk(s)")
        for pairs, want in spec.get("psc", []):
            got = lib.launch_shape(lib.SHAPE_PSC, pairs)[:2]
            assert got == want, f"expression round over {pairs} pairs: (workgroups, spread) = {got}, written for {want}"
            _ok(f"expression round over {pairs} pairs: {want[0]} workgroups, spread {want[1]}")
        import pytest
        here = os.path.dirname(os.path.abspath(__file__))
        rc = pytest.main(["-q", "-x", "-p", "no:cacheprovider"] + [os.path.join(here, node) for node in spec["pytest"]])
        assert rc == 0, f"pytest ended with {rc}"
    else:
        c = Checks()
        if "eq" in spec:
            c.eq(spec["eq"])
        if "spartan" in spec:
            c.spartan(spec["spartan"])
        if "fold" in spec:
            c.fold(spec["fold"], spec["fold_min_trips"], spec["fold_ragged"])
        if "run_clamp" in spec:
            c.run_clamp(spec["run_clamp"])
    print("launch shapes ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
