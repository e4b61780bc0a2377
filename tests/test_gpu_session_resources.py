"""The runtime's shared session resources (csrc/runtime.hip: device blocks, pinned buffers, mailboxes, zeroed counter blocks, streams) as
they pass from one kind of session to another, under ZG_POOL_DEBUG=1. A closed session keeps nothing: its counter block, mailbox, stream
and tables are what the next session of ANY kind is handed, so each step below closes one kind and opens another on what it left, and
holds every result against oracle.binding. The steps run in order, each in a fresh child process (the debug mode is read from the
environment once) under a time limit of its own; the first one that does not end with status 0 ends the chain."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sc_len():
    """the first power of two from 2^13 at which a session's sums launch and its fold launch both have at least two workgroups
    (csrc/poly.hip: sums_grid = div_up(len / 2, sums_threads * SC_SUMS_U), fold_grid = div_up(len / 2, fold_threads), both capped), so
    that the arrival counters of the counter block are really used; 2^13 where a switch caps every grid at one workgroup"""
    src = open(os.path.join(ROOT, "zolt_amd", "csrc", "poly.hip")).read()
    m = re.search(r"constexpr\s+int\s+SC_SUMS_U\s*=\s*(\d+)\s*;", src)
    dflt = {name: int(d) for name, d in re.findall(r'env_uint\(\s*"(ZG_SC_(?:SUMS|FOLD)_THREADS)"\s*,\s*(\d+)\s*,', src)}
    assert m and set(dflt) == {"ZG_SC_SUMS_THREADS", "ZG_SC_FOLD_THREADS"} and "div_up(half ? half : 1, (size_t)sums_threads() * SC_SUMS_U)" in src \
        and "div_up(half ? half : 1, fold_threads())" in src, "csrc/poly.hip: sums_grid / fold_grid are not what this helper restates: bring it up to date"
    unroll = int(m.group(1))
    threads = {name: max(64, min(d, int(os.environ.get(name) or d))) & ~63 for name, d in dflt.items()}
    cap = int(os.environ.get("ZG_SC_MAX_BLOCKS") or 0) or 256
    for v in range(13, 20):
        half = (1 << v) // 2
        sums = min(cap, -(-half // (threads["ZG_SC_SUMS_THREADS"] * unroll)))
        fold = min(cap, -(-half // threads["ZG_SC_FOLD_THREADS"]))
        if sums >= 2 and fold >= 2:
            return 1 << v
    return 1 << 13


PRELUDE = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from zolt_amd import api, lib
from oracle import binding as ob
from tests import util as U
N = %(n)d


def fr(seed, n):
    return ob.f_to_mont(ob.FR, U.random_raw256(seed, n))


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def sc_rounds(s, ev, seed, what):
    # sums, bind, sums on an open single-table session, then close
    for rnd in range(2):
        g, w = s.round_sums(), ob.fr_sum_halves(ev)
        assert eq(g[0], w[0]) and eq(g[1], w[1]), (what, "round_sums", rnd)
        if rnd == 0:
            r = fr(seed, 1)[0]
            s.bind(r)
            ev = ob.fr_bind_high(ev, r)
    assert eq(s.read().reshape(-1, 4), ev), (what, "table")
    s.close()


def run_sumcheck(ev, what):
    got, want = lib.run_sumcheck(ev), ob.run_sumcheck(ev)
    assert got["result"] and want[4] == 1, what
    for key, w in zip(("claim", "rounds", "final_point", "final_eval"), want):
        assert eq(got[key], w), (what, key)


def psc_rounds(s, tabs, seed, what, rounds=2):
    # two tables, their product: evaluations, bind, evaluations (the second set comes out of the fused fold), then close
    cur = [t.copy() for t in tabs]
    for rnd in range(rounds):
        want = ob.ValEvaluationProver(cur[0], cur[1], None, cur[0][0]).computeRoundPolynomial()
        assert eq(s.round_evals((0, 1)), want), (what, "round_evals", rnd)
        r = fr(seed + rnd, 1)[0]
        s.bind(r)
        cur = [ob.fr_bind_low(t, r) for t in cur]
    for j in range(2):
        assert eq(s.read(j), cur[j]), (what, "table", j)
    s.close()
    return cur
"""

STEPS = {}

# 1 + 2: one counter block and one mailbox through zg_sc (flag at word 12), zg_run_sumcheck (flag in the last word, 17 + 12 v result
# words over the first ones), a second zg_sc — whose first round_sums would return at once with old values on a stale flag word — then
# zg_psc (flag at word 24; its counter block is of another size: a block of its own, zeroed once) and zg_sc again
STEPS["hand_over"] = r"""
lib.init(0)
ev, tabs = fr(1, N), [fr(2, N), fr(3, N)]
sc_rounds(lib.SumcheckSession.open(ev), ev, 10, "first sc")
run_sumcheck(ev, "run_sumcheck after sc")
sc_rounds(lib.SumcheckSession.open(ev), ev, 11, "second sc")
psc_rounds(lib.ProductSumcheckSession.open(tabs), tabs, 20, "first psc")
run_sumcheck(tabs[0], "run_sumcheck after psc")
psc_rounds(lib.ProductSumcheckSession.open(tabs), tabs, 30, "second psc")
sc_rounds(lib.SumcheckSession.open(tabs[1]), tabs[1], 12, "sc after psc")
d = lib.DeviceBuffer.from_host(ev)  # a borrowed table: the session's own blocks are the folds' only
sc_rounds(lib.SumcheckSession.open_dev(d.ptr, N, borrow=True), ev, 13, "borrowed sc")
d.free()
lib.dev_trim()
print(json.dumps(lib.pool_debug_stats()))
"""

# 3: the tables of a registers session (log_t = 4) and of a RAM session (log_k = 4, log_t = 4, 8 entries) go back to the pool and are
# taken again in the opposite order; both provers against the restatements their own tests use
STEPS["tables_travel"] = r"""
from tests.test_gpu_stage4 import seeded_steps
from tests.test_gpu_rwc import _trace
lib.init(0)
P = ob._R_P
r = fr(40, 1 + 4 + 11)
gamma, r_cycle, chals = r[0], r[1:5], r[5:]
steps = seeded_steps(104, 16)
acc, initial = _trace(4004, 4, 4, 8, 0x80000000)
zero = np.zeros(4, dtype=np.uint64)


def registers(what):
    o, d = ob.Stage4GruenProver(steps, gamma, r_cycle, 4, 7), api.Stage4GruenProver(steps, gamma, r_cycle, 4, 7)
    claim = o.computeInputClaim()
    for k in range(11):
        eo = o.computeRoundEvals(k, claim)
        assert eq(eo, d.computeRoundEvals(k, claim)), (what, k)
        claim = ob.raf_update_claim(eo, chals[k])
        o.bindChallenge(k, chals[k])
        d.bindChallenge(k, chals[k])
    fo, fd = o.getFinalClaims(), d.getFinalClaims()
    assert all(eq(fo[name], fd[name]) for name in fo), what
    d.deinit()


def ram(what):
    o = ob.RamReadWriteCheckingProver(acc, gamma, r_cycle, 4, 4, 2, 0x80000000, zero, initial)
    assert len(o.entries) == 8
    g = ob.fr_to_int(gamma)
    claim = sum(ob.fr_to_int(o.eq_evals[e[0]]) * e[2] * (e[3] + g * (e[3] + ob.fr_to_int(o.inc[e[0]]))) for e in o.entries) % P
    o.current_claim = claim
    d = api.RamReadWriteCheckingProver(acc, gamma, r_cycle, 4, 4, 2, 0x80000000, ob.fr_from_int(claim), initial)
    used = []
    for rd in range(8):
        we = o.computeRoundPolynomialCubic()
        assert eq(d.computeRoundPolynomialCubic(), we), (what, rd)
        used.append(chals[rd])
        for x in (o, d):
            x.updateClaim(we, chals[rd])
            x.bindChallenge(chals[rd])
        assert d.current_claim == o.current_claim, (what, rd)
    assert d.entries_full() == [[e[0], e[1], e[2] % P, e[3] % P, e[4], e[5]] for e in o.entries], what
    assert all(eq(a, b) for a, b in zip(d.getOpeningClaims(np.stack(used)), o.getOpeningClaims(np.stack(used)))), what
    d.deinit()


registers("registers, first")
ram("ram, first")
ram("ram, on the blocks the two left")
registers("registers, after the ram sessions")
lib.dev_trim()
print(json.dumps(lib.pool_debug_stats()))
"""

# 4: a zg_sc and a zg_psc session live across zg_shutdown: used and closed after the next zg_init (their counter blocks and mailboxes
# are not the runtime's any more: freed, once), then fresh ones that compute the same
STEPS["lifecycle"] = r"""
ev, tabs = fr(5, N), [fr(6, N), fr(7, N)]
for cycle in range(2):
    lib.init(0)
    sc_rounds(lib.SumcheckSession.open(ev), ev, 50, ("idle resources for the shutdown", cycle))
    s, p = lib.SumcheckSession.open(ev), lib.ProductSumcheckSession.open(tabs)
    lib.shutdown()
    lib.init(0)
    sc_rounds(s, ev, 51, ("sc that outlived a shutdown", cycle))
    psc_rounds(p, tabs, 60, ("psc that outlived a shutdown", cycle))
    sc_rounds(lib.SumcheckSession.open(ev), ev, 51, ("fresh sc", cycle))
    psc_rounds(lib.ProductSumcheckSession.open(tabs), tabs, 60, ("fresh psc", cycle))
    run_sumcheck(ev, ("run_sumcheck", cycle))
    lib.dev_trim()
    stats = lib.pool_debug_stats()
    lib.shutdown()
print(json.dumps(stats))
"""


@pytest.fixture(scope="module")
def chain():
    env = dict(os.environ)
    env.pop("ZG_DEV_ALLOC_CACHE_MB", None)  # (0 = the pool keeps nothing: there is no reuse to check)
    env["ZG_POOL_DEBUG"] = "1"
    prelude = PRELUDE % {"root": ROOT, "n": _sc_len()}
    done = {}
    for name, body in STEPS.items():
        res = subprocess.run([sys.executable, "-c", prelude + body], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        done[name] = res
        if res.returncode != 0:
            break
    return done


def _stats(chain, name):
    assert name in chain, "not run: an earlier step did not end with status 0"
    res = chain[name]
    assert res.returncode == 0, (res.returncode, res.stdout[-500:], res.stderr[-1500:])
    st = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert st["mode"] == 1 and st["hits"] == 0 and st["blocks_verified"] > 0, st
    return st


def test_counter_blocks_and_mailboxes_pass_between_session_kinds(chain):
    _stats(chain, "hand_over")


def test_table_blocks_travel_between_session_kinds(chain):
    _stats(chain, "tables_travel")


def test_sessions_that_outlive_a_shutdown_free_their_resources_once(chain):
    _stats(chain, "lifecycle")
