"""An MSM's result must not depend on what its workspace held before.

msm_enqueue hands every MSM the handle's next workspace ("lane", zg_bases_s::Lane) in round robin, and a lane carries sorted lists,
bucket starts, non-empty lists, partial sums, bucket sums, heavy lists, arrival counters and slice buffers from one launch set to the
next (docs/design/05_msm.md: "What a lane carries between launch sets"). Which of them a kernel rewrites on every launch and which it
assumes are already right is the line every change to the sort, accumulate and bucket-tail kernels moves. Elsewhere in the suite a lane
is either fresh or last held an MSM of the same shape, whose leftovers are correct data. Here one handle per configuration runs
workloads of very different shapes (tests/msm_reuse_workloads.py: dense, empty, one entry, top window only, one huge bucket, hundreds of
heavy buckets, cancelling pairs, a 37-point range, a side-table prefix) in the order of all_pairs_order: every workload is launched
right after every other one and after itself, on the lane the other one just used. Every result is compared bit for bit, coordinates
and flag, with the closed form (sum s_i k_i) * G for bases k_i * G, computed once per workload; the identity is all-zero words with flag 1.
A mismatch is reported as (configuration, previous workload, this workload, position in the walk).

tests/test_msm_reuse_workloads.py holds the CPU side: the closed form against the oracle, the census of what each workload leaves in a
workspace under each configuration's plan, and the walk.

msm_rows_shared_tail (rows_cap and the d_rows_* buffers) is not reachable through zg_msm_g1_batch: it runs only for the long levels of
HyperKZG.open on a key without a table (msm_batch_dev_wide; more than 16384 entries a level) whose bucket sets are too many to fuse
(15-bit windows), and vectors of at most 16384 scalars on such a handle go to its side table. The batch legs on the one-proof key therefore hold the side table's fused workspace and the
handle's own lane; test_rows_of_long_levels_on_a_key_without_a_table holds the rows' buffers through openings.
"""
import numpy as np
import pytest

from tests import msm_reuse_workloads as W
from tests import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


@pytest.fixture(scope="module")
def gm(ob):
    return ob.g1_gen_multiples(20000)  # (i + 1) G: both halves of the largest handle (40000 bases)


_prepared = {}


def _prepare(gm, N, c, extra=(), flagged=False):
    """bases, flags, workloads, their Montgomery scalars and expected records (closed form, once per workload), and the walk"""
    key = (N, c, extra, flagged)
    if key not in _prepared:
        flags = W.default_flags(N) if flagged else None
        ks = W.base_multipliers(N, flags)
        wls = W.workloads(N, c, extra=extra)
        _prepared[key] = dict(xy=W.bases(gm, N), flags=flags, wls=wls, sc=[W.fr_mont(w[3]) for w in wls],
                              want=[W.result_record(W.closed_form(ks, w)) for w in wls], walk=W.all_pairs_order(len(wls)))
    return _prepared[key]


def _upload(zl, monkeypatch, conf, xy, flags=None, **more_env):
    for k in W.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**conf["env"], **more_env}.items():
        monkeypatch.setenv(k, v)
    b = zl.Bases.upload(xy, flags, **conf["cfg"])
    c, windows, levels = b.plan()
    assert c == conf["plan"]["c"] and windows == (255 + c - 1) // c and (levels == 1) == (conf["plan"]["G"] > 1), (c, windows, levels)
    return b


def _mismatches(label, prep, records, lanes=1):
    """records[pos]: the nine words MSM number pos of the walk gave"""
    wls, walk, out = prep["wls"], prep["walk"], []
    for pos, j in enumerate(walk):
        if not np.array_equal(records[pos], prep["want"][j]):
            prev = wls[walk[pos - 1]][0] if pos else None
            on_lane = wls[walk[pos - lanes]][0] if lanes > 1 and pos >= lanes else prev
            out.append((label, prev, wls[j][0], pos) + ((f"lane last held {on_lane}",) if lanes > 1 else ()))
    return out


def _walk_host(b, label, prep, lanes=1):
    """the walk through zg_msm_g1: host scalars, one MSM at a time"""
    records = []
    for j in prep["walk"]:
        _, off, n, _ = prep["wls"][j]
        got, ginf = b.msm(prep["sc"][j], off=off, n=n)
        records.append(np.concatenate([got, np.array([ginf], dtype=np.uint64)]))
    bad = _mismatches(label, prep, records, lanes)
    assert not bad, (len(bad), bad[:12])


def _walk_async(b, label, prep, nstreams):
    """the walk through zg_msm_g1_dev_async over nstreams streams in turn: every workload's scalars are resident before the first call,
    the records land in one device array, and nothing synchronises with the host until the last call is enqueued. On a handle with one
    lane consecutive calls on different streams are ordered by the lane's `done` event alone."""
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(sc.view(np.int64)).to(dev) for sc in prep["sc"]]
    outs = torch.zeros((len(prep["walk"]), 9), dtype=torch.int64, device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(nstreams)]
    torch.cuda.synchronize()
    for pos, j in enumerate(prep["walk"]):
        _, off, n, _ = prep["wls"][j]
        b.msm_dev_async(d[j].data_ptr(), n, outs[pos].data_ptr(), outs[pos, 8:].data_ptr(), off=off, stream=streams[pos % nstreams].cuda_stream)
    torch.cuda.synchronize()
    o = outs.cpu().numpy().view(np.uint64)
    o[:, 8] &= np.uint64(0xFF)  # the flag is one byte
    bad = _mismatches(label, prep, list(o))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("name", list(W.CONFIGS))
def test_walk(zl, gm, name, monkeypatch):
    conf = W.CONFIGS[name]
    prep = _prepare(gm, conf["N"], conf["plan"]["c"], conf["extra"])
    assert len(prep["walk"]) == len(prep["wls"]) ** 2 + 1 and len(prep["wls"]) == 11 + len(conf["extra"])
    b = _upload(zl, monkeypatch, conf, prep["xy"])
    try:
        _walk_host(b, name, prep, lanes=1 if "ZG_MSM_LANES" in conf["env"] or conf["cfg"].get("expected_uses") else 6)
    finally:
        b.free()


@pytest.mark.parametrize("nstreams", [1, 2], ids=["one-stream", "two-streams"])
@pytest.mark.parametrize("name", ["one-lane", "two-pass"])
def test_walk_async(zl, gm, name, nstreams, monkeypatch):
    conf = W.CONFIGS[name]
    prep = _prepare(gm, conf["N"], conf["plan"]["c"], conf["extra"])
    b = _upload(zl, monkeypatch, conf, prep["xy"])
    try:
        _walk_async(b, f"{name}, {nstreams} stream(s)", prep, nstreams)
    finally:
        b.free()


def test_walk_with_infinity_flags(zl, gm, monkeypatch):
    """flagged bases are never referenced: fewer entries in every workload, CANCEL no longer cancels, the same code path"""
    conf = W.CONFIGS["one-lane"]
    prep = _prepare(gm, conf["N"], conf["plan"]["c"], conf["extra"], flagged=True)
    assert prep["flags"].sum() > 20 and prep["flags"][:conf["N"] // 2].any() and prep["flags"][conf["N"] // 2:].any()
    b = _upload(zl, monkeypatch, conf, prep["xy"], prep["flags"])
    try:
        _walk_host(b, "one-lane, flags", prep)
    finally:
        b.free()


# ---- batches on one handle: the fused workspace (batch_lane, batch_plan: "kept while (k, n) fit") serves 5 vectors, then 2 in the same
# workspace, is rebuilt for n = 100 and again for n = 3000, grows to 8 and serves 2 again; a single MSM over the whole handle runs
# between every two batch calls. The rows of call 3 are empty, one huge bucket and dense.
BATCH_CALLS = [(5, 3000), (2, 3000), (5, 100), (3, 3000), (8, 3000), (2, 3000)]
ROW_KINDS = ["U", "BITS", "BYTE", "Z", "EQ", "TOP", "NEG", "ONE"]
# on a handle without a table, vectors this short go to its side table (16384 bases); two more calls reach the handle's own lane
LONG_BATCH_CALLS = [(3, 17000), (2, 17000)]


def _batch_rows(call, k, n, c):
    kinds = ["Z", "BITS", "U"] if call == 3 else [ROW_KINDS[(3 * call + i) % len(ROW_KINDS)] for i in range(k)]
    return [W.vector(kind, n, c, seed=7000 + 10 * call + i) for i, kind in enumerate(kinds)]


@pytest.mark.parametrize("leg,cfg,env", [("fused", {}, {}), ("unfused", {}, {"ZG_MSM_BATCH_FUSE": "0"}), ("one-proof key", {"expected_uses": 2}, {}),
                                         ("one-proof key, a reduction per row", {"expected_uses": 2}, {"ZG_MSM_ROWS_SHARED_TAIL": "0"})],
                         ids=["fused", "unfused", "uses2", "uses2-rows-apart"])
def test_batches_on_one_handle(zl, gm, leg, cfg, env, monkeypatch):
    """fused: one launch set per call in batch_lane. unfused: a launch set per vector, rotating over the six lanes and four streams. On the
    key planned for two uses (13-bit windows, no table, one lane) the short vectors fuse on the side table and the long ones run one
    after the other on the handle's lane; ZG_MSM_ROWS_SHARED_TAIL does not change that (see the module docstring) and is run to show it."""
    N = 20000
    c = 13 if cfg else 10
    conf = dict(cfg=cfg, env=env, plan=dict(c=c, G=20 if cfg else 1))
    prep = _prepare(gm, N, c)
    for k in ("ZG_MSM_BATCH_FUSE", "ZG_MSM_ROWS_SHARED_TAIL"):
        monkeypatch.delenv(k, raising=False)
    b = _upload(zl, monkeypatch, conf, prep["xy"])
    ks = W.base_multipliers(N)
    bad = []
    try:
        calls = BATCH_CALLS + (LONG_BATCH_CALLS if cfg else [])
        for call, (k, n) in enumerate(calls):
            rows = _batch_rows(call, k, n, c)
            xy, inf = b.msm_batch([W.fr_mont(r[3]) for r in rows], n=n)
            for i, r in enumerate(rows):
                want = W.result_record(W.closed_form(ks, r))
                if inf[i] != want[8] or not np.array_equal(xy[i], want[:8]):
                    bad.append((leg, f"call {call}: k={k} n={n}", f"row {i} ({r[0]})"))
            j = call % 2  # U, then Z, between the batch calls
            got, ginf = b.msm(prep["sc"][j])
            if ginf != prep["want"][j][8] or not np.array_equal(got, prep["want"][j][:8]):
                bad.append((leg, f"single MSM {prep['wls'][j][0]} after call {call}"))
    finally:
        b.free()
    assert not bad, bad


_long_level_openings = {}


@pytest.mark.parametrize("window_bits,shared", [(15, "1"), (15, "0"), (0, "1")], ids=["shared-tail", "rows-apart", "fused-rows"])
def test_rows_of_long_levels_on_a_key_without_a_table(zl, ob, gm, window_bits, shared, monkeypatch):
    """20000 bases planned for two uses (no table: one bucket set per window), openings of 2^17, 2^18 and 2^17 evaluations. Levels of more
    than 16384 entries are committed as the rows of one matrix: two rows (20000, 20000), then three (a 0 / 1 polynomial), then two again
    in buffers sized for three that last held other sums. With 15-bit windows (the plan of 2^19 bases and up) 17 x 2^14 buckets a row
    are too many to fuse, and the rows go through msm_rows_shared_tail: d_rows_buckets / d_rows_bits / d_rows_rg grow with rows_cap from 2
    to 3 and then serve 2 (ZG_MSM_ROWS_SHARED_TAIL=0: a reduction per row on the handle's one lane instead). With the automatic 13-bit
    windows up to four rows fuse into one two-pass launch set: batch_lane is rebuilt for three rows and re-planned `within` for two.
    Each opening against the oracle's; the third repeats the first one's inputs, so the oracle runs twice, once for all cases."""
    from zolt_amd import api
    for k in W.SWITCHES + ("ZG_HK_FUSE_LONG", "ZG_MSM_BATCH_FUSE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ZG_MSM_ROWS_SHARED_TAIL", shared)
    n = 20000
    inf = np.zeros(n, dtype=np.uint8)
    inf[11::501] = 1
    dev = zl.Bases.upload(gm[:n], inf, window_bits=window_bits, expected_uses=2)
    assert dev.plan()[2] == 1 and dev.plan()[0] == (window_bits or 13)  # no table; both widths reduce by rows and columns (c >= 11)
    params = api.HyperKZG.SetupParams(gm[:n], inf, dev=dev)
    zero = np.zeros(4, dtype=np.uint64)
    bits = ob.f_from_u64(ob.FR, np.random.default_rng(18).integers(0, 2, size=1 << 18).astype(np.uint64))
    inputs = {17: (ob.f_to_mont(ob.FR, U.random_raw256(8917, 1 << 17)), ob.f_to_mont(ob.FR, U.random_raw256(8918, 17))),
              18: (bits, ob.f_to_mont(ob.FR, U.random_raw256(8919, 18)))}
    if not _long_level_openings:
        _long_level_openings.update({v: ob.hyperkzg_open(gm[:n], inf, ev, pt, zero) for v, (ev, pt) in inputs.items()})
    want = _long_level_openings
    bad = []
    try:
        for step, v in enumerate([17, 18, 17]):
            quotients, final = api.HyperKZG.open(params, *inputs[v], zero)
            wq, wqi, wfin = want[v]
            if not np.array_equal(final, wfin) or len(quotients) != v:
                bad.append((step, v, "final evaluation"))
            bad += [(step, v, f"quotient {i}") for i, (q, qi) in enumerate(quotients) if qi != wqi[i] or not np.array_equal(q, wq[i])]
    finally:
        params.deinit()
    assert not bad, bad


def test_hyperkzg_opens_on_one_key(zl, ob):
    """One key serves a long skewed opening (13 variables, 0 / 1 evaluations), a short one (5), a long uniform one (13) and a middle one
    (9): its handle and fused workspace take long, short, skewed and uniform levels in turn. Each against the oracle's open."""
    from zolt_amd import api
    params = api.HyperKZG.setup(8192)
    wsrs, winf = ob.hyperkzg_setup(8192)
    assert np.array_equal(params.powers_of_tau_g1, wsrs) and np.array_equal(params.infinity, winf)
    bits = ob.f_from_u64(ob.FR, np.random.default_rng(13).integers(0, 2, size=1 << 13).astype(np.uint64))
    zero = np.zeros(4, dtype=np.uint64)
    bad = []
    try:
        for step, (v, ev) in enumerate([(13, bits), (5, None), (13, None), (9, None)]):
            ev = ob.f_to_mont(ob.FR, U.random_raw256(8800 + step, 1 << v)) if ev is None else ev
            pt = ob.f_to_mont(ob.FR, U.random_raw256(8850 + step, v))
            quotients, final = api.HyperKZG.open(params, ev, pt, zero)
            wq, wqi, wfin = ob.hyperkzg_open(wsrs, winf, ev, pt, zero)
            if not np.array_equal(final, wfin) or len(quotients) != v:
                bad.append((step, v, "final evaluation"))
            bad += [(step, v, f"quotient {i}") for i, (q, qi) in enumerate(quotients) if qi != wqi[i] or not np.array_equal(q, wq[i])]
    finally:
        params.deinit()
    assert not bad, bad
