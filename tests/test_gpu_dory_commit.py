"""Dory commitments on the device (zg_dory_key_*, zg_dory_commit_batch[_dev]: lib.DoryKey, api.Dory.setup / batchCommit) against
tests/dory_commit_model.py. Keys come from setup, whose generators have known discrete logarithms, so an expected commitment is the closed
form e(G1, G2)^(sum_r b_r sum_c a_c M[r][c]): one power of the model's pairing of the generators per value, whatever the size. Row
commitments are compared as points ((row exponent) G1). Everything is compared as canonical integers or bit for bit."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import dory_commit_model as DM
from tests import g2_model as G2
from tests import pairing_model as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = DM.R
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


class Key:
    """a setup key on the device with the scalars it was made from"""

    def __init__(self, zl, max_num_vars, a=None, b=None):
        from zolt_amd import api
        if a is None:
            self.sigma, self.nu, self.a, self.b = DM.setup_scalars(max_num_vars)
            self.params = api.Dory.setup(max_num_vars)
        else:
            self.a, self.b = [x % R for x in a], [x % R for x in b]
            g1 = zl.g1_fixed_base_mul_batch(api.generator(), DM.fr_pack(self.a))
            g2 = zl.g2_fixed_base_mul_batch(api.g2_generator(), DM.fr_pack(self.b)) if b else (np.zeros((0, 16), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
            self.params = api.Dory.SetupParams(g1, g2, 0, 0)
        self.dev = api.Dory.key(self.params)


@pytest.fixture(scope="module")
def keys(zl):
    made = {}

    def get(max_num_vars):
        if max_num_vars not in made:
            made[max_num_vars] = Key(zl, max_num_vars)
        return made[max_num_vars]

    yield get
    for k in made.values():
        k.dev.free()
        k.params.deinit()


def _gt(exp):
    return PM.gt_pack([PM.power(DM.e_gen(), exp % R)])[0]


GT_ONE = PM.gt_pack([PM.ONE])[0]


def _poly(rng, kind, n, zero_share=0.0):
    """(what batchCommit takes, the model's values) for n entries of one kind"""
    def sparse(v):
        return 0 if rng.random() < zero_share else v
    if kind == "fr":
        vals = [sparse(rng.randrange(R)) for _ in range(n)]
        return ("fr", DM.fr_pack(vals)), DM.values_fr(vals)
    if kind == "u64":
        words = [sparse(rng.getrandbits(64)) for _ in range(n)]
        signs = [rng.getrandbits(1) for _ in range(n)]
        return ("u64", np.array(words, dtype=np.uint64), np.array(signs, dtype=np.uint8)), DM.values_u64(words, signs)
    if kind == "chunk64":
        col = [sparse(rng.getrandbits(64)) for _ in range(n)]
        shift, bits = rng.choice([(0, 4), (60, 4), (56, 8), (13, 7), (63, 1), (28, 4)])
        return ("chunk", np.array(col, dtype=np.uint64), shift, bits), DM.values_chunk(col, shift, bits)
    col = [sparse(rng.getrandbits(128)) for _ in range(n)]
    shift, bits = rng.choice([(124, 4), (60, 8), (62, 4), (0, 4), (120, 8), (64, 4), (57, 8)])
    return ("chunk", DM.u128_pack(col), shift, bits), DM.values_chunk(col, shift, bits)


KINDS = ("fr", "u64", "chunk64", "chunk128")


def _check_batch(key, polys, values, rows_too=True):
    """the batch against the closed form, value by value; the rows as points"""
    from zolt_amd import api
    gt, rows = api.Dory.batchCommit(key.dev, polys, want_rows=True)
    assert gt.shape == (len(polys), 48) and len(rows) == len(polys)
    for j, vals in enumerate(values):
        assert np.array_equal(gt[j], _gt(DM.exponent(key.a, key.b, vals))), j
        want = DM.row_exponents(key.a, vals)
        assert rows[j][0].shape == (len(want), 8) and rows[j][1].shape == (len(want),), j
        if rows_too:
            assert PM.g1_unpack(*rows[j]) == [PM.g1_mul(PM.G1_GEN, e) if e else None for e in want], j
        else:
            assert [int(f) for f in rows[j][1]] == [0 if e else 1 for e in want], j
        assert not rows[j][0][rows[j][1] == 1].any(), j  # an identity is written x = y = 0
    return gt, rows


# ---------------------------------------------------------------- 1. setup
@pytest.mark.parametrize("max_num_vars", [3, 6, 13])
def test_setup_keys_are_the_models_points(zl, keys, max_num_vars):
    from zolt_amd import api
    key = keys(max_num_vars)
    sigma, nu, a, b = api.Dory.setupScalars(max_num_vars)
    assert (sigma, nu, a, b) == DM.setup_scalars(max_num_vars) and (key.params.sigma, key.params.nu) == (sigma, nu)
    assert (sigma, nu) == ((max_num_vars + 1) // 2, max_num_vars - (max_num_vars + 1) // 2)
    g1, g2 = DM.setup(max_num_vars)
    assert PM.g1_unpack(*key.params.g1_vec) == g1 and G2.unpack(*key.params.g2_vec) == g2
    assert key.dev.lens() == (1 << sigma, 1 << nu) and key.dev.table_bytes() == 255 * 64 << sigma


# ---------------------------------------------------------------- 2. every kind at every layout
@pytest.mark.parametrize("num_vars", [1, 2, 3, 6])
def test_every_kind_at_small_layouts(zl, keys, num_vars):
    rng = random.Random(100 + num_vars)
    key = keys(6)
    made = [_poly(rng, kind, 1 << num_vars) for kind in KINDS]
    _check_batch(key, [m[0] for m in made], [m[1] for m in made])


@pytest.mark.parametrize("num_vars", [13, 14])
def test_every_kind_where_a_lane_takes_several_columns(zl, keys, num_vars):
    """sigma = 7: 128 columns, 8 lanes of 16 columns per row, 64 or 128 rows — several waves per virtual polynomial; a uniform and a
    mostly-zero digit distribution"""
    rng = random.Random(200 + num_vars)
    key = keys(14)
    made = [_poly(rng, kind, 1 << num_vars, zero_share) for kind in KINDS for zero_share in ((0.0, 0.9) if kind != "fr" else (0.0,))]
    _check_batch(key, [m[0] for m in made], [m[1] for m in made], rows_too=False)
    # the rows of one polynomial of each integer kind as points, four rows each
    from zolt_amd import api
    for m in made[1:6:2]:
        _, rows = api.Dory.batchCommit(key.dev, [m[0]], want_rows=True)
        want = DM.row_exponents(key.a, m[1])
        pick = [0, 1, len(want) // 2, len(want) - 1]
        assert PM.g1_unpack(rows[0][0][pick], rows[0][1][pick]) == [PM.g1_mul(PM.G1_GEN, want[r]) if want[r] else None for r in pick]


def test_lengths_that_are_no_power_of_two_and_the_layout_edges(zl, keys):
    """lengths 0, 1, 2, 3, 8, 11: the first 2^num_vars entries are read, a one-entry polynomial has a one-entry row, an empty one is GT one"""
    rng = random.Random(31)
    key = keys(6)
    for kind in KINDS:
        made = [_poly(rng, kind, n) for n in (0, 1, 2, 3, 8, 11)]
        gt, rows = _check_batch(key, [m[0] for m in made], [m[1] for m in made])
        assert np.array_equal(gt[0], GT_ONE) and rows[0][0].shape == (0, 8)
        assert [r[0].shape[0] for r in rows] == [0, 1, 1, 1, 2, 2]


# ---------------------------------------------------------------- 3. one batch, more than eight segments
def test_a_batch_of_eleven_equals_eleven_single_calls(zl, keys):
    from zolt_amd import api
    rng = random.Random(41)
    key = keys(14)
    spec = [("chunk128", 1 << 10), ("fr", 1 << 6), ("u64", 1 << 13), ("chunk64", 0), ("chunk64", 1 << 12), ("fr", 1 << 11), ("chunk128", 1 << 14), ("u64", 5),
            ("zero", 1 << 8), ("chunk128", 1 << 3), ("u64", 1 << 9)]
    made = [(("u64", np.zeros(n, dtype=np.uint64)), [0] * n) if kind == "zero" else _poly(rng, kind, n, 0.5 if j % 2 else 0.0) for j, (kind, n) in enumerate(spec)]
    gt, rows = api.Dory.batchCommit(key.dev, [m[0] for m in made], want_rows=True)
    assert gt.shape == (11, 48)
    for j, m in enumerate(made):
        g1, r1 = api.Dory.batchCommit(key.dev, [m[0]], want_rows=True)
        assert np.array_equal(g1[0], gt[j]) and np.array_equal(r1[0][0], rows[j][0]) and np.array_equal(r1[0][1], rows[j][1]), j
    assert np.array_equal(gt[3], GT_ONE) and np.array_equal(gt[8], GT_ONE) and rows[8][1].all() and rows[8][0].shape == (16, 8)
    for j in (0, 2, 5, 6, 7):
        assert np.array_equal(gt[j], _gt(DM.exponent(key.a, key.b, made[j][1]))), j


# ---------------------------------------------------------------- 4. value edges
def test_fr_values_at_the_top_of_the_field(zl, keys):
    """canonical values from 2^253 up to r - 1 (the MSM's top window), and Montgomery words at and above 2^254 — not canonical: the MSM
    takes them through the Montgomery reduction, value = words * 2^-256 mod r"""
    key = keys(6)
    top = [R - 1, R - 2, 1 << 253, (1 << 253) + 1, R - (1 << 64), R >> 1, 0, 1] * 8
    words = [1 << 254, (1 << 254) + 1, (1 << 255) + 5, (1 << 256) - 1, R, R + 1, 2 * R, 3 * R + 7] * 8
    raw = np.array([[(w >> (64 * i)) & M64 for i in range(4)] for w in words], dtype=np.uint64)
    inv = pow(1 << 256, -1, R)
    _check_batch(key, [("fr", DM.fr_pack(top)), ("fr", raw)], [DM.values_fr(top), [w * inv % R for w in words]])


def test_u64_byte_seven_and_negative_increments(zl, keys):
    key = keys(6)
    rng = random.Random(51)
    hi = [rng.randrange(1, 256) << 56 for _ in range(64)]
    full = [M64] * 32 + [0] * 16 + [1] * 16
    signs = [1] * 64
    inc = [rng.getrandbits(rng.choice([1, 8, 33, 64])) for _ in range(64)]
    inc_signs = [rng.getrandbits(1) for _ in range(64)]
    polys = [("u64", np.array(hi, dtype=np.uint64)), ("u64", np.array(full, dtype=np.uint64), np.array(signs, dtype=np.uint8)),
             ("u64", np.array(inc, dtype=np.uint64), np.array(inc_signs, dtype=np.uint8)), ("u64", np.zeros(64, dtype=np.uint64), np.ones(64, dtype=np.uint8))]
    gt, _ = _check_batch(key, polys, [DM.values_u64(hi), DM.values_u64(full, signs), DM.values_u64(inc, inc_signs), [0] * 64])
    assert np.array_equal(gt[3], GT_ONE)  # a zero word with the sign set is zero


# ---------------------------------------------------------------- 5. keys
def test_degenerate_keys(zl, keys):
    """every generator the same point: each addition of a row is a doubling or a general case; generators that alternate in sign with equal
    digits: rows cancel to the identity"""
    from zolt_amd import api
    rng = random.Random(61)
    b = keys(6).b
    same = Key(zl, None, a=[1] * 8, b=b)
    alt = Key(zl, None, a=[(-1) ** c for c in range(8)], b=b)
    try:
        col = [rng.getrandbits(64) for _ in range(64)]
        words = [rng.getrandbits(64) for _ in range(64)]
        polys = [("chunk", np.array(col, dtype=np.uint64), 8, 8), ("chunk", np.array([1] * 64, dtype=np.uint64), 0, 4), ("u64", np.array(words, dtype=np.uint64)),
                 ("u64", np.array([3] * 64, dtype=np.uint64), np.array([c & 1 for c in range(64)], dtype=np.uint8))]
        values = [DM.values_chunk(col, 8, 8), [1] * 64, DM.values_u64(words), DM.values_u64([3] * 64, [c & 1 for c in range(64)])]
        _, rows = _check_batch(same, polys, values)
        assert rows[3][1].all()  # 3 G - 3 G + ...: the identity met inside the sums
        pairs = [v for v in (rng.getrandbits(64) for _ in range(32)) for _ in range(2)]  # equal entries under g and -g
        polys = [("chunk", np.array(pairs, dtype=np.uint64), 4, 8), ("u64", np.array(pairs, dtype=np.uint64)), ("fr", DM.fr_pack(pairs))]
        gt, rows = _check_batch(alt, polys, [DM.values_chunk(pairs, 4, 8), DM.values_u64(pairs), DM.values_fr(pairs)])
        assert all(np.array_equal(g, GT_ONE) for g in gt) and all(r[1].all() for r in rows)
    finally:
        for k in (same, alt):
            k.dev.free()
            k.params.deinit()


def test_a_key_with_fewer_g2_generators_than_rows(zl, keys):
    rng = random.Random(71)
    full = keys(6)
    short = Key(zl, None, a=full.a, b=full.b[:3])
    none = Key(zl, None, a=full.a, b=[])
    try:
        made = [_poly(rng, kind, 64) for kind in KINDS]
        gt, _ = _check_batch(short, [m[0] for m in made], [m[1] for m in made], rows_too=False)
        assert not any(np.array_equal(g, GT_ONE) for g in gt)
        gt, _ = _check_batch(none, [m[0] for m in made], [m[1] for m in made], rows_too=False)
        assert all(np.array_equal(g, GT_ONE) for g in gt)
    finally:
        for k in (short, none):
            k.dev.free()
            k.params.deinit()


def test_a_key_with_too_few_g1_generators_is_refused_and_nothing_is_written(zl, keys):
    key = keys(3)  # 4 columns
    ok = ("chunk", np.arange(8, dtype=np.uint64), 0, 4)
    wide = ("chunk", np.arange(64, dtype=np.uint64), 0, 4)  # sigma = 3: 8 columns
    args = zl._dory_batch_args([(zl.DORY_POLY_CHUNK64, ok[1], None, 0, 4), (zl.DORY_POLY_CHUNK64, wide[1], None, 0, 4)], False)
    k, kinds, data, aux, lens, shifts, bits, keep = args
    gt = np.full((2, 48), 0xA5, dtype=np.uint64)
    rows = np.full((16, 9), 0xA5, dtype=np.uint64)
    off = np.full(3, 0xA5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = zl._lib.zg_dory_commit_batch(key.dev._h, k, p(kinds), data, aux, p(lens), p(shifts), p(bits), p(gt), p(rows), p(off))
    assert rc == zl.ERR_INVALID and (gt == 0xA5).all() and (rows == 0xA5).all() and (off == 0xA5).all()
    for bad in ((zl.DORY_POLY_CHUNK64, ok[1], None, 60, 5), (zl.DORY_POLY_CHUNK128, DM.u128_pack([1, 2]), None, 121, 8), (zl.DORY_POLY_CHUNK64, ok[1], None, 0, 9),
                (zl.DORY_POLY_CHUNK64, ok[1], None, 0, 0), (7, ok[1], None, 0, 0)):
        with pytest.raises(zl.ZgError) as err:
            zl.dory_commit_batch(key.dev, [bad])
        assert err.value.code == zl.ERR_INVALID
    from zolt_amd import api
    assert api.Dory.batchCommit(key.dev, []).shape == (0, 48)
    assert np.array_equal(api.Dory.batchCommit(key.dev, [ok])[0], _gt(DM.exponent(key.a, key.b, list(range(8)))))


# ---------------------------------------------------------------- 6. against the per-call composition, and into an opening
def test_against_the_per_call_composition_at_twelve_variables(zl, keys):
    """api.Dory.commit — zg_msm_g1_batch + zg_multi_pairing, a call per polynomial — on the widened field elements: GT and rows bit-equal"""
    from zolt_amd import api
    rng = random.Random(81)
    key = keys(12)
    evals = [rng.randrange(R) for _ in range(1 << 12)]
    col = [rng.getrandbits(128) if rng.random() < 0.7 else 0 for _ in range(1 << 12)]
    polys = [("fr", DM.fr_pack(evals)), ("chunk", DM.u128_pack(col), 62, 4)]
    gt, rows = api.Dory.batchCommit(key.dev, polys, want_rows=True)
    for j, widened in enumerate((DM.fr_pack(evals), DM.fr_pack(DM.values_chunk(col, 62, 4)))):
        want_rows = api.Dory.computeRowCommitments(key.params.g1_bases(), widened, 64)
        assert np.array_equal(rows[j][0], want_rows[0]) and np.array_equal(rows[j][1], want_rows[1]), j
        assert np.array_equal(gt[j], api.Dory.commit(key.params.g1_bases(), key.params.g2_vec, widened, 64)), j


def test_rows_of_the_batch_open_the_polynomial(zl, keys):
    """out_rows into api.Dory.openWithTranscript at (nu, sigma) = (3, 3): the proof bytes of the call that computes its own rows"""
    from zolt_amd import api
    rng = random.Random(91)
    key = keys(6)
    col = [rng.getrandbits(64) for _ in range(64)]
    evals = DM.fr_pack(DM.values_chunk(col, 20, 8))
    point = G2.fr_pack([rng.randrange(R) for _ in range(6)])
    _, rows = api.Dory.batchCommit(key.dev, [("chunk", np.array(col, dtype=np.uint64), 20, 8)], want_rows=True)
    got = api.Dory.openWithTranscript(key.params, evals, point, rows[0], api.Blake2bTranscript(b"Jolt"))
    want = api.Dory.openWithTranscript(key.params, evals, point, None, api.Blake2bTranscript(b"Jolt"))
    assert got.toBytes() == want.toBytes()


# ---------------------------------------------------------------- 7. transport
def test_a_shared_column_crosses_once_and_changes_nothing(zl, keys):
    """the reference's list from integer columns: the 32 InstructionRa chunks name one array; distinct copies give the same bytes"""
    from zolt_amd import api
    rng = random.Random(95)
    key = keys(12)
    T = 1 << 10
    lookup = DM.u128_pack([rng.getrandbits(128) if rng.random() < 0.5 else rng.getrandbits(20) for _ in range(T)])
    addr, pc = (np.array([rng.getrandbits(12) for _ in range(T)], dtype=np.uint64) for _ in range(2))
    incs = [(np.array([rng.getrandbits(40) for _ in range(T)], dtype=np.uint64), np.array([rng.getrandbits(1) for _ in range(T)], dtype=np.uint8)) for _ in range(2)]
    polys = api.Dory.traceColumnPolys(incs[0], incs[1], lookup, addr, pc, ram_d=3, bytecode_d=3)
    assert len(polys) == 2 + 32 + 3 + 3 and [p[2] for p in polys[2:34]] == [4 * (31 - j) for j in range(32)] and [p[2] for p in polys[34:]] == [8, 4, 0] * 2
    shared = api.Dory.commitTraceColumns(key.dev, incs[0], incs[1], lookup, addr, pc, ram_d=3, bytecode_d=3)
    copies = api.Dory.batchCommit(key.dev, [(p[0], p[1].copy()) + tuple(p[2:]) for p in polys])
    assert shared.shape == (40, 48) and np.array_equal(shared, copies)
    ints = [int(lo) | int(hi) << 64 for lo, hi in lookup]
    for j in (2, 17, 33):
        assert np.array_equal(shared[j], _gt(DM.exponent(key.a, key.b, DM.values_chunk(ints, polys[j][2], 4)))), j
    assert np.array_equal(shared[0], _gt(DM.exponent(key.a, key.b, DM.values_u64(incs[0][0], incs[0][1]))))
    assert np.array_equal(shared[36], _gt(DM.exponent(key.a, key.b, DM.values_chunk(addr, 0, 4))))


def test_the_device_pointer_entry_on_a_stream_of_its_own(zl, keys):
    import torch
    from zolt_amd import api
    rng = random.Random(97)
    key = keys(12)
    made = [_poly(rng, kind, n) for kind, n in (("u64", 1 << 10), ("chunk128", 1 << 12), ("fr", 1 << 8), ("chunk64", 1), ("fr", 1))]
    want, want_rows = api.Dory.batchCommit(key.dev, [m[0] for m in made], want_rows=True)
    bufs, items = [], []
    for m in made:
        p = m[0]
        d = zl.DeviceBuffer.from_host(np.ascontiguousarray(p[1]))
        bufs.append(d)
        n = p[1].shape[0]
        if p[0] == "fr":
            items.append((zl.DORY_POLY_FR, (d.ptr, n), 0, 0, 0))
        elif p[0] == "u64":
            s = zl.DeviceBuffer.from_host(p[2])
            bufs.append(s)
            items.append((zl.DORY_POLY_U64, (d.ptr, n), s.ptr, 0, 0))
        else:
            items.append((zl.DORY_POLY_CHUNK128 if p[1].ndim == 2 else zl.DORY_POLY_CHUNK64, (d.ptr, n), 0, p[2], p[3]))
    total = sum(r[0].shape[0] for r in want_rows)
    d_gt, d_rows = zl.DeviceBuffer(len(made) * 48 * 8), zl.DeviceBuffer(total * 72)
    work = torch.cuda.Stream()
    off = zl.dory_commit_batch_dev(key.dev, items, d_gt.ptr, d_rows.ptr, stream=work.cuda_stream)
    assert list(off) == list(np.cumsum([0] + [r[0].shape[0] for r in want_rows]))
    assert np.array_equal(d_gt.to_host()[:len(made) * 48].reshape(-1, 48), want)
    got_rows = d_rows.to_host()[:total * 9].reshape(-1, 9)
    assert np.array_equal(got_rows[:, :8], np.concatenate([r[0] for r in want_rows])) and np.array_equal(got_rows[:, 8] & 1, np.concatenate([r[1] for r in want_rows]))
    d_gt2 = zl.DeviceBuffer(len(made) * 48 * 8)
    zl.dory_commit_batch_dev(key.dev, items, d_gt2.ptr, 0, stream=work.cuda_stream)  # rows not wanted
    assert np.array_equal(d_gt2.to_host()[:len(made) * 48].reshape(-1, 48), want)
    for b in bufs + [d_gt, d_rows, d_gt2]:
        b.free()


def test_feature_bit_and_key_lifecycle(zl, keys):
    from zolt_amd import _abi
    assert zl.abi_features() & 64 and _abi.ZG_FEATURE_DORY_COMMIT == 64 and zl.abi_version() == (1, 11)
    assert zl._lib.zg_dory_key_free(None) == 0 and zl._lib.zg_dory_key_len(None, None, None) == zl.ERR_INVALID
    with pytest.raises(zl.ZgError) as err:
        zl.DoryKey.create((np.zeros((0, 8), dtype=np.uint64), None), (np.zeros((0, 16), dtype=np.uint64), None))
    assert err.value.code == zl.ERR_INVALID
    # an identity generator contributes nothing, to any kind
    full = keys(3)
    g1 = (full.params.g1_vec[0].copy(), np.array([0, 1, 0, 0], dtype=np.uint8))
    key = zl.DoryKey.create(g1, full.params.g2_vec)
    from zolt_amd import api
    a = [full.a[0], 0, full.a[2], full.a[3]]
    vals = list(range(1, 9))
    gt = api.Dory.batchCommit(key, [("chunk", np.array(vals, dtype=np.uint64), 0, 4), ("u64", np.array(vals, dtype=np.uint64)), ("fr", DM.fr_pack(vals))])
    key.free()
    assert all(np.array_equal(g, _gt(DM.exponent(a, full.b, vals))) for g in gt)


# ---------------------------------------------------------------- 8. the C++ mirror
def test_cpp_dory_commit_mirror(zl, keys, tmp_path):
    """tests/cpp/test_dory_commit_mirror.cpp prints zolt::Dory::setup's first generators and zolt::Dory::batchCommit's GT values for a fixed
    input; the Python mirror gives the same words"""
    from zolt_amd import api
    exe = str(tmp_path / "test_dory_commit_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dory_commit_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    got = {l.split()[0]: l.split()[1:] for l in res.stdout.splitlines()}
    key = keys(6)
    assert got["g1_0"] == [f"{int(w):x}" for w in key.params.g1_vec[0][0]] and got["g2_7"] == [f"{int(w):x}" for w in key.params.g2_vec[0][7]]
    # the same fixed input: evals[i] = 1000 + 17 i, words[i] = 3 i * 2^40 + i with every third negated, column[i] = (i * 0x9e3779b97f4a7c15) mod 2^64, shift 60
    n = 64
    words = [(3 * i << 40) + i for i in range(n)]
    signs = [1 if i % 3 == 0 else 0 for i in range(n)]
    col = [i * 0x9e3779b97f4a7c15 & M64 for i in range(n)]
    want = api.Dory.batchCommit(key.dev, [("fr", DM.fr_pack([1000 + 17 * i for i in range(n)])), ("u64", np.array(words, dtype=np.uint64), np.array(signs, dtype=np.uint8)),
                                          ("chunk", np.array(col, dtype=np.uint64), 60, 4)])
    for j in range(3):
        assert got[f"gt_{j}"] == [f"{int(w):x}" for w in want[j]], j
