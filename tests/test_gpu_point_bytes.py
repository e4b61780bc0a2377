"""Points from bytes on the device (include/zolt_gpu.h, "Points from bytes"; zolt_amd/csrc/point_bytes.hip) against the model of
tests/point_bytes_model.py, against the host path the mirrors had before (wire.srs_g1_from_raw, wire._g1_from_le, zg_field_op), and
the two handle calls against the existing constructors over the decoded points.

    python -m pytest tests/test_gpu_point_bytes.py -m gpu -q"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dory_captured as DC
from tests import g2_model as G2
from tests import point_bytes_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]
ENCODINGS = [M.BE, M.LE, M.ARK, M.ARK_COMPRESSED]
WORDS = {M.G1: 8, M.G2_: 16}
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def zl():
    from zolt_amd import lib
    lib.init()
    return lib


def _from_bytes(zl, group, data, encoding, flags=0):
    return (zl.g1_points_from_bytes if group == M.G1 else zl.g2_points_from_bytes)(data, encoding, flags)


# ---------------------------------------------------------------- the shared reference: 1000 points a group, made and packed once
@pytest.fixture(scope="module")
def reference():
    """per group: the points, their packed arrays, their records in every encoding — never modified by a test"""
    out = {}
    for group in (M.G1, M.G2_):
        pts = M.g1_multiples(1000, 5) if group == M.G1 else M.g2_multiples(1000, 5)
        xy, inf = M.pack(group, pts)
        ident = M.pack(group, [None])
        recs = {e: [M.encode(group, e, p) for p in pts] for e in ENCODINGS}
        # the model's decode of every record is the point it was made from (what the device is then held to)
        for e in ENCODINGS:
            for k in (0, 1, 499, 999):
                assert M.decode(group, e, recs[e][k], 0 if e == M.ARK_COMPRESSED else M.CHECK) == (M.OK, pts[k])
        xy.setflags(write=False)
        out[group] = {"pts": pts, "xy": xy, "inf": inf, "ident_xy": ident[0][0], "recs": recs}
    return out


def _batch(ref, group, encoding, n):
    """n records with identities at index 0 and n - 1 -> (bytes, xy, inf)"""
    r = ref[group]
    recs = list(r["recs"][encoding][:n])
    xy, inf = r["xy"][:n].copy(), np.zeros(n, dtype=np.uint8)
    for k in {0, n - 1} if n else ():
        recs[k] = M.encode(group, encoding, None)
        xy[k], inf[k] = r["ident_xy"], 1
    return b"".join(recs), xy, inf


# ---------------------------------------------------------------- 1. sizes and layout
@pytest.mark.parametrize("encoding", ENCODINGS, ids=["be", "le", "ark", "ark_compressed"])
@pytest.mark.parametrize("group", [M.G1, M.G2_], ids=["g1", "g2"])
def test_every_size_against_the_model(zl, reference, group, encoding):
    flags = 0 if encoding == M.ARK_COMPRESSED else M.CHECK
    for n in SIZES:
        data, xy, inf = _batch(reference, group, encoding, n)
        got_xy, got_inf = _from_bytes(zl, group, data, encoding, flags)
        assert got_xy.shape == (n, WORDS[group]) and np.array_equal(got_inf, inf), (n,)
        assert np.array_equal(got_xy, xy), (n, np.flatnonzero((got_xy != xy).any(axis=1))[:4])
    # the model itself on one whole batch, decoded record by record (the reference above is its inverse)
    data, xy, inf = _batch(reference, group, encoding, 65)
    pts, bad, reason = M.decode_all(group, encoding, data, flags)
    assert bad == 65 and reason is None
    mxy, minf = M.pack(group, pts)
    assert np.array_equal(mxy, xy) and np.array_equal(minf, inf)


def test_ark_flag_bits_negatives_and_both_root_branches(zl, reference):
    """ARK records with the ignored top bits set; compressed records of P and -P, with the 0xC0 flag, with junk under an identity flag;
    the G2 points cover both branches of the Fp2 root"""
    for group in (M.G1, M.G2_):
        pts = reference[group]["pts"][:70]
        recs = [M.encode(group, M.ARK, p, top_bits=(0x40, 0x80, 0xC0)[k % 3]) for k, p in enumerate(pts)] + [M.encode(group, M.ARK, None, top_bits=0xC0)]
        xy, inf = M.pack(group, pts + [None])
        got = _from_bytes(zl, group, b"".join(recs), M.ARK, M.CHECK)
        assert np.array_equal(got[0], xy) and np.array_equal(got[1], inf)
        neg = (lambda p: (p[0], -p[1] % M.P)) if group == M.G1 else G2.neg
        recs = [M.encode(group, M.ARK_COMPRESSED, neg(p) if k & 1 else p, sign=0xC0 if k % 5 == 1 else None) for k, p in enumerate(pts)]
        recs.append(bytes([9] * (M.record_bytes(group, M.ARK_COMPRESSED) - 1)) + bytes([0x40 | 0x21]))
        want = [M.decode(group, M.ARK_COMPRESSED, r)[1] for r in recs]
        positive = M.y_is_positive if group == M.G1 else M.fp2_is_positive
        assert want[-1] is None and want[3] == neg(pts[3]) and want[0] == pts[0]
        assert want[1] in (pts[1], neg(pts[1])) and not positive(want[1][1])  # 0xC0 is not 0: the root that is not positive
        xy, inf = M.pack(group, want)
        got = _from_bytes(zl, group, b"".join(recs), M.ARK_COMPRESSED)
        assert np.array_equal(got[0], xy) and np.array_equal(got[1], inf)
    assert {"+", "-"} <= {M.fp2_sqrt_branch(M.g2_rhs(p[0])) for p in reference[M.G2_]["pts"][:70]}


def test_the_fp2_root_with_a_real_argument(zl):
    """x with Im(x^3 + b') = 0: the a1 = 0 case (dory.zig:273-286), both of its sub-cases, both signs"""
    from tests.test_point_bytes_model import _g2_x_with_real_rhs
    recs, want = [], []
    for x in _g2_x_with_real_rhs():
        y = M.fp2_sqrt(M.g2_rhs(x))
        for p in ((x, y), (x, G2.f2_neg(y))):
            recs.append(M.encode(M.G2_, M.ARK_COMPRESSED, p))
            want.append(p)
    xy, inf = M.pack(M.G2_, want)
    got = zl.g2_points_from_bytes(b"".join(recs), M.ARK_COMPRESSED)
    assert np.array_equal(got[0], xy) and not got[1].any()


# ---------------------------------------------------------------- 2. agreement with the existing path
def test_be_and_le_g1_are_the_existing_host_path_word_for_word(zl, reference):
    from zolt_amd import api
    from zolt_amd.api import wire
    _, xy, inf = _batch(reference, M.G1, M.BE, 257)
    raw = api.srs_g1_to_raw(xy, inf)
    want_xy, want_inf, trailer = api.srs_g1_from_raw(raw)
    got_xy, got_inf = zl.g1_points_from_bytes(raw[4:4 + 64 * 257], zl.POINT_BYTES_BE, zl.POINT_BYTES_CHECK)
    assert np.array_equal(got_xy, want_xy) and np.array_equal(got_inf, want_inf) and np.array_equal(want_xy, xy) and len(trailer) == 320
    data, xy, inf = _batch(reference, M.G1, M.LE, 257)
    want_xy, want_inf = wire._g1_from_le(data, 257)
    got_xy, got_inf = zl.g1_points_from_bytes(data, zl.POINT_BYTES_LE, zl.POINT_BYTES_CHECK)
    assert np.array_equal(got_xy, want_xy) and np.array_equal(got_inf, want_inf)


def test_a_coordinate_above_p_is_to_mont_of_zg_field_op(zl):
    """random 256-bit coordinates (nearly all >= p, none on a curve, no check asked for)"""
    rng = np.random.default_rng(11)
    n = 130
    raw = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    raw[0, :] = 0xFF
    want = zl.field_op(zl.FP, zl.OP_TO_MONT, np.ascontiguousarray(raw).view(np.uint64).reshape(2 * n, 4)).reshape(n, 8)
    got = zl.g1_points_from_bytes(raw, zl.POINT_BYTES_LE)
    assert np.array_equal(got[0], want) and not got[1].any()
    be = np.ascontiguousarray(raw.reshape(n, 2, 32)[:, :, ::-1])
    assert np.array_equal(zl.g1_points_from_bytes(be, zl.POINT_BYTES_BE)[0], want)
    # ARK clears two bits of the last byte first
    masked = raw.copy()
    masked[:, 63] &= 0x3F
    want_ark = zl.field_op(zl.FP, zl.OP_TO_MONT, np.ascontiguousarray(masked).view(np.uint64).reshape(2 * n, 4)).reshape(n, 8)
    assert np.array_equal(zl.g1_points_from_bytes(raw, zl.POINT_BYTES_ARK)[0], want_ark)
    # G2: LE in file order; BE stores c1 before c0
    raw2 = rng.integers(0, 256, size=(n, 4, 32), dtype=np.uint8)
    want2 = zl.field_op(zl.FP, zl.OP_TO_MONT, np.ascontiguousarray(raw2).view(np.uint64).reshape(4 * n, 4)).reshape(n, 16)
    assert np.array_equal(zl.g2_points_from_bytes(raw2, zl.POINT_BYTES_LE)[0], want2)
    be2 = np.ascontiguousarray(raw2[:, [1, 0, 3, 2], ::-1])
    assert np.array_equal(zl.g2_points_from_bytes(be2, zl.POINT_BYTES_BE)[0], want2)


# ---------------------------------------------------------------- 3. bad records
def _raw_call(zl, group, data, encoding, flags):
    """the C call with sentinel-filled outputs -> (rc, first_bad, outputs untouched, error text)"""
    n = len(data) // M.record_bytes(group, encoding)
    a = np.frombuffer(data, dtype=np.uint8)
    xy = np.full((n, WORDS[group]), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    inf = np.full(n, SENTINEL, dtype=np.uint8)
    bad = C.c_size_t(12345)
    fn = zl._lib.zg_g1_points_from_bytes if group == M.G1 else zl._lib.zg_g2_points_from_bytes
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = fn(p(a), n, encoding, flags, p(xy), p(inf), C.byref(bad))
    return rc, bad.value, bool((xy == 0xA5A5A5A5A5A5A5A5).all() and (inf == SENTINEL).all()), zl.last_error()


def _off_curve(ref, group, encoding):
    pts = ref[group]["pts"]
    return M.encode(group, encoding, (pts[0][0], pts[1][1]))


def _no_root(group):
    for v in range(1, 60):
        x = v if group == M.G1 else (v, 1)
        rhs = M.g1_rhs(x) if group == M.G1 else M.g2_rhs(x)
        if (M.fp_sqrt(rhs) if group == M.G1 else M.fp2_sqrt(rhs)) is None:
            return M.encode(group, M.ARK_COMPRESSED, (x, 0 if group == M.G1 else (0, 0)), sign=0)
    raise AssertionError


@pytest.mark.parametrize("group", [M.G1, M.G2_], ids=["g1", "g2"])
def test_bad_records_are_reported_by_smallest_index_and_nothing_is_written(zl, reference, group):
    n = 300
    for encoding, reason, flags in ((M.BE, "PointNotOnCurve", M.CHECK), (M.LE, "PointNotOnCurve", M.CHECK), (M.ARK, "PointNotOnCurve", M.CHECK),
                                    (M.ARK_COMPRESSED, "DecompressionFailed", 0)):
        good = list(reference[group]["recs"][encoding][:n])
        bad_rec = _no_root(group) if encoding == M.ARK_COMPRESSED else _off_curve(reference, group, encoding)
        assert M.decode(group, encoding, bad_rec, flags)[0] != M.OK
        for where in ((0,), (n - 1,), (200, 77), (64, 63, 299)):
            recs = list(good)
            for k in where:
                recs[k] = bad_rec
            data = b"".join(recs)
            assert M.decode_all(group, encoding, data, flags)[1:] == (min(where), reason)
            rc, first_bad, untouched, text = _raw_call(zl, group, data, encoding, flags)
            assert rc == zl.ERR_INVALID and first_bad == min(where) and untouched, (encoding, where, rc, first_bad)
            assert reason in text and f"record {min(where)}:" in text, text
            with pytest.raises(zl.PointBytesError) as err:
                _from_bytes(zl, group, data, encoding, flags)
            assert err.value.first_bad == min(where) and err.value.reason == reason and err.value.code == zl.ERR_INVALID
            # the library stays usable: the next call succeeds
            rc, first_bad, untouched, _ = _raw_call(zl, group, b"".join(good), encoding, flags)
            assert rc == zl.OK and first_bad == n and not untouched
        if encoding != M.ARK_COMPRESSED:  # without the flag the same record is just a point
            recs = list(good)
            recs[5] = bad_rec
            got = _from_bytes(zl, group, b"".join(recs), encoding, 0)
            assert np.array_equal(np.delete(got[0], 5, axis=0), np.delete(reference[group]["xy"][:n], 5, axis=0))


def test_bad_records_make_no_handle(zl, reference):
    n = 300
    recs = list(reference[M.G1]["recs"][M.LE][:n])
    recs[123] = recs[7][:32] + recs[8][32:]
    h, bad = C.c_void_p(), C.c_size_t(999)
    a = np.frombuffer(b"".join(recs), dtype=np.uint8)
    rc = zl._lib.zg_g1_bases_from_bytes(a.ctypes.data_as(C.c_void_p), n, M.LE, M.CHECK, None, C.byref(h), C.byref(bad))
    assert rc == zl.ERR_INVALID and h.value is None and bad.value == 123 and "record 123: PointNotOnCurve" in zl.last_error()
    with pytest.raises(zl.PointBytesError):
        zl.bases_from_bytes(a, M.LE, M.CHECK)
    b = zl.bases_from_bytes(b"".join(reference[M.G1]["recs"][M.LE][:n]), M.LE, M.CHECK)
    assert b.n == n
    b.free()
    # the key: a bad G2 record is reported behind the G1 records
    g1 = b"".join(reference[M.G1]["recs"][M.ARK_COMPRESSED][:16])
    g2 = list(reference[M.G2_]["recs"][M.ARK_COMPRESSED][:8])
    g2[3] = _no_root(M.G2_)
    with pytest.raises(zl.PointBytesError) as err:
        zl.DoryKey.from_bytes(g1, M.ARK_COMPRESSED, b"".join(g2), M.ARK_COMPRESSED)
    assert err.value.first_bad == 16 + 3 and err.value.reason == "DecompressionFailed"
    g1b = list(reference[M.G1]["recs"][M.ARK_COMPRESSED][:16])
    g1b[9] = _no_root(M.G1)
    with pytest.raises(zl.PointBytesError) as err:
        zl.DoryKey.from_bytes(b"".join(g1b), M.ARK_COMPRESSED, b"".join(g2), M.ARK_COMPRESSED)
    assert err.value.first_bad == 9
    key = zl.DoryKey.from_bytes(g1, M.ARK_COMPRESSED, b"".join(reference[M.G2_]["recs"][M.ARK_COMPRESSED][:8]), M.ARK_COMPRESSED)
    assert key.lens() == (16, 8)
    key.free()


# ---------------------------------------------------------------- 4. handle equivalence
def _le_bytes(zl, xy, inf):
    """Montgomery points -> LE / ARK records (identities all zero)"""
    xy = np.ascontiguousarray(xy, dtype=np.uint64)
    canon = zl.field_op(zl.FP, zl.OP_FROM_MONT, xy.reshape(-1, 4)).reshape(xy.shape)
    canon[np.asarray(inf) == 1] = 0
    return canon.tobytes()


@pytest.mark.parametrize("n", [257, 4097])
def test_bases_from_bytes_is_bases_upload_over_the_decoded_points(zl, n):
    from zolt_amd import api
    rng = np.random.default_rng(n)
    scalars = G2.fr_pack([int(v) for v in rng.integers(1, 1 << 62, size=n)])
    xy, inf = zl.g1_fixed_base_mul_batch(api.generator(), scalars)
    xy[n // 2], inf[n // 2] = 0, 1
    data = _le_bytes(zl, xy, inf)
    dxy, dinf = zl.g1_points_from_bytes(data, zl.POINT_BYTES_LE, zl.POINT_BYTES_CHECK)
    assert np.array_equal(dxy, xy) and np.array_equal(dinf, inf)
    sc = G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(n)])
    for cfg in (dict(), dict(precompute_levels=1, expected_uses=1)):
        a = zl.bases_from_bytes(data, zl.POINT_BYTES_LE, zl.POINT_BYTES_CHECK, **cfg)
        b = zl.Bases.upload(dxy, dinf, **cfg)
        try:
            assert zl._lib.zg_g1_bases_len(a._h) == zl._lib.zg_g1_bases_len(b._h) == n and a.plan() == b.plan() and a.table_bytes() == b.table_bytes()
            ra, rb = a.msm(sc), b.msm(sc)
            assert np.array_equal(ra[0], rb[0]) and ra[1] == rb[1] == 0
        finally:
            a.free()
            b.free()


def _or_code(zl, fn):
    try:
        return fn()
    except zl.ZgError as e:
        return ("error", e.code)


def _same(a, b):
    if isinstance(a, tuple) and a and isinstance(a[0], str):
        return a == b
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("compressed", [False, True], ids=["ark", "ark_compressed"])
@pytest.mark.parametrize("n_g1,n_g2", [(16, 8), (64, 64)])
def test_dory_key_from_bytes_is_dory_key_create_over_the_decoded_points(zl, n_g1, n_g2, compressed):
    from zolt_amd import api
    from tests import dory_open_key_model as K
    rng = np.random.default_rng(100 * n_g1 + n_g2)
    s1 = G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(n_g1)])
    s2 = G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(n_g2)])
    g1 = zl.g1_fixed_base_mul_batch(api.generator(), s1)
    g2 = zl.g2_fixed_base_mul_batch(api.g2_generator(), s2)
    g1[0][5], g1[1][5] = 0, 1  # an identity generator in either vector
    ident2 = M.pack(M.G2_, [None])[0][0]
    g2[0][n_g2 - 1], g2[1][n_g2 - 1] = ident2, 1
    if compressed:
        enc = zl.POINT_BYTES_ARK_COMPRESSED
        b1 = b"".join(api.compressG1(g1[0][i], int(g1[1][i])) for i in range(n_g1))
        b2 = b"".join(api.compressG2(g2[0][i], int(g2[1][i])) for i in range(n_g2))
    else:
        enc = zl.POINT_BYTES_ARK
        b1, b2 = _le_bytes(zl, g1[0], g1[1]), _le_bytes(zl, g2[0], g2[1])
    d1, d2 = zl.g1_points_from_bytes(b1, enc), zl.g2_points_from_bytes(b2, enc)
    assert np.array_equal(d1[0], g1[0]) and np.array_equal(d1[1], g1[1]) and np.array_equal(d2[0], g2[0]) and np.array_equal(d2[1], g2[1])
    ka = zl.DoryKey.from_bytes(b1, enc, b2, enc)
    kb = zl.DoryKey.create(d1, d2)
    try:
        assert ka.lens() == kb.lens() == (n_g1, n_g2)
        assert np.array_equal(ka.g1_0[0], kb.g1_0[0]) and ka.g1_0[1] == kb.g1_0[1] and np.array_equal(ka.g2_0[0], kb.g2_0[0]) and ka.g2_0[1] == kb.g2_0[1]
        nu = sigma = 3
        evals = G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(1 << (nu + sigma))])
        column = rng.integers(0, 1 << 63, size=1 << (nu + sigma), dtype=np.uint64)
        polys = [(zl.DORY_POLY_FR, evals, None, 0, 0), (zl.DORY_POLY_CHUNK64, column, None, 4, 4)]
        ca, cb = zl.dory_commit_batch(ka, polys, want_rows=True), zl.dory_commit_batch(kb, polys, want_rows=True)
        assert _same(ca, cb)
        assert _same(_or_code(zl, lambda: zl.dory_verifier_setup(ka)), _or_code(zl, lambda: zl.dory_verifier_setup(kb)))
        rows = ca[1][0]
        v, right, left = (G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(1 << m)]) for m in (sigma, sigma, nu))
        words = K.challenge_words(K.open_challenges(sigma)).reshape(-1, 4)
        recs = []
        for key in (ka, kb):
            ses = zl.DoryOpenSession.begin_key(key, rows, v, right, left, nu, sigma)
            try:
                recs.append((ses.vmv,) + tuple(ses.run(words)))
            finally:
                ses.close()
        assert _same(recs[0], recs[1])
    finally:
        ka.free()
        kb.free()


# ---------------------------------------------------------------- 5. the captured fixtures on the device
def test_captured_points_decompress_on_the_device_and_pair_to_chi_0(zl):
    with open(os.path.join(GOLDEN, "dory_open_captured.bin"), "rb") as f:
        pts = M.captured_open_points(f.read())
    cap = DC.parse()
    pts += [(M.G1, "g1_0", cap.g1_0_bytes), (M.G2_, "g2_0", cap.g2_0_bytes), (M.G1, "h1", cap.h1_bytes), (M.G2_, "h2", cap.h2_bytes)]
    got = {}
    for group in (M.G1, M.G2_):
        recs = [b for g, _, b in pts if g == group]
        want = M.pack(group, [M.decode(group, M.ARK_COMPRESSED, b)[1] for b in recs])
        got[group] = _from_bytes(zl, group, b"".join(recs), M.ARK_COMPRESSED)
        assert np.array_equal(got[group][0], want[0]) and np.array_equal(got[group][1], want[1])
    g1_0 = zl.g1_points_from_bytes(cap.g1_0_bytes, zl.POINT_BYTES_ARK_COMPRESSED)
    g2_0 = zl.g2_points_from_bytes(cap.g2_0_bytes, zl.POINT_BYTES_ARK_COMPRESSED)
    assert np.array_equal(zl.pairing_batch(g1_0[0], g1_0[1], g2_0[0], g2_0[1])[0], cap.chi_words[0])


# ---------------------------------------------------------------- 6. the mirrors
def _be_g2(zl, xy):
    canon = zl.field_op(zl.FP, zl.OP_FROM_MONT, np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4)).reshape(-1, 4, 4)
    return np.ascontiguousarray(canon.view(np.uint8).reshape(-1, 4, 32)[:, [1, 0, 3, 2], ::-1]).tobytes()


def test_dory_load_from_file(zl, tmp_path):
    from zolt_amd import api
    params = api.Dory.setup(5)  # sigma = 3, nu = 2: 8 G1 and 4 G2 generators
    g1, g2 = params.g1_vec, params.g2_vec
    blob = _dory_file(zl, params, 5)
    path = tmp_path / "dory.srs"
    path.write_bytes(blob)
    want = zl.DoryKey.create(g1, g2)
    evals = G2.fr_pack(list(range(1, 33)))
    for src in (blob, str(path)):
        key = api.Dory.loadFromFile(src)
        assert (key.sigma, key.nu, key.max_num_vars) == (3, 2, 5) and key.lens() == (8, 4)
        assert _same(zl.dory_commit_batch(key, [(zl.DORY_POLY_FR, evals, None, 0, 0)], want_rows=True),
                     zl.dory_commit_batch(want, [(zl.DORY_POLY_FR, evals, None, 0, 0)], want_rows=True))
        key.free()
    want.free()
    params.deinit()
    d1 = api.decompressG1([api.compressG1(g1[0][i], int(g1[1][i])) for i in range(8)])
    d2 = api.decompressG2([api.compressG2(g2[0][i], int(g2[1][i])) for i in range(4)])
    assert np.array_equal(d1[0], g1[0]) and np.array_equal(d2[0], g2[0]) and not d1[1].any() and not d2[1].any()


def _raw_file(zl, reference, n):
    from zolt_amd import api
    _, xy, inf = _batch(reference, M.G1, M.BE, n)
    trailer = _be_g2(zl, reference[M.G2_]["xy"][3]) + api.commitment_to_bytes(api.generator(), 0) + _be_g2(zl, api.g2_generator())
    return api.srs_g1_to_raw(xy, inf, trailer)


def _ptau_file(reference):
    """a hand-built ptau: power 3 -> 15 of 17 TauG1, 9 TauG2, 8 alpha, 6 of at most 8 beta, one beta_g2"""
    g1le, g2le = reference[M.G1]["recs"][M.LE], reference[M.G2_]["recs"][M.LE]

    def section(typ, payload):
        return typ.to_bytes(4, "little") + len(payload).to_bytes(8, "little") + payload

    header = (32).to_bytes(4, "little") + M.P.to_bytes(32, "little") + (3).to_bytes(4, "little") + (10).to_bytes(4, "little")
    return (b"ptau" + (1).to_bytes(4, "little") + (6).to_bytes(4, "little") + section(1, header) + section(2, b"".join(g1le[:17])) + section(3, b"".join(g2le[:9]))
            + section(4, b"".join(g1le[20:28])) + section(5, b"".join(g1le[30:36])) + section(6, g2le[40]))


def _dory_file(zl, params, max_num_vars):
    g1, g2 = params.g1_vec, params.g2_vec
    return (b"JOLT_DORY_SRS_V1" + max_num_vars.to_bytes(8, "little") + g1[0].shape[0].to_bytes(8, "little") + _le_bytes(zl, g1[0], g1[1])
            + g2[0].shape[0].to_bytes(8, "little") + _le_bytes(zl, g2[0], g2[1]) + bytes([0x5A] * 192))


def test_srs_from_raw_and_from_ptau(zl, reference):
    from zolt_amd import api
    rng = np.random.default_rng(5)
    n = 300
    g2pts = reference[M.G2_]["xy"]
    raw = _raw_file(zl, reference, n)
    srs = api.srs_from_raw(raw)
    sc = G2.fr_pack([int.from_bytes(rng.bytes(32), "little") % G2.R for _ in range(n)])
    old = zl.Bases.upload(*api.srs_g1_from_raw(raw)[:2])
    a, b = srs["bases"].msm(sc), old.msm(sc)
    assert srs["max_degree"] == n and np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert np.array_equal(srs["tau_g2"][0], g2pts[3]) and np.array_equal(srs["g1"][0], api.generator()) and np.array_equal(srs["g2"][0], api.g2_generator())
    assert (srs["tau_g2"][1], srs["g1"][1], srs["g2"][1]) == (0, 0, 0)
    srs["bases"].free()
    old.free()
    broken = bytearray(raw)
    broken[4 + 64 * 40 + 63] ^= 1
    with pytest.raises(api.SRSError, match="PointNotOnCurve"):
        api.srs_from_raw(bytes(broken))
    with pytest.raises(api.SRSError, match="TruncatedData"):
        api.srs_from_raw(raw[:-1])
    ptau = _ptau_file(reference)
    got = api.srs_from_ptau(ptau)
    want = api.srs_g1_from_ptau(ptau)
    assert (got["power"], got["ceremony_power"], got["n_g1"]) == (3, 10, 15) == (want["power"], want["ceremony_power"], want["powers_of_tau_g1"][0].shape[0])
    old = zl.Bases.upload(*want["powers_of_tau_g1"])
    a, b = got["bases"].msm(sc[:15]), old.msm(sc[:15])
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    got["bases"].free()
    old.free()
    for name in ("alpha_tau_g1", "beta_tau_g1"):
        assert np.array_equal(got[name][0], want[name][0]) and np.array_equal(got[name][1], want[name][1])
    assert got["beta_tau_g1"][0].shape[0] == 6
    assert np.array_equal(got["powers_of_tau_g2"][0], g2pts[:9]) and np.array_equal(got["beta_g2"][0], g2pts[40]) and got["beta_g2"][1] == 0


def _hex(words):
    return "".join("%016x" % int(w) for w in np.asarray(words, dtype=np.uint64).reshape(-1))


def test_cpp_mirror_prints_what_the_python_mirror_computes(zl, reference, tmp_path):
    """tests/cpp/test_point_bytes_mirror.cpp over the same five files: wire::srsFromRaw, wire::srsFromPtau, Dory::loadFromFile,
    wire::decompressG1 / decompressG2, and the error names"""
    import subprocess
    from zolt_amd import api
    exe = str(tmp_path / "test_point_bytes_mirror")
    libdir = os.path.join(ROOT, "zolt_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zolt_amd", "host"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_point_bytes_mirror.cpp"), "-L" + libdir, "-lzolt_gpu", "-lpthread", "-ldl",
                           "-Wl,-rpath," + libdir])
    params = api.Dory.setup(5)
    files = {"raw": _raw_file(zl, reference, 70), "ptau": _ptau_file(reference), "dory": _dory_file(zl, params, 5),
             "g1c": b"".join(reference[M.G1]["recs"][M.ARK_COMPRESSED][:5]) + M.encode(M.G1, M.ARK_COMPRESSED, None),
             "g2c": b"".join(reference[M.G2_]["recs"][M.ARK_COMPRESSED][:5]) + M.encode(M.G2_, M.ARK_COMPRESSED, None)}
    params.deinit()
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    res = subprocess.run([exe] + [str(tmp_path / name) for name in files], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    counting = lambda n: np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)  # noqa: E731
    point = lambda r: _hex(r[0]) + str(int(r[1]))  # noqa: E731
    srs = api.srs_from_raw(files["raw"])
    assert lines[0] == "raw 70 " + point(srs["bases"].msm_u64(counting(70))) + _hex(srs["tau_g2"][0]) + point(srs["g1"]) + _hex(srs["g2"][0])
    srs["bases"].free()
    pt = api.srs_from_ptau(files["ptau"])
    assert lines[1] == ("ptau 3 10 15 " + point(pt["bases"].msm_u64(counting(15))) + _hex(pt["powers_of_tau_g2"][0]) + _hex(pt["alpha_tau_g1"][0])
                        + _hex(pt["beta_tau_g1"][0]) + _hex(pt["beta_g2"][0]))
    pt["bases"].free()
    key = api.Dory.loadFromFile(files["dory"])
    assert lines[2] == "dory 3 2 " + _hex(zl.dory_commit_batch(key, [(zl.DORY_POLY_U64, counting(32), None, 0, 0)])[0])
    key.free()
    d1, d2 = zl.g1_points_from_bytes(files["g1c"], zl.POINT_BYTES_ARK_COMPRESSED), zl.g2_points_from_bytes(files["g2c"], zl.POINT_BYTES_ARK_COMPRESSED)
    assert lines[3] == "points " + _hex(d1[0]) + _hex(d2[0]) + "000001" * 2
    assert lines[4:] == ["bad PointNotOnCurve", "short TruncatedData"]
