"""Points from bytes without a device: the model of tests/point_bytes_model.py pinned on bytes the reference wrote (every compressed point
of tests/golden/dory_open_captured.bin and of tests/golden/dory_verifier_setup_captured.bin); the kernels' lane functions
(zolt_amd/csrc/point_bytes.hip.h) compiled for the host — once as they are, once under the address and undefined-behaviour sanitizers, a
stand-alone program — against the model; the header section, the bindings, the exports, the no-device answer and the containers' error
names.

    python -m pytest tests/test_point_bytes_model.py -q"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dory_captured as DC
from tests import dory_open_model as DOM
from tests import g2_model as G2
from tests import point_bytes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P = M.P


@pytest.fixture(scope="module")
def captured_points():
    with open(os.path.join(GOLDEN, "dory_open_captured.bin"), "rb") as f:
        pts = M.captured_open_points(f.read())
    data = DC.read()
    pos = DC.POINTS_AT
    for name, group in (("g1_0", M.G1), ("g2_0", M.G2_), ("h1", M.G1), ("h2", M.G2_)):
        size = M.record_bytes(group, M.ARK_COMPRESSED)
        pts.append((group, "vsetup." + name, data[pos:pos + size]))
        pos += size
    return pts


# ---------------------------------------------------------------- 1. the model on the reference's own bytes
def test_every_captured_point_decompresses_and_recompresses(captured_points):
    from zolt_amd import api
    assert [g for g, _, _ in captured_points].count(M.G1) == 17 + 2 and len(captured_points) == 17 + 16 + 4
    negatives = 0
    for group, name, b in captured_points:
        st, p = M.decode(group, M.ARK_COMPRESSED, b)
        assert st == M.OK and (M.on_curve(group, p) if p is not None else b[-1] == 0x40 and not any(b[:-1])), name  # (the run has identities)
        xy, inf = M.pack(group, [p])
        assert (api.compressG1 if group == M.G1 else api.compressG2)(xy[0], int(inf[0])) == bytes(b), name
        assert M.encode(group, M.ARK_COMPRESSED, p) == bytes(b), name
        want = DC.decompress_g1(b) if group == M.G1 else DC.decompress_g2(b)
        assert p == want, name
        if group == M.G1:
            assert p == DOM.decompress_g1(b), name
        negatives += b[-1] >> 7
    assert 0 < negatives < len(captured_points)  # both sign flags occur in what the reference wrote


def test_square_roots_and_sign_rules():
    for v in (0, 1, 2, 3, 4, P - 1, 5 ** 40 % P):
        r = M.fp_sqrt(v)
        assert (r is None) == (pow(v, (P - 1) // 2, P) == P - 1) and (r is None or r * r % P == v)
    assert M.y_is_positive(0) and M.y_is_positive((P - 1) // 2) and not M.y_is_positive((P + 1) // 2)
    assert M.fp2_is_positive((P - 1, 1)) and not M.fp2_is_positive((1, P - 1)) and M.fp2_is_positive((1, 0)) and not M.fp2_is_positive((P - 1, 0))
    for a in [(3, 0), (P - 3, 0), (0, 5), (7, 11), (123456789, 987654321), (0, 0)]:
        r = M.fp2_sqrt(a)
        assert r is None or G2.f2_sqr(r) == (a[0] % P, a[1] % P)
        assert (r is None) == (M.fp2_sqrt_branch(a) == "none")


# ---------------------------------------------------------------- 2. the lane functions on the host
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")


def _build(tmp, flags):
    path = str(tmp / "point_bytes_host")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "point_bytes_host.cpp"), "-o", path], check=True, capture_output=True, text=True)
    return path


def _run(exe, group, encoding, flags, records):
    res = subprocess.run([exe], input=b"%d %d %d %d\n" % (group, encoding, flags, len(records)) + b"".join(records), capture_output=True, check=True)
    out = []
    for line in res.stdout.decode().splitlines():
        t = line.split()
        out.append((int(t[0]), int(t[1]), [int(w, 16) for w in t[2:]]))
    assert len(out) == len(records)
    return out


def _g2_x_with_real_rhs():
    """x in Fp2 with Im(x^3 + b') = 0, so the root is the a1 = 0 case (dory.zig:273-286): 3 x0^2 x1 - x1^3 + b1 = 0 solved for x0, one for
    each of the two sub-cases (the real part a square in Fp, or not)"""
    found = {}
    for x1 in range(1, 200):
        x0 = M.fp_sqrt((x1 ** 3 - G2.B_TWIST[1]) * pow(3 * x1, -1, P) % P)
        if x0 is None:
            continue
        x = (x0, x1)
        rhs = M.g2_rhs(x)
        assert rhs[1] == 0
        found.setdefault(M.fp2_sqrt_branch(rhs), x)
        if len(found) == 2:
            break
    assert sorted(found) == ["a1=0,+", "a1=0,-"]
    return [found["a1=0,+"], found["a1=0,-"]]


def vectors(group, encoding):
    """[(record, flags)] over the cases of the section: points, identities, a coordinate >= p, ARK flag bits, both sign flags, an x
    without a root, the Fp2 root's branches, off-curve points with and without the check"""
    pts = M.g1_multiples(12, 3) if group == M.G1 else M.g2_multiples(12, 3)
    neg = (lambda p: (p[0], -p[1] % P)) if group == M.G1 else G2.neg
    recs = []
    if encoding == M.ARK_COMPRESSED:
        for p in pts:
            recs += [M.encode(group, encoding, p), M.encode(group, encoding, neg(p)), M.encode(group, encoding, p, sign=0xC0)]
        recs += [M.encode(group, encoding, None), bytes([7] * (M.record_bytes(group, encoding) - 1)) + bytes([0x40 | 0x15])]  # 0x40 alone decides
        # a coordinate >= p: x + p in x's place, the flag bits left zero (G1: an x small enough for x + p to fit under them)
        if group == M.G1:
            small = next(p for p in M.g1_multiples(40, 3) if p[0] + P < 1 << 254 and M.y_is_positive(p[1]))
            recs.append((small[0] + P).to_bytes(32, "little"))
        else:
            q = next(p for p in pts if M.fp2_is_positive(p[1]))
            recs.append((q[0][0] + P).to_bytes(32, "little") + q[0][1].to_bytes(32, "little"))
        no_root = []
        for v in range(1, 60):
            x = v if group == M.G1 else (v, 1)
            rhs = M.g1_rhs(x) if group == M.G1 else M.g2_rhs(x)
            if (M.fp_sqrt(rhs) if group == M.G1 else M.fp2_sqrt(rhs)) is None:
                no_root.append(M.encode(group, encoding, (x, 0 if group == M.G1 else (0, 0)), sign=0))
        assert len(no_root) >= 4
        recs += no_root[:4]
        if group == M.G2_:
            branches = {M.fp2_sqrt_branch(M.g2_rhs(p[0])) for p in pts}
            assert {"+", "-"} <= branches  # both c^2 = delta and c^2 = -delta among the multiples
            for x in _g2_x_with_real_rhs():
                y = M.fp2_sqrt(M.g2_rhs(x))
                recs += [M.encode(group, encoding, (x, y)), M.encode(group, encoding, (x, G2.neg((x, y))[1]))]
        return [(r, 0) for r in recs]
    out = []
    for p in pts[:6]:
        out += [(M.encode(group, encoding, p), 0), (M.encode(group, encoding, p), M.CHECK)]
    out += [(M.encode(group, encoding, None), 0), (M.encode(group, encoding, None), M.CHECK)]
    off = (pts[0][0], pts[1][1])  # x of one point, y of another
    out += [(M.encode(group, encoding, off), 0), (M.encode(group, encoding, off), M.CHECK)]
    # a coordinate >= p: x + p (< 2^255) in x's place — the same point
    p0 = pts[2]
    over = (p0[0] + P, p0[1]) if group == M.G1 else ((p0[0][0] + P, p0[0][1] + P), p0[1])
    out += [(M.encode(group, encoding, over), M.CHECK)]
    if encoding == M.ARK:
        for bits in (0x40, 0x80, 0xC0):
            out += [(M.encode(group, encoding, pts[3], top_bits=bits), M.CHECK), (M.encode(group, encoding, None, top_bits=bits), 0)]
    else:  # without ARK's mask the last coordinate may exceed p too, up to 2^256 - 1
        out += [(bytes([0xFF]) * M.record_bytes(group, encoding), 0)]
    return out


def expected(group, encoding, rec, flags):
    st, p = M.decode(group, encoding, rec, flags)
    if st != M.OK:
        return st, None, None
    xy, inf = M.pack(group, [p])
    return st, int(inf[0]), [int(w) for w in xy[0]]


@needs_hipcc
@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_lane_functions_on_the_host(tmp_path, flags):
    exe = _build(tmp_path, flags)
    seen = set()
    for group in (M.G1, M.G2_):
        for encoding in (M.BE, M.LE, M.ARK, M.ARK_COMPRESSED):
            vec = vectors(group, encoding)
            for fl in sorted({f for _, f in vec}):
                recs = [r for r, f in vec if f == fl]
                got = _run(exe, group, encoding, fl, recs)
                for k, (rec, g) in enumerate(zip(recs, got)):
                    st, inf, words = expected(group, encoding, rec, fl)
                    assert g[0] == st, (group, encoding, fl, k)
                    seen.add((group, encoding, st))
                    if st == M.OK:
                        assert (g[1], g[2]) == (inf, words), (group, encoding, fl, k)
                        seen.add((group, encoding, "inf" if inf else "point"))
    for group in (M.G1, M.G2_):
        for encoding in (M.BE, M.LE, M.ARK):
            assert {(group, encoding, M.OK), (group, encoding, M.NOT_ON_CURVE), (group, encoding, "inf"), (group, encoding, "point")} <= seen
        assert {(group, M.ARK_COMPRESSED, M.OK), (group, M.ARK_COMPRESSED, M.NO_ROOT), (group, M.ARK_COMPRESSED, "inf")} <= seen


# ---------------------------------------------------------------- 3. header, bindings, exports, no device, containers
NAMES = ["zg_g1_points_from_bytes", "zg_g2_points_from_bytes", "zg_g1_bases_from_bytes", "zg_dory_key_from_bytes"]


def test_header_section_and_bindings():
    from zolt_amd import _abi, lib
    text = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "#define ZG_FEATURE_POINT_BYTES 1024u" in text and "#define ZG_ABI_MINOR 11\n" in text
    assert text.index("------ Pairings (engine) */") < text.index("------ Points from bytes */") < text.index("------ poly tables */")
    assert all(n in lib.SYMBOLS and hasattr(lib._lib, n) for n in NAMES)
    assert subprocess.run([os.sys.executable, os.path.join(ROOT, "tools", "gen_bindings.py"), "--check"], capture_output=True).returncode == 0
    zig = open(os.path.join(ROOT, "zig", "gpu", "ffi.zig")).read()
    assert all(f"pub extern fn {n}(" in zig for n in NAMES) and "pub const FEATURE_POINT_BYTES: u32 = 1024;" in zig
    pt = (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    assert _abi.PROTOS["zg_g1_points_from_bytes"] == pt == _abi.PROTOS["zg_g2_points_from_bytes"]
    assert _abi.PROTOS["zg_g1_bases_from_bytes"] == (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    assert _abi.PROTOS["zg_dory_key_from_bytes"] == (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                                               C.c_void_p])
    assert _abi.ZG_FEATURE_POINT_BYTES == 1024 and lib.abi_features() & 1024 and lib.abi_version() == (1, 11)
    assert (_abi.ZG_POINT_BYTES_BE, _abi.ZG_POINT_BYTES_LE, _abi.ZG_POINT_BYTES_ARK, _abi.ZG_POINT_BYTES_ARK_COMPRESSED, _abi.ZG_POINT_BYTES_CHECK) == (0, 1, 2, 3, 1)


def test_bad_arguments_are_invalid_and_nothing_decodes_without_a_device():
    from zolt_amd import lib
    L = lib._lib
    data = np.zeros(4 * 128, dtype=np.uint8)
    out = np.full(4 * 16, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    inf = np.full(4, 0xA5, dtype=np.uint8)
    bad, h = C.c_size_t(99), C.c_void_p(77)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for fn in (L.zg_g1_points_from_bytes, L.zg_g2_points_from_bytes):
        assert fn(None, 4, 0, 0, p(out), p(inf), C.byref(bad)) == lib.ERR_INVALID   # NULL data with n > 0
        assert fn(p(data), 4, 4, 0, p(out), p(inf), C.byref(bad)) == lib.ERR_INVALID  # unknown encoding
        assert fn(p(data), 4, 0, 2, p(out), p(inf), C.byref(bad)) == lib.ERR_INVALID  # unknown flag bits
        assert fn(p(data), 4, 0, 0, None, p(inf), C.byref(bad)) == lib.ERR_INVALID    # no output
        assert fn(p(data), (1 << 28) + 1, 0, 0, p(out), p(inf), C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_g1_bases_from_bytes(p(data), 0, 0, 0, None, C.byref(h), C.byref(bad)) == lib.ERR_INVALID  # n = 0
    assert h.value is None
    h = C.c_void_p(77)
    assert L.zg_g1_bases_from_bytes(p(data), 4, 0, 0, None, None, C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_g1_bases_from_bytes(None, 4, 0, 0, None, C.byref(h), C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_dory_key_from_bytes(p(data), 0, 2, p(data), 4, 2, 0, C.byref(h), C.byref(bad)) == lib.ERR_INVALID  # n_g1 = 0
    assert L.zg_dory_key_from_bytes(p(data), (1 << 16) + 1, 2, p(data), 4, 2, 0, C.byref(h), C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_dory_key_from_bytes(p(data), 4, 2, None, 4, 2, 0, C.byref(h), C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_dory_key_from_bytes(p(data), 4, 2, p(data), 4, 5, 0, C.byref(h), C.byref(bad)) == lib.ERR_INVALID
    assert L.zg_dory_key_from_bytes(p(data), 4, 2, p(data), 4, 2, 0, None, C.byref(bad)) == lib.ERR_INVALID
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and (inf == 0xA5).all() and bad.value == 99
    if os.path.exists("/dev/kfd"):
        return  # a GPU is present: the no-device answer cannot be observed (tests/test_gpu_point_bytes.py runs the section instead)
    h = C.c_void_p()
    assert L.zg_g1_points_from_bytes(p(data), 4, 0, 1, p(out), p(inf), C.byref(bad)) == lib.ERR_NO_DEVICE
    assert L.zg_g2_points_from_bytes(p(data), 4, 3, 0, p(out), None, None) == lib.ERR_NO_DEVICE
    assert L.zg_g1_points_from_bytes(None, 0, 0, 0, None, None, None) == lib.ERR_NO_DEVICE
    assert L.zg_g1_bases_from_bytes(p(data), 4, 1, 1, None, C.byref(h), C.byref(bad)) == lib.ERR_NO_DEVICE
    assert L.zg_dory_key_from_bytes(p(data), 4, 2, p(data), 4, 2, 0, C.byref(h), C.byref(bad)) == lib.ERR_NO_DEVICE
    assert (out == 0xA5A5A5A5A5A5A5A5).all() and (inf == 0xA5).all() and bad.value == 99 and h.value is None


def test_containers_reach_their_error_names_before_any_device_call():
    from zolt_amd import api
    # loadFromRawBinary: u32 n | n * 64 | 128 | 64 | 128
    for data in (b"", b"\x01\x00", (2).to_bytes(4, "little") + bytes(2 * 64 + 128 + 64 + 127)):
        with pytest.raises(api.SRSError, match="TruncatedData"):
            api.srs_from_raw(data)
    # loadFromPtau
    with pytest.raises(api.SRSError, match="TruncatedData"):
        api.srs_from_ptau(b"ptau")
    with pytest.raises(api.SRSError, match="InvalidFileFormat"):
        api.srs_from_ptau(b"utap" + bytes(8))
    with pytest.raises(api.SRSError, match="UnsupportedFormat"):
        api.srs_from_ptau(b"ptau" + (2).to_bytes(4, "little") + bytes(4))
    with pytest.raises(api.SRSError, match="TruncatedData"):
        api.srs_from_ptau(b"ptau" + (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + (2).to_bytes(4, "little") + (640).to_bytes(8, "little") + bytes(64))
    with pytest.raises(api.SRSError, match="InvalidFileFormat"):  # no header section
        api.srs_from_ptau(b"ptau" + (1).to_bytes(4, "little") + (0).to_bytes(4, "little"))
    # the Jolt Dory SRS
    good = b"JOLT_DORY_SRS_V1" + (3).to_bytes(8, "little") + (4).to_bytes(8, "little") + bytes(4 * 64) + (2).to_bytes(8, "little") + bytes(2 * 128) + bytes(192)
    with pytest.raises(api.DorySrsError, match="InvalidSrsFormat"):
        api.Dory.loadFromFile(b"JOLT_DORY_SRS_V2" + good[16:])
    for cut in (10, 20, 30, 32 + 4 * 64 - 1, 32 + 4 * 64 + 4, 32 + 4 * 64 + 8 + 128, len(good) - 1):
        with pytest.raises(api.DorySrsError, match="TruncatedData"):
            api.Dory.loadFromFile(good[:cut])
    assert api.Dory.parseSrsContainer(good)[:1] == (3,) and api.Dory.parseSrsContainer(good)[3:] == (2, 1)
