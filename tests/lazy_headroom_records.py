"""Edge records for the un-carried linear forms of the mixed addition (zolt_amd/csrc/fp29.hip.h: f29_sub7_raw, f29_pmsub45_raw,
f29_neg4_raw; g1_29.hip.h: xyzz29_madd_nz), in the record format of zg_selftest_lazy_g1, and the checks of what comes back. Built on
tests/lazy_model.py (the big-integer model, the class bounds, the group law); shared by tests/test_lazy_g1_headroom_host.py (the CPU)
and tests/test_gpu_lazy_g1_headroom.py (the device). Plain module: no fixtures, no pytest hooks.

What the un-carried forms change is the SIZE of the limbs the multiplier sees, so the records aim at limbs: every limb of acc.x at
2^29 + 7 (limb 0 at 2^29 - 1: acc.x is a carry output), the point's and the products' limbs (U2, S2) all at 2^29 - 1, the classes'
top representatives, both signs, and acc = +-P, where the zero test reads un-carried limbs."""
import os
import shutil
import subprocess

import numpy as np

from tests import lazy_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def host_harness(exe, extra=()):
    """build tests/cpp/lazy_g1_headroom_host.cpp (the kernels' headers for the CPU) as `exe`; -> run(op, items) -> (as given, carried
    reference), each (n, 146) u32. The program exits non-zero if the two forms of an addition differ in any word."""
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-DZG_F29_SERIAL", "-std=c++17", "-O1", *extra, "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lazy_g1_headroom_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)

    def run(op, items):
        res = subprocess.run([exe], input=f"{op} {len(items)}\n".encode() + lm.pack(items).tobytes(), capture_output=True)
        assert res.returncode == 0, (res.returncode, res.stderr.decode()[-2000:])
        out = np.frombuffer(res.stdout, dtype=np.uint32).reshape(len(items), 2, lm.OUT_WORDS)
        return out[:, 0], out[:, 1]

    return run


P, MASK = lm.P, lm.MASK
MADD_CARRY_ALL = 1 << 3  # lazy_selftest.hip.h: LAZY_MADD_CARRY_ALL
LIN_RAW = 1 << 16        # lazy_selftest.hip.h: LAZY_LIN_RAW
RAW_BITS = (lm.LIN_SUB7, lm.LIN_PMSUB_POS, lm.LIN_PMSUB_NEG, lm.LIN_NEG4)
HI = [lm.NEAR - 1] * 8   # 2^29 + 7


def raised(k, r):
    """fp29.hip.h RAW4P / RAW5P / RAW7P: k*p with limbs 0..7 raised by 2^r, the excess borrowed from the next limb"""
    L, e = lm.limbs(k * P), 1 << (r - 29)
    return [L[0] + (1 << r)] + [L[i] + (1 << r) - e for i in range(1, 8)] + [L[8] - e]


RAW4P, RAW5P, RAW7P = raised(4, 29), raised(5, 30), raised(7, 29)


def top_for(lo, bound, back=0):
    """limbs `lo` (0..7) plus the largest top limb that keeps the value below `bound`, minus `back`"""
    return list(lo) + [((bound - 1 - lm.val(lo)) >> 232) - back]


def acc_from_z(g, pt, z, xmode="rand", ymode="rand", ybound=lm.ACC_Y):
    """the accumulator (x, y, zz, zzz) of the affine point pt with a given z; exact limbs"""
    zz, zzz = z * z % P, z * z * z % P
    vals = [lm.to_mont(pt[0] * zz % P), lm.to_mont(pt[1] * zzz % P), lm.to_mont(zz), lm.to_mont(zzz)]
    return [lm.limbs(g.rep(vals[0], lm.ACC_X, xmode)), lm.limbs(g.rep(vals[1], ybound, ymode)), lm.limbs(vals[2]), lm.limbs(vals[3])]


def _forced_x_acc(g, pt, lo):
    """an accumulator of pt whose x has the low limbs `lo`: the top limb walks down from the class maximum until z exists"""
    for back in range(64):
        fl = top_for(lo, lm.ACC_X, back)
        z = lm.sqrt_mod(lm.from_mont(lm.val(fl)) * pow(pt[0], -1, P) % P)
        if z:
            a = acc_from_z(g, pt, z)
            assert lm.val(fl) % P == lm.val(a[0]) % P
            a[0] = fl
            return a
    raise AssertionError("no square root in 64 tries")


def _all_ones_row(g, coord):
    """a table row (x, y < 1.1p, exact limbs) with every limb 0..7 of one coordinate at 2^29 - 1; the point is solved for"""
    for back in range(256):
        fl = top_for([MASK] * 8, lm.ROW, back)
        v = lm.from_mont(lm.val(fl))
        if coord == "x":
            y = lm.sqrt_mod((v ** 3 + lm.B) % P)
            if y:
                return (v, y), [fl, lm.limbs(lm.to_mont(y))]
        else:
            x = lm.cbrt_mod((v * v - lm.B) % P)
            if x:
                return (x, v), [lm.limbs(lm.to_mont(x)), fl]
    raise AssertionError("no point in 256 tries")


def _product_all_ones(g, q, row, which):
    """an accumulator for which U2 = px * zz (which = 0) or S2 = py * zzz (1) comes out with every limb 0..7 at 2^29 - 1. The lazy product
    of a < 1.1p and b < 1.6p is the representative of a*b*2^-261 in [a*b/2^261, a*b/2^261 + p), and a*b/2^261 < 0.011p: a target T in
    (0.011p, p) is returned as T itself."""
    for back in range(256):
        T = lm.val(top_for([MASK] * 8, P, back))
        assert P // 64 < T < P
        w = lm.from_mont(T) * pow(q[which], -1, P) % P  # zz (or zzz) as a field element
        z = lm.sqrt_mod(w) if which == 0 else lm.cbrt_mod(w)
        if z:
            a = acc_from_z(g, g.point(), z, "top", "top")
            assert lm.val(a[2 + which]) * lm.val(row[which]) * lm.MONT_INV % P == T
            return a
    raise AssertionError("no root in 256 tries")


def edge_madd_records(seed):
    """[(kind, record, effective point, accumulator's point)] as lm.madd_records; both signs of every record"""
    g = lm.Gen(seed)
    out = []

    def put(kind, acc, q, row=None):
        for s in (0, 1):
            out.append((f"{kind}{'-' if s else '+'}", lm.record(acc + (row or g.row(q)), s), lm.neg(q) if s else q, lm.acc_point(acc)))

    x_hi = [MASK] + HI[1:]  # every limb of acc.x at 2^29 + 7, limb 0 at 2^29 - 1
    for _ in range(4):
        a = g.point()
        put("x-limbs-max", _forced_x_acc(g, a, x_hi), g.point())
        # ... and acc = +-P on such an accumulator: P = U2 + 7p - X1 = k p is tested un-carried
        acc = _forced_x_acc(g, a, x_hi)
        put("x-limbs-max-double", acc, a)         # + : double, - : infinity
        put("x-limbs-max-infinity", acc, lm.neg(a))
    for coord in ("x", "y"):
        q, row = _all_ones_row(g, coord)
        put(f"row-{coord}-all-ones", g.acc(g.point(), "top", "top", "top"), q, row)
        put(f"row-{coord}-all-ones-x-max", _forced_x_acc(g, g.point(), x_hi), q, row)
        for which in (0, 1):
            put(f"{'s2' if which else 'u2'}-all-ones", _product_all_ones(g, q, row, which), q, row)
    for _ in range(4):
        q = g.point()
        row = g.row(q)
        for which in (0, 1):
            put(f"{'s2' if which else 'u2'}-all-ones", _product_all_ones(g, q, row, which), q, row)
    # the classes' top representatives: x < 6.6p, y < 1.4p, and the run-start accumulator with y <= 2p (a negated affine y)
    for _ in range(8):
        put("class-top", g.acc(g.point(), "top", "top", "top"), g.point())
        put("run-start-negated", g.run_start(g.point(), True), g.point())
        put("run-start-y-2p", lm._start_like(g), g.point())
        a = g.point()
        put("class-top-double", g.acc(a, "top", "top", "top"), a)
        put("run-start-double", g.run_start(a, False), a)
    return out


def madd_items(seed, n_random):
    """the edge records, then the generator's own families (regular, double, infinity, forced limbs, run starts; both signs)"""
    return edge_madd_records(seed) + lm.madd_records(seed + 1, n_random)


def check_madd(items, out_new, out_ref, device):
    """the un-carried addition against the carried one limb for limb, and against the big-integer model (lm.check: group element,
    classes, exact output limbs, exc code, inf flag)"""
    out_new, out_ref = np.asarray(out_new), np.asarray(out_ref)
    for i, it in enumerate(items):
        assert np.array_equal(out_new[i], out_ref[i]), (i, it[0], "un-carried and carried additions differ")
    lm.check(lm.MADD, items, out_ref, device)
    return lm.check(lm.MADD, items, out_new, device)


def _raw(a, bias, b, xor=0):
    return [((x ^ xor) + c - y) & 0xFFFFFFFF for x, c, y in zip(a, bias, b)]


def lin_items(seed, n):
    """LIN records for the raw slots: [(kind, record)]. a: a mul output (exact limbs, < 1.6p), b: a near-normalised subtrahend of the
    call sites' classes (acc.x < 6.6p under 7p; acc.y <= 2p under 4p / 5p). Then the zero test on UN-CARRIED limbs: k p written as
    U2 + RAW7P - X1 and as +-S2 + RAW4P|RAW5P - Y1, and the same off by one in one limb."""
    g = lm.Gen(seed)
    r = g.rng
    bit = lambda *ks: sum(1 << k for k in ks)
    z9 = [0] * 9
    out = []
    a_set = [lm.limbs(lm.MUL_OUT - 1), [MASK] * 8 + [((lm.MUL_OUT - 1) >> 232) - 1], z9, lm.limbs(1)]
    for a in a_set + [lm.limbs(r.randrange(lm.MUL_OUT)) for _ in range(4)]:
        for bound, mask in ((lm.ACC_X, bit(lm.LIN_SUB7)), (lm.NEG_Y + 1, bit(lm.LIN_PMSUB_POS, lm.LIN_PMSUB_NEG, lm.LIN_NEG4))):
            for b in (top_for(HI, bound), top_for([MASK] + HI[1:], bound), lm.limbs(bound - 1), z9, g.forced(bound, False)):
                out.append(("raw-extreme", lm.record([a, b, z9], mask | LIN_RAW)))
    while len(out) < n // 2:
        a = lm.limbs(r.randrange(lm.MUL_OUT))
        b = g.forced(lm.NEG_Y + 1, False) if r.random() < 0.5 else g.enc(r.randrange(lm.NEG_Y + 1), False)
        out.append(("raw-random", lm.record([a, b, z9], bit(*RAW_BITS) | LIN_RAW)))
    zero = bit(lm.LIN_IS_ZERO)
    while len(out) < n:
        k = r.randrange(1, 9)
        if r.random() < 0.5:  # P = U2 + 7p - X1 = k p: X1 = U2 + (7 - k) p < 6.6p
            u2 = r.randrange(lm.kp("0.5") if k == 1 else lm.MUL_OUT)
            x1 = u2 + (7 - k) * P
            if not 0 <= x1 < lm.ACC_X:
                continue
            x = _raw(lm.limbs(u2), RAW7P, g.enc(x1, True))
        else:  # R = S2 + 4p - Y1 (k <= 4) or 5p - S2 - Y1 (k <= 5) = k p
            s2 = r.randrange(lm.MUL_OUT)
            if r.random() < 0.5:
                y1, bias, xor = s2 + (4 - k) * P, RAW4P, 0
            else:
                y1, bias, xor = (5 - k) * P - s2, [c + 1 for c in RAW5P], 0xFFFFFFFF
            if not 0 <= y1 <= lm.NEG_Y:
                continue
            x = _raw(lm.limbs(s2), bias, g.enc(y1, False), xor)
        assert lm.val(x) == k * P and max(x[:8]) < 3 << 29
        out.append((f"raw-zero-{k}p", lm.record([x, z9, z9], zero)))
        i = r.randrange(9)
        near = list(x)
        near[i] += r.choice((1, -1))
        out.append(("raw-near-zero", lm.record([near, z9, z9], zero)))
    return out[:n]


def check_lin(items, out_new, out_ref):
    """the raw slots: the same integers as the carried forms and as the exact formulas, limbs 0..7 within the bounds fp29.hip.h states
    and a top limb that did not wrap; the zero test on un-carried limbs: yes to k p, no to its neighbours"""
    seen = set()
    for i, (it, o, ref) in enumerate(zip(items, np.asarray(out_new), np.asarray(out_ref))):
        kind, rec = it[0], it[1]
        a, b = (lm.val(rec[9 * k:9 * k + 9]) for k in range(2))
        al = [int(x) for x in rec[:9]]
        mask = int(rec[90])
        exact = {lm.LIN_SUB7: (a + 7 * P - b, RAW7P), lm.LIN_PMSUB_POS: (a + 4 * P - b, RAW4P), lm.LIN_PMSUB_NEG: (5 * P - a - b, RAW5P),
                 lm.LIN_NEG4: (4 * P - b, RAW4P)}
        for k, (v, bias) in exact.items():
            l = [int(x) for x in o[9 * k:9 * k + 9]]
            if not mask >> k & 1:
                assert not any(l), (i, kind, k, "not asked for")
                continue
            assert mask & LIN_RAW
            assert lm.val(l) == v == lm.val([int(x) for x in ref[9 * k:9 * k + 9]]), (i, kind, k, "value")
            minuend = [0] * 9 if k in (lm.LIN_NEG4, lm.LIN_PMSUB_NEG) else al
            assert all(0 <= x <= m + c for x, m, c in zip(l, minuend, bias)) and max(l[:8]) < 3 << 29, (i, kind, k, [hex(x) for x in l])
            seen.add(k)
        if mask >> lm.LIN_IS_ZERO & 1:
            want = 1 if a % P == 0 and a // P <= lm.ZERO_DOMAIN else 0
            assert int(o[144]) == want == int(ref[144]), (i, kind, "f29_is_zero_modp on un-carried limbs", int(o[144]), a / P)
            assert want == (1 if kind.startswith("raw-zero") else 0), (i, kind)
            seen.add(kind.rsplit("-", 1)[0] if kind.startswith("raw-zero") else kind)
    assert seen >= set(RAW_BITS) | {"raw-zero", "raw-near-zero"}, seen
