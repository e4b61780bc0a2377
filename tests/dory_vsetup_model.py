"""DoryVerifierSetup (src/zkvm/preprocessing.zig:833-1166) restated literally over tests/pairing_model.py and tests/g2_model.py: multiPair
with its pairing AND its multiplication per pair (:833-850), fromSRS level by level (:889-973), and serialize with that file's own point
encodings (:975-1166). Points are affine integer tuples, None the identity; GT elements the model's Fp12 tuples. Nothing here batches or
reorders: it is what the device's one-launch-set form is compared against."""
from tests import g2_model as g2m
from tests import pairing_model as pm

P = g2m.P


def multi_pair(g1_vec, g2_vec):
    """multiPair (:833-850): one pairingFp and one product per pair, identities skipped (:839)"""
    n = min(len(g1_vec), len(g2_vec))
    if n == 0:
        return pm.ONE
    result = pm.ONE
    for i in range(n):
        if g1_vec[i] is None or g2_vec[i] is None:
            continue
        result = pm.mul(result, pm.pairing(g1_vec[i], g2_vec[i]))
    return result


class VerifierSetup:
    """the struct of :854-878 with its field names"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def from_srs(g1_vec, g2_vec):
    """fromSRS (:889-973)"""
    max_num_rounds = len(g1_vec).bit_length() - 1  # std.math.log2_int (:890)
    delta_1l, delta_1r, delta_2r, chi = [], [], [], []
    for k in range(max_num_rounds + 1):
        if k == 0:
            delta_1l.append(pm.ONE)
            delta_1r.append(pm.ONE)
            delta_2r.append(pm.ONE)
            chi.append(pm.pairing(g1_vec[0], g2_vec[0]))  # :914 (pairingFp answers one for an identity)
        else:
            half_len, full_len = 1 << (k - 1), 1 << k
            if full_len > len(g2_vec):
                raise IndexError("g2_vec is sliced out of bounds (:922-923)")
            g1_first, g1_second = g1_vec[0:half_len], g1_vec[half_len:full_len]
            g2_first, g2_second = g2_vec[0:half_len], g2_vec[half_len:full_len]
            delta_1l.append(chi[k - 1])                            # :926
            delta_1r.append(multi_pair(g1_second, g2_first))       # :929
            delta_2r.append(multi_pair(g1_first, g2_second))       # :932
            chi.append(pm.mul(chi[k - 1], multi_pair(g1_second, g2_second)))  # :935
    delta_2l = list(delta_1l)  # :940-945
    h1, h2 = g1_vec[0], g2_vec[0]  # :950-951
    return VerifierSetup(delta_1l=delta_1l, delta_1r=delta_1r, delta_2l=delta_2l, delta_2r=delta_2r, chi=chi, g1_0=g1_vec[0], g2_0=g2_vec[0],
                         h1=h1, h2=h2, ht=pm.pairing(h1, h2), max_log_n=max_num_rounds * 2)


def _u64(v):
    return int(v).to_bytes(8, "little")


def _limbs_le(v, last_or=0):
    """four u64 limbs little-endian, the flags ORed into the last (:1074-1089)"""
    limbs = [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
    limbs[3] |= last_or
    return b"".join(_u64(l) for l in limbs)


def serialize_gt(gt):
    """serializeGT (:1029-1059): c0 then c1, each Fp6 its three Fp2, each Fp 32 bytes of standard form — Fp12.toBytes' order"""
    return pm.to_bytes(gt)


def lexicographically_less(a, b):  # :1129-1139: limb by limb from the top = as integers, strictly
    return a < b


def lexicographically_less_fp2(a, b):  # :1141-1166: c1 first, then c0; equal is not less
    if a[1] != b[1]:
        return a[1] < b[1]
    return a[0] < b[0]


def serialize_g1(point):
    """serializeG1 (:1061-1090)"""
    if point is None:
        return _u64(0) * 3 + _u64(0x4000000000000000)
    x, y = point
    y_is_positive = lexicographically_less(y, -y % P)
    return _limbs_le(x, 0 if y_is_positive else 0x8000000000000000)


def serialize_g2(point):
    """serializeG2 (:1092-1127)"""
    if point is None:
        return _u64(0) * 7 + _u64(0x4000000000000000)
    x, y = point
    y_is_positive = lexicographically_less_fp2(y, g2m.f2_neg(y))
    return _limbs_le(x[0]) + _limbs_le(x[1], 0 if y_is_positive else 0x8000000000000000)


def serialize(vs):
    """serialize (:977-1025)"""
    out = b""
    for vec in (vs.delta_1l, vs.delta_1r, vs.delta_2l, vs.delta_2r, vs.chi):
        out += _u64(len(vec)) + b"".join(serialize_gt(g) for g in vec)
    out += serialize_g1(vs.g1_0) + serialize_g2(vs.g2_0) + serialize_g1(vs.h1) + serialize_g2(vs.h2)
    return out + serialize_gt(vs.ht) + _u64(vs.max_log_n)


def serialized_len(K):
    return 5 * (8 + (K + 1) * 384) + 32 + 64 + 32 + 64 + 384 + 8
