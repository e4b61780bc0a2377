"""Pins tests/pairing_model.py — the big-integer model tests/test_gpu_pairing.py checks the device pairing against — to the one value of
the reference's pairing that is recorded (Jolt's e(G1, G2), tests/golden/pairing_generator_jolt.json), to the algebra a pairing must
satisfy, and the ABI facts of the section "Pairings (Dory)". CPU only."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np

from tests import g2_model as G2
from tests import pairing_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_generator_jolt.json")))
PAIRING_EXPORTS = ("zg_miller_loop_batch", "zg_final_exponentiation_batch", "zg_pairing_batch", "zg_multi_pairing", "zg_multi_pairing_dev")
P, R = M.P, M.R

_rng = random.Random(0x9A1E)


def _rand_fp12(rng=_rng):
    return tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))


_cache = {}


def _gen_miller():
    if "m" not in _cache:
        _cache["m"] = M.miller_loop(M.G1_GEN, G2.G)
        _cache["e"] = M.final_exponentiation(_cache["m"])
    return _cache["m"], _cache["e"]


def test_fixture_operands_are_the_generators():
    assert (FIXTURE["g1"]["x"], FIXTURE["g1"]["y"]) == M.G1_GEN
    for name, v in zip(("x_c0", "x_c1", "y_c0", "y_c1"), (G2.G[0][0], G2.G[0][1], G2.G[1][0], G2.G[1][1])):
        assert v.to_bytes(32, "little")[:16].hex() == FIXTURE["g2_generator_le_prefix_hex"][name]


def test_generator_pairing_has_jolts_bytes():
    _, e = _gen_miller()
    assert M.to_bytes(e)[:16].hex() == FIXTURE["pairing_to_bytes_first_16_hex"] == "950e879d73631f5eb5788589eb5f7ef8"


def test_pairing_has_order_r_and_is_not_one():
    _, e = _gen_miller()
    assert e != M.ONE and M.power(e, R) == M.ONE


def test_loop_count_is_6x_plus_2_in_65_signed_digits():
    d = M.ATE_LOOP_COUNT
    assert len(d) == 65 and set(d) <= {-1, 0, 1} and sum(v << i for i, v in enumerate(d)) == 6 * M.X + 2
    assert all(not (d[i] and d[i + 1]) for i in range(63))  # non-adjacent below the leading (1, 1)


def test_bilinearity():
    rng = random.Random(7)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    _, e = _gen_miller()
    assert M.pairing(M.g1_mul(M.G1_GEN, a), G2.scalar_mul(G2.G, b)) == M.power(e, a * b % R)


def test_final_exponentiation_is_a_homomorphism_and_inverse_points_cancel():
    m1, e1 = _gen_miller()
    q = G2.scalar_mul(G2.G, 5)
    p = M.g1_mul(M.G1_GEN, 3)
    m2 = M.miller_loop(p, q)
    e2 = M.final_exponentiation(m2)
    assert M.final_exponentiation(M.mul(m1, m2)) == M.mul(e1, e2)
    assert M.multi_pairing([M.G1_GEN, p], [G2.G, q]) == M.mul(e1, e2)
    assert M.mul(e2, M.pairing(M.g1_neg(p), q)) == M.ONE
    assert M.multi_pairing([p, M.g1_neg(p)], [q, q]) == M.ONE


def test_identities_and_zero():
    assert M.pairing(None, G2.G) == M.ONE and M.pairing(M.G1_GEN, None) == M.ONE and M.miller_loop(None, None) == M.ONE
    assert M.final_exponentiation(M.ZERO) == M.ONE and M.final_exponentiation(M.ONE) == M.ONE
    assert M.multi_pairing([], []) == M.ONE


def test_chain_is_one_power_by_the_stated_exponent():
    """the Fuentes-Castaneda chain realises c (p^4 - p^2 + 1) / r with c = 2x(6x^2 + 3x + 1), not (p^4 - p^2 + 1) / r"""
    x = M.X
    phi = P ** 4 - P ** 2 + 1
    assert phi % R == 0
    # the chain's exponents restated as integers (pairing.zig:1812-1880): y0 = r^-x ... y16
    y1 = -2 * x
    y3 = 3 * y1
    y4 = -x * y3
    y6 = x * (2 * y4)  # conjugate(exp_by_neg_x(y5))
    y8 = y6 + y4 - y3
    y9 = y8 + y1
    y11 = y8 + y4 + 1
    h = P * y9 + y11 + P * P * y8 + P ** 3 * (y9 - 1)
    assert (h - M.HARD_C * (phi // R)) % phi == 0
    assert M.HARD_EXPONENT == M.HARD_C * (phi // R)
    m, e = _gen_miller()
    assert M.power(m, M.FINAL_EXPONENT) == e
    f = _rand_fp12()
    assert M.power(f, M.FINAL_EXPONENT) == M.final_exponentiation(f)


def test_frobenius_is_the_power_by_p():
    f = _rand_fp12()
    fp = M.power(f, P)
    assert M.frobenius(f) == fp
    assert M.frobenius(f, 2) == M.frobenius(fp) and M.frobenius(f, 3) == M.frobenius(M.frobenius(fp))
    assert M.frobenius(f, 6) == M.conj(f) and M.frobenius(f, 12) == f


def test_mul_by_034_is_the_product_by_the_sparse_element():
    f = _rand_fp12()
    c0, c3, c4 = ((_rng.randrange(P), _rng.randrange(P)) for _ in range(3))
    # in the tower: c0 in c0.c0, c3 in c1.c0 (w), c4 in c1.c1 (v w = w^3)
    sparse = M.from_bytes(b"".join(v.to_bytes(32, "little") for v in (c0[0], c0[1], 0, 0, 0, 0, c3[0], c3[1], c4[0], c4[1], 0, 0)))
    assert M.mul_by_034(f, c0, c3, c4) == M.mul(f, sparse)


def test_inverse_and_exp_by_x():
    f = _rand_fp12()
    assert M.mul(M.inv(f), f) == M.ONE and M.inv(M.ZERO) == M.ZERO and M.inv(M.ONE) == M.ONE
    assert M.exp_by_x(f) == M.power(f, 4965661367192848881)
    assert M.mul(f, M.ONE) == f and M.sqr(f) == M.mul(f, f) and M.mul(f, M.conj(f)) == M.mul(M.conj(f), f)


def test_tower_layout_w_squared_is_v_and_v_cubed_is_xi():
    def at(place, val=(1, 0)):  # the element with `val` at Fp2 place 0..5 of toBytes' order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2
        vals = [0] * 12
        vals[2 * place], vals[2 * place + 1] = val
        return M.from_bytes(b"".join(v.to_bytes(32, "little") for v in vals))
    w, v = at(3), at(1)
    assert M.sqr(w) == v and M.mul(v, at(2)) == at(0, M.XI) and M.mul(v, v) == at(2) and M.mul(w, v) == at(4)


def test_to_bytes_round_trip_and_packing():
    f = _rand_fp12()
    b = M.to_bytes(f)
    assert len(b) == 384 and M.from_bytes(b) == f
    assert b[:32] == f[0][0].to_bytes(32, "little") and b[64:96] == f[2][0].to_bytes(32, "little") and b[192:224] == f[1][0].to_bytes(32, "little")
    packed = M.gt_pack([f, M.ONE])
    assert packed.shape == (2, 48) and M.gt_unpack(packed) == [f, M.ONE]
    assert list(packed[1][:4]) == G2.fp_limbs(1) and not packed[1][4:].any()
    pts = [M.G1_GEN, None, M.g1_mul(M.G1_GEN, 9)]
    assert M.g1_unpack(*M.g1_pack(pts)) == pts


def test_wire_gt_bytes_are_to_bytes():
    from zolt_amd import api
    f = _rand_fp12()
    words = M.gt_pack([f])[0]
    assert api.gt_to_bytes(words) == M.to_bytes(f)
    assert np.array_equal(api.gt_from_bytes(M.to_bytes(f)), words)


def test_device_constants_are_derived_and_match_the_model():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pairing_consts.py"), "--check"], cwd=ROOT).returncode == 0
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_pairing_consts as gen
    finally:
        sys.path.pop(0)
    for n in (1, 2, 3):
        for k in range(1, 6):
            w = [(0, 0)] * 6
            w[k] = (1, 0)
            assert M.frobenius(tuple(w), n)[k] == gen.gamma(n, k)
    assert gen.gamma(1, 2) == M.TWIST_MUL_BY_Q_X and gen.gamma(1, 3) == M.TWIST_MUL_BY_Q_Y
    assert gen.loop_digits(6 * gen.X + 2) == M.ATE_LOOP_COUNT


def test_abi_carries_the_pairing_section():
    from zolt_amd import _abi, lib
    assert _abi.ZG_ABI_MINOR == 11 and _abi.ZG_FEATURE_PAIRING == 16
    for name in PAIRING_EXPORTS:
        assert name in _abi.PROTOS, name
        assert hasattr(lib._lib, name)
    hdr = open(os.path.join(ROOT, "include", "zolt_gpu.h")).read()
    assert "Pairings (Dory)" in hdr and re.search(r"#define ZG_FEATURE_PAIRING 16u", hdr)
    assert hdr.index("G2 (Dory) */") < hdr.index("Pairings (Dory) */") < hdr.index("poly tables */")
    codes = [_abi.ZG_OP_FP12_MUL, _abi.ZG_OP_FP12_SQR, _abi.ZG_OP_FP12_INV, _abi.ZG_OP_FP12_CONJ, _abi.ZG_OP_FP12_FROB1, _abi.ZG_OP_FP12_FROB2,
             _abi.ZG_OP_FP12_FROB3, _abi.ZG_OP_FP12_EXP_X]
    assert codes == list(range(17, 25)) and "ZG_OP_FP12" not in hdr  # self-test hooks stay in the internal header
    assert [lib.OP_FP12_MUL, lib.OP_FP12_SQR, lib.OP_FP12_INV, lib.OP_FP12_CONJ, lib.OP_FP12_FROB1, lib.OP_FP12_FROB2, lib.OP_FP12_FROB3,
            lib.OP_FP12_EXP_X] == codes
    assert not any("fp12" in s.lower() or "pair" in s.lower() for s in _abi.INTERNAL_SYMBOLS)  # no new internal export
    for fn in ("miller_loop_batch", "final_exponentiation_batch", "pairing_batch", "multi_pairing", "multi_pairing_dev"):
        assert callable(getattr(lib, fn)), fn
    from zolt_amd import api
    for fn in ("multiPairG1G2", "multiPairBatch", "commit"):
        assert callable(getattr(api.Dory, fn)), fn
