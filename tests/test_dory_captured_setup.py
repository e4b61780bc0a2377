"""The pairing and the Dory verifier setup held to bytes the REFERENCE wrote: tests/golden/dory_verifier_setup_captured.bin is
DoryVerifierSetup.serialize (src/zkvm/preprocessing.zig:977-1025) from the reference's captured prove run, K = 8 — a full 384-byte pairing
value at a non-generator input (chi[0] = e(g1_0, g2_0)), 41 GT values, four compressed points with their real sign flags. Without a GPU:
the models (tests/pairing_model.py, pairing_wave_model.py, dory_vsetup_model.py), the kernels' own headers compiled for the host
(tests/cpp/pairing_host.cpp) and the Python mirror's serialiser are each made answerable to those bytes. The device's side is
tests/test_gpu_dory_captured_setup.py. Every comparison is on bytes or words.

    python -m pytest tests/test_dory_captured_setup.py -q"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import dory_captured as DC
from tests import dory_vsetup_model as VM
from tests import g2_model as G2
from tests import pairing_model as M
from tests import pairing_wave_model as W
from tests.test_pairing_host import HIPCC, OP_FINAL_EXP, OP_MILLER, exe  # noqa: F401  (exe: the host build of the kernels' headers)

P, R = M.P, M.R
ONE_BYTES = M.to_bytes(M.ONE)


@pytest.fixture(scope="module")
def cap():
    return DC.parse()


@pytest.fixture(scope="module")
def miller(cap):
    """the model's unreduced Miller value of the captured pair, computed once"""
    return M.miller_loop(cap.g1_0, cap.g2_0)


# ---------------------------------------------------------------- 1. the fixture and its structure
def test_fixture_is_the_recorded_slice():
    data = DC.read()
    assert len(data) == DC.LENGTH == 17904 == VM.serialized_len(DC.K)
    assert hashlib.sha256(data).hexdigest() == DC.SHA256


def test_structural_facts(cap):
    data = cap.raw
    # every Fp component canonical: the 5 * 9 * 12 = 540 of the vectors and ht's twelve
    gts = [b for name in DC.VECTORS for b in getattr(cap, name + "_bytes")] + [cap.ht_bytes]
    comps = [int.from_bytes(b[32 * i:32 * i + 32], "little") for b in gts for i in range(12)]
    assert len(comps) == 540 + 12 and all(c < P for c in comps)
    # the copies and the ones of fromSRS (:889-973)
    assert cap.delta_1l_bytes == cap.delta_2l_bytes
    assert cap.delta_1l_bytes[0] == cap.delta_1r_bytes[0] == cap.delta_2r_bytes[0] == ONE_BYTES
    assert all(cap.delta_1l_bytes[k] == cap.chi_bytes[k - 1] for k in range(1, DC.K + 1))
    assert cap.h1_bytes == cap.g1_0_bytes and cap.h2_bytes == cap.g2_0_bytes and cap.ht_bytes == cap.chi_bytes[0]
    assert cap.max_log_n == 2 * DC.K == 16 and int.from_bytes(data[17896:], "little") == 16
    assert data[DC.POINTS_AT:17896] == cap.g1_0_bytes + cap.g2_0_bytes + cap.h1_bytes + cap.h2_bytes + cap.ht_bytes
    # the parser's two forms say the same, and parsing loses nothing
    for name in DC.VECTORS:
        assert M.gt_unpack(getattr(cap, name + "_words")) == getattr(cap, name)
        assert [M.to_bytes(g) for g in getattr(cap, name)] == getattr(cap, name + "_bytes")
    # the points are on their curves, no identities, and none of the four is a group generator
    assert cap.g1_0 is not None and (cap.g1_0[1] ** 2 - cap.g1_0[0] ** 3 - 3) % P == 0
    assert cap.g2_0 is not None and G2.is_on_curve(cap.g2_0)
    assert cap.g1_0 != M.G1_GEN and cap.g2_0 != G2.G and cap.h1 == cap.g1_0 and cap.h2 == cap.g2_0
    vals, words = DC.gt_values(cap)
    assert len(vals) == 41 and words.shape == (41, 48) and len({M.to_bytes(v) for v in vals}) == 25


def test_chi0_is_in_gt(cap):
    chi0 = cap.chi[0]
    assert M.power(chi0, R) == M.ONE and M.mul(chi0, M.conj(chi0)) == M.ONE and chi0 != M.ONE


# ---------------------------------------------------------------- 2. decompression
def test_sign_flags_follow_the_reference_orderings(cap):
    """bit 63 is set exactly when y is not lexicographically less than -y — for G2 under lexicographicallyLessFp2, c1 before c0 (whether
    THAT root is the reference's is test_model_pairing_is_chi0's: only one root pairs to chi[0])"""
    g1_flag = bool(cap.g1_0_bytes[31] & 0x80)
    g2_flag = bool(cap.g2_0_bytes[63] & 0x80)
    y = cap.g1_0[1]
    assert g1_flag == (not y < -y % P)
    y = cap.g2_0[1]
    ny = G2.f2_neg(y)
    assert g2_flag == (not (y[1], y[0]) < (ny[1], ny[0]))
    # what this one real point can and cannot tell: c1 decides (it differs from its negation), and both components lie in the upper
    # half, so a rule that compared c0 FIRST would set the same bit here — the component order rests on the reading of :1141-1166 and on
    # the constructed points of test_decompression_on_constructed_points, the polarity of the bit on the reference's bytes
    assert y[1] != ny[1] and y[1] > (P - 1) // 2 and y[0] > (P - 1) // 2 and g2_flag and not g1_flag
    assert g2_flag == (not DC.lexicographically_less_fp2(y, ny)) == (not VM.lexicographically_less_fp2(y, ny))
    assert not cap.g1_0_bytes[31] & 0x40 and not cap.g2_0_bytes[63] & 0x40
    # flip=True is the other root with the same x
    assert DC.decompress_g1(cap.g1_0_bytes, flip=True) == M.g1_neg(cap.g1_0)
    assert DC.decompress_g2(cap.g2_0_bytes, flip=True) == G2.neg(cap.g2_0)


def test_identity_encodings_on_constructed_bytes():
    from zolt_amd import api
    id1 = bytes(24) + (0x4000000000000000).to_bytes(8, "little")
    id2 = bytes(56) + (0x4000000000000000).to_bytes(8, "little")
    assert DC.decompress_g1(id1) is None and DC.decompress_g2(id2) is None
    assert id1 == VM.serialize_g1(None) == api.serializeG1(np.zeros(8, dtype=np.uint64), 1)
    assert id2 == VM.serialize_g2(None) == api.serializeG2(api.g2_identity(), 1)
    for bad in (bytes([1]) + id1[1:], id1[:31] + bytes([0xC0])):  # bit 62 with anything else beside it
        with pytest.raises(AssertionError):
            DC.decompress_g1(bad)
    for bad in (bytes([1]) + id2[1:], id2[:32] + bytes([1]) + id2[33:], id2[:63] + bytes([0xC0])):
        with pytest.raises(AssertionError):
            DC.decompress_g2(bad)
    with pytest.raises(AssertionError):  # x = 4: 67 is no square, not a point's x
        DC.decompress_g1((4).to_bytes(32, "little"))
    with pytest.raises(AssertionError):  # non-canonical x
        DC.decompress_g1((P + 1).to_bytes(32, "little"))


def test_decompression_on_constructed_points():
    """both signs of a few multiples of the generators through the model's and the Python mirror's serialisers and back; the Fp2 root's
    branches (a1 = 0 with a0 a square and not) on constructed squares"""
    from zolt_amd import api
    half, mixed = (P - 1) // 2, 0
    for k in (1, 2, 3, 0xD0C1):
        for p in (M.g1_mul(M.G1_GEN, k), M.g1_neg(M.g1_mul(M.G1_GEN, k))):
            b = VM.serialize_g1(p)
            assert DC.decompress_g1(b) == p and api.serializeG1(M.g1_pack([p])[0][0], 0) == b
            assert bool(b[31] & 0x80) == (p[1] > half)
        for q in (G2.scalar_mul(G2.G, k), G2.neg(G2.scalar_mul(G2.G, k))):
            b = VM.serialize_g2(q)
            assert DC.decompress_g2(b) == q and api.serializeG2(G2.pack([q])[0][0], 0) == b
            assert bool(b[63] & 0x80) == (q[1][1] > half)  # c1 decides when it is not zero
            mixed += (q[1][0] > half) != (q[1][1] > half)
    assert mixed  # points on which comparing c0 first would set the other bit are among them
    for a in ((4, 0), (P - 4, 0), (0, 0), (0, 2), (5, 0), (3, 4)):
        y = DC.f2_sqrt(G2.f2_sqr(a))
        assert y is not None and G2.f2_sqr(y) == G2.f2_sqr(a)
    assert DC.f2_sqrt(M.XI) is None  # xi = 9 + u is no square (it is a sextic non-residue)


# ---------------------------------------------------------------- 3. the models on the reference's pairing value
def test_model_pairing_is_chi0(cap, miller):
    """e(g1_0, g2_0) = chi[0] in all 384 bytes with the signs the flags name. A pairing only sees the product of the two signs
    (e(-P, -Q) = e(P, Q)), so of the other three choices the two with ONE sign flipped give conj(chi[0]) != chi[0]; each flag on its own
    is pinned by the serialiser round trips below."""
    p, q = cap.g1_0, cap.g2_0
    chi0 = cap.chi_bytes[0]
    assert M.to_bytes(M.pairing(p, q)) == chi0 == cap.ht_bytes
    neg_p, neg_q = M.g1_neg(p), G2.neg(q)
    e_np_q, e_p_nq, e_np_nq = M.pairing(neg_p, q), M.pairing(p, neg_q), M.pairing(neg_p, neg_q)
    assert M.to_bytes(e_np_q) != chi0 and M.to_bytes(e_p_nq) != chi0
    assert M.to_bytes(e_np_q) == M.to_bytes(e_p_nq) == M.to_bytes(M.conj(cap.chi[0]))
    assert M.to_bytes(e_np_nq) == chi0
    assert [M.to_bytes(e) == chi0 for e in (e_np_q, e_p_nq, e_np_nq)] == [False, False, True]  # the other three do not all match


def test_model_sub_steps(cap, miller):
    assert M.to_bytes(M.final_exponentiation(miller)) == cap.chi_bytes[0]
    assert M.to_bytes(M.multi_pairing([cap.g1_0], [cap.g2_0])) == cap.chi_bytes[0]
    assert M.to_bytes(VM.multi_pair([cap.g1_0], [cap.g2_0])) == cap.chi_bytes[0]
    vs = VM.from_srs([cap.g1_0], [cap.g2_0])  # K = 0
    assert VM.serialize(vs)[-(DC.LENGTH - DC.POINTS_AT):-8] == cap.raw[DC.POINTS_AT:17896] and vs.max_log_n == 0


def test_wave_restatement(cap, miller):
    got = W.miller_loop(cap.g1_0, cap.g2_0)
    assert got == miller
    assert M.to_bytes(W.final_exponentiation(got)) == cap.chi_bytes[0]
    assert W.final_exponentiation(M.ZERO) == M.ONE


def test_gt_membership_of_all_41_values(cap):
    """unitary (so that the inverse is the conjugate) and of order r — each distinct value once, the 41 are 25 values"""
    vals, _ = DC.gt_values(cap)
    seen = {}
    for g in vals:
        key = M.to_bytes(g)
        if key not in seen:
            seen[key] = M.inv(g) == M.conj(g) and M.power(g, R) == M.ONE and g != M.ONE
        assert seen[key]
    assert len(seen) == 25


# ---------------------------------------------------------------- 4. the kernels' own headers on the host
def _host_words(exe, op, rec):  # noqa: F811
    """one 96-word record -> the 48 words the lane wrote, as they are (no reduction on the way)"""
    rec = np.ascontiguousarray(rec, dtype=np.uint64).reshape(1, 96)
    res = subprocess.run([exe], input=b"%d 1\n" % op + rec.tobytes(), capture_output=True, check=True)
    return np.frombuffer(res.stdout, dtype=np.uint64).reshape(48)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")
def test_host_compiled_kernels_give_chi0(cap, miller, exe):  # noqa: F811
    """pair_miller then pair_final_exp of pairing.hip.h / fp12.hip.h, one lane's code compiled for the host, on the reference's pair"""
    rec = np.zeros(96, dtype=np.uint64)
    rec[:8] = M.g1_pack([cap.g1_0])[0][0]
    rec[8:24] = G2.pack([cap.g2_0])[0][0]
    mil = _host_words(exe, OP_MILLER, rec)
    assert np.array_equal(mil, M.gt_pack([miller])[0])
    rec = np.zeros(96, dtype=np.uint64)
    rec[:48] = mil
    assert np.array_equal(_host_words(exe, OP_FINAL_EXP, rec), cap.chi_words[0])
    rec[:8] = M.g1_pack([M.g1_neg(cap.g1_0)])[0][0]  # one sign flipped: the conjugate, not chi[0]
    rec[8:24] = G2.pack([cap.g2_0])[0][0]
    rec[24:] = 0
    rec[:48] = _host_words(exe, OP_MILLER, rec)
    assert np.array_equal(_host_words(exe, OP_FINAL_EXP, rec), M.gt_pack([M.conj(cap.chi[0])])[0])


# ---------------------------------------------------------------- 5. the serialisers on the whole 17 904 bytes
def _python_setup(cap, g1=None, g2=None):
    from zolt_amd import api
    g1 = cap.g1_0 if g1 is None else g1
    g2 = cap.g2_0 if g2 is None else g2
    return api.DoryVerifierSetup(cap.chi_words, cap.delta_1r_words, cap.delta_2r_words, (M.g1_pack([g1])[0][0], 0), (G2.pack([g2])[0][0], 0))


def test_python_mirror_round_trip(cap):
    from zolt_amd import api
    got = _python_setup(cap).serialize()
    assert len(got) == DC.LENGTH and got == cap.raw
    # the pieces on their own: gtToBytes / gt_to_bytes on reference values, the point encodings with the reference's flags
    assert [api.gtToBytes(w) for w in cap.chi_words] == cap.chi_bytes == [api.gt_to_bytes(w) for w in cap.chi_words]
    assert api.serializeG1(M.g1_pack([cap.g1_0])[0][0], 0) == cap.g1_0_bytes
    assert api.serializeG2(G2.pack([cap.g2_0])[0][0], 0) == cap.g2_0_bytes
    # either point's other root changes exactly the flag bit, so the comparison sees each sign on its own
    for kw, at in (({"g1": M.g1_neg(cap.g1_0)}, (DC.POINTS_AT + 31, DC.POINTS_AT + 96 + 31)), ({"g2": G2.neg(cap.g2_0)}, (DC.POINTS_AT + 95, DC.POINTS_AT + 96 + 95))):
        other = _python_setup(cap, **kw).serialize()
        assert [i for i in range(DC.LENGTH) if other[i] != cap.raw[i]] == list(at)
        assert all(other[i] ^ cap.raw[i] == 0x80 for i in at)


def test_model_serialiser_round_trip(cap):
    vs = VM.VerifierSetup(delta_1l=cap.delta_1l, delta_1r=cap.delta_1r, delta_2l=cap.delta_2l, delta_2r=cap.delta_2r, chi=cap.chi,
                          g1_0=cap.g1_0, g2_0=cap.g2_0, h1=cap.h1, h2=cap.h2, ht=cap.ht, max_log_n=cap.max_log_n)
    assert VM.serialize(vs) == cap.raw
    assert VM.serialize_g1(cap.g1_0) == cap.g1_0_bytes and VM.serialize_g2(cap.g2_0) == cap.g2_0_bytes
    assert VM.serialize_gt(cap.ht) == cap.ht_bytes


def test_the_fixture_needs_no_reference_tree(monkeypatch):
    """the tests read the committed slice only: a ZOLT_REFERENCE that points nowhere changes nothing"""
    monkeypatch.setenv("ZOLT_REFERENCE", os.path.join(os.sep, "nonexistent", "reference"))
    assert hashlib.sha256(DC.parse().raw).hexdigest() == DC.SHA256
