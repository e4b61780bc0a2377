"""The model of Dory's opening proof (tests/dory_open_model.py) and the host-side wire forms, CPU only: compressG1 against its definition
(src/poly/commitment/dory.zig:51-78, yIsPositive :162-177) and its inverse, the GT appender (src/transcripts/blake2b.zig:496-522), the
length of DoryProof.toBytes (:481-535), and bilinearity of the model's first-round products — a check no device code shares."""
import random

import numpy as np
import pytest

from tests import dory_open_model as D
from tests import g2_model as G2
from tests import pairing_model as PM

P, R = D.P, D.R


@pytest.fixture(scope="module")
def run22():
    inp = D.make_inputs(2, 2, seed=2202, zero_v=(1,))
    return inp, D.run_model(inp, D.Transcript(b"Jolt"))


def _points_with_both_signs():
    rng = random.Random(9)
    pts = [PM.g1_mul(PM.G1_GEN, rng.randrange(1, R)) for _ in range(6)]
    pts += [PM.g1_neg(p) for p in pts]
    assert any(p[1] <= (-p[1]) % P for p in pts) and any(p[1] > (-p[1]) % P for p in pts)
    return pts


def test_compress_g1_follows_its_definition_and_round_trips():
    from zolt_amd import api
    assert D.compress_g1(None) == bytes(31) + b"\x40"
    gen = D.compress_g1(PM.G1_GEN)
    assert gen == (1).to_bytes(32, "little")  # y = 2 <= p - 2: positive, no flag
    assert D.compress_g1(PM.g1_neg(PM.G1_GEN))[31] == 0x80 and D.compress_g1(PM.g1_neg(PM.G1_GEN))[:31] == gen[:31]
    for p in [PM.G1_GEN] + _points_with_both_signs():
        b = D.compress_g1(p)
        x = int.from_bytes(b[:31] + bytes([b[31] & 0x3F]), "little")
        assert x == p[0] and (b[31] & 0x40) == 0
        assert bool(b[31] & 0x80) == (p[1] > P - p[1])  # YIsNegative exactly when y is the larger of (y, -y)
        assert D.decompress_g1(b) == p
        xy, inf = PM.g1_pack([p])
        assert api.compressG1(xy[0], int(inf[0])) == b  # the package's mirror
    assert D.decompress_g1(D.compress_g1(None)) is None
    assert api.compressG1(np.zeros(8, dtype=np.uint64), 1) == D.compress_g1(None)


def test_compress_g2_mirror_agrees_with_the_model():
    from zolt_amd import api
    rng = random.Random(10)
    pts = [G2.scalar_mul(G2.G, rng.randrange(1, R)) for _ in range(4)]
    pts += [G2.neg(p) for p in pts] + [None]
    xy, inf = G2.pack(pts)
    assert [api.compressG2(xy[i], int(inf[i])) for i in range(len(pts))] == [G2.compress(p) for p in pts]


def test_append_gt_is_the_reversed_serialisation(run22):
    from zolt_amd import api
    f = PM.gt_unpack(run22[1]["vmv"][:48])[0]
    raw = PM.to_bytes(f)
    assert len(raw) == 384 and raw != raw[::-1]
    a, b = D.Transcript(b"Jolt"), D.Transcript(b"Jolt")
    a.appendGT(f)
    b.appendBytes(raw[::-1])
    assert a.state == b.state and a.n_rounds == 1
    c, d = api.Blake2bTranscript(b"Jolt"), api.Blake2bTranscript(b"Jolt")
    c.appendGT(run22[1]["vmv"][:48])
    d.appendBytes(raw[::-1])
    assert c.state == d.state == a.state
    assert api.gtToBytes(run22[1]["vmv"][:48]) == raw
    # the compressed appenders are NOT reversed
    e1 = D.g1_point(run22[1]["vmv"][96:105])
    a.appendG1Compressed(e1)
    c.appendG1Compressed((run22[1]["vmv"][96:104], int(run22[1]["vmv"][104])))
    b.appendBytes(D.compress_g1(e1))
    assert a.state == b.state == c.state
    q = D.g2_point(run22[1]["first"][0][201:218])
    a.appendG2Compressed(q)
    c.appendG2Compressed((run22[1]["first"][0][201:217], int(run22[1]["first"][0][217])))
    b.appendBytes(G2.compress(q))
    assert a.state == b.state == c.state
    assert np.array_equal(a.challengeScalar(), c.challengeScalar())


def test_proof_length_and_layout(run22):
    from zolt_amd import api
    inp, out = run22
    sigma = inp["sigma"]
    assert len(out["proof"]) == 800 + 4 + sigma * (1632 + 960) + 96 + 8
    assert out["proof"][800:804] == sigma.to_bytes(4, "little") and out["proof"][-8:] == (2).to_bytes(4, "little") + sigma.to_bytes(4, "little")
    assert [m.shape for m in out["first"]] == [(218,)] * sigma and [m.shape for m in out["second"]] == [(148,)] * sigma
    assert out["vmv"].shape == (105,) and out["final"].shape == (26,)
    # the package's serialiser over the same records
    assert api.DoryProof(out["vmv"], out["first"], out["second"], out["final"], inp["nu"], sigma).toBytes() == out["proof"]


def test_first_round_products_are_bilinear(run22):
    """d1_left * d1_right = prod_i e(v1[i], g2_vec[i mod n2]) (:1549-1550), and with v1[i] = k_i G that is e(G, sum_i k_i g2_vec[i mod n2])"""
    inp, out = run22
    d1_left, d1_right, v1_pts, g2 = out["first_round"]
    n2 = len(v1_pts) // 2
    assert PM.mul(d1_left, d1_right) == PM.multi_pairing(v1_pts, g2[:n2] + g2[:n2])
    ks = inp["row_ks"]
    assert v1_pts == [PM.g1_mul(PM.G1_GEN, k) for k in ks]
    assert PM.mul(d1_left, d1_right) == PM.pairing(PM.G1_GEN, G2.msm(g2[:n2] + g2[:n2], ks))


def test_vmv_message_is_bilinear_in_the_row_commitments(run22):
    """c = e(MSM(rows, v_vec), g2_vec[0]) = e(G, g2_vec[0]) ^ (sum k_i v_i): the same value through one G2 scalar multiplication"""
    inp, out = run22
    s = sum(k * v for k, v in zip(inp["row_ks"], inp["v_vec"])) % R
    assert PM.gt_unpack(out["vmv"][:48])[0] == PM.pairing(PM.G1_GEN, G2.scalar_mul(inp["g2_pts"][0], s))
