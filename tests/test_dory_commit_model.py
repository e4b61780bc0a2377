"""tests/dory_commit_model.py held to tests/pairing_model.py and to itself (CPU): the reference's commit as row MSMs and a multi-pairing
against the closed form over keys with known discrete logarithms, the three polynomial kinds, the layout edges, setup's rule — and the
library's new section as far as it can be seen without a GPU: exported, announced, and refusing to compute."""
import ctypes as C
import hashlib
import os
import random

import numpy as np

from tests import dory_commit_model as DM
from tests import g2_model as G2
from tests import pairing_model as PM

R = DM.R


def _key(rng, cols, rows):
    a = [rng.randrange(1, R) for _ in range(cols)]
    b = [rng.randrange(1, R) for _ in range(rows)]
    return a, b, DM.g1_from_scalars(a), DM.g2_from_scalars(b)


def test_commit_is_the_multi_pairing_of_its_rows_and_the_closed_form_at_two_and_four_rows():
    rng = random.Random(1)
    a, b, g1, g2 = _key(rng, 4, 4)
    for n in (8, 16):  # sigma = 2: two rows; sigma = 2, nu = 2: four rows
        vals = [rng.randrange(R) for _ in range(n)]
        rows = DM.row_commitments(g1, vals)
        assert len(rows) == n // 4 and rows == [PM.g1_mul(PM.G1_GEN, e) for e in DM.row_exponents(a, vals)]
        direct = PM.multi_pairing(rows, g2[:len(rows)])
        assert DM.commit(g1, g2, vals) == direct == DM.commit_closed_form(a, b, vals)
    # the closed form is the pairing's bilinearity, not a restatement of the model: e(a G1, b G2) = e(G1, G2)^(a b)
    assert PM.pairing(g1[1], g2[2]) == PM.power(DM.e_gen(), a[1] * b[2] % R)


def test_layout_edges():
    assert [DM.layout(n) for n in (1, 2, 3, 8, 11, 1 << 13, 1 << 14)] == [(1, 1, 0, 1), (1, 1, 0, 2), (1, 1, 0, 2), (3, 2, 1, 8), (3, 2, 1, 8),
                                                                          (13, 7, 6, 1 << 13), (14, 7, 7, 1 << 14)]
    assert DM.matrix([]) == [] and DM.matrix([5]) == [[5]] and DM.matrix([5, 6, 7]) == [[5, 6]]
    assert DM.matrix(list(range(11))) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    rng = random.Random(2)
    a, b, g1, g2 = _key(rng, 4, 2)
    assert DM.commit(g1, g2, []) == PM.ONE == DM.commit_closed_form(a, b, [])
    for n in (1, 2, 3, 8, 11):
        vals = [rng.randrange(R) for _ in range(n)]
        assert DM.commit(g1, g2, vals) == DM.commit_closed_form(a, b, vals), n
    # rows past g2_vec are left out (:1030); an identity generator contributes nothing
    vals = [rng.randrange(R) for _ in range(8)]
    assert DM.commit(g1, g2[:1], vals) == DM.commit_closed_form(a, b[:1], vals) == PM.pairing(DM.row_commitments(g1, vals)[0], g2[0])
    assert DM.commit([g1[0], None, g1[2], g1[3]], g2, vals) == DM.commit_closed_form([a[0], 0, a[2], a[3]], b, vals)
    assert DM.commit(g1, g2, [0] * 8) == PM.ONE


def test_the_three_kinds():
    m64 = (1 << 64) - 1
    assert DM.values_u64([5, 0, m64, 7], [0, 1, 1, 1]) == [5, 0, R - m64, R - 7] and DM.values_u64([3, 4]) == [3, 4]
    e = (0xAB << 60) | (0xF << 124) | 0x3
    assert DM.values_chunk([e], 60, 8) == [0xAB] and DM.values_chunk([e], 124, 4) == [0xF] and DM.values_chunk([e], 0, 4) == [3]
    assert DM.values_chunk([m64], 56, 8) == [255] and DM.values_chunk([e], 64, 4) == [0xA]
    # InstructionRa[j][i] = (lookup_index[i] >> 4 (31 - j)) & 15: the 32 chunks put the index back together
    idx = random.Random(3).getrandbits(128)
    assert sum(DM.values_chunk([idx], 4 * (31 - j), 4)[0] << (4 * (31 - j)) for j in range(32)) == idx
    assert np.array_equal(DM.u128_pack([e]), np.array([[e & m64, e >> 64]], dtype=np.uint64))
    # a 64-bit polynomial is its eight byte polynomials under Horner: sum_w 2^(8 w) byte_w
    w = random.Random(4).getrandbits(64)
    assert sum(DM.values_chunk([w], 8 * k, 8)[0] << (8 * k) for k in range(8)) == w


def test_setup_rule():
    seed = hashlib.sha3_256(b"Jolt Dory URS seed").digest()
    for m in (1, 2, 3, 6, 13):
        sigma, nu, a, b = DM.setup_scalars(m)
        assert (sigma, nu, len(a), len(b)) == ((m + 1) // 2, m // 2, 1 << ((m + 1) // 2), 1 << (m // 2))
        assert a[1] == int.from_bytes(hashlib.sha3_256(seed + (1).to_bytes(8, "little") + b"G1").digest(), "little") % R
        assert b[0] == int.from_bytes(hashlib.sha3_256(seed + (1 << sigma).to_bytes(8, "little") + b"G2").digest(), "little") % R
    g1, g2 = DM.setup(3)
    _, _, a, b = DM.setup_scalars(3)
    assert len(g1) == 4 and len(g2) == 2 and all(PM.g1_add(PM.g1_neg(p), PM.g1_mul(PM.G1_GEN, s)) is None for p, s in zip(g1, a))
    assert all(G2.is_on_curve(q) for q in g2) and g2[1] == G2.scalar_mul(G2.G, b[1])
    from zolt_amd import api
    assert api.Dory.setupScalars(13) == DM.setup_scalars(13)


def test_the_library_exports_the_section_and_refuses_to_compute_without_a_device():
    from zolt_amd import _abi, lib
    names = ["zg_dory_key_create", "zg_dory_key_free", "zg_dory_key_len", "zg_dory_commit_batch", "zg_dory_commit_batch_dev"]
    assert all(n in lib.SYMBOLS and hasattr(lib._lib, n) for n in names)
    assert _abi.ZG_FEATURE_DORY_COMMIT == 64 and lib.abi_features() & 64 and lib.abi_version() == (1, 11)
    assert (_abi.ZG_DORY_POLY_FR, _abi.ZG_DORY_POLY_U64, _abi.ZG_DORY_POLY_CHUNK64, _abi.ZG_DORY_POLY_CHUNK128) == (0, 1, 2, 3)
    assert lib._lib.zg_dory_key_free(None) == lib.OK and lib._lib.zg_dory_key_len(None, None, None) == lib.ERR_INVALID
    if os.path.exists("/dev/kfd"):
        return  # a GPU is present: the no-device answers cannot be observed (tests/test_gpu_dory_commit.py runs the section instead)
    g1 = np.zeros((2, 8), dtype=np.uint64)
    h = C.c_void_p()
    assert lib._lib.zg_dory_key_create(g1.ctypes.data_as(C.c_void_p), None, 2, None, None, 0, C.byref(h)) == lib.ERR_NO_DEVICE and not h.value
    one = np.zeros(1, dtype=np.uint64)
    gt = np.zeros(48, dtype=np.uint64)
    for fn, extra in ((lib._lib.zg_dory_commit_batch, ()), (lib._lib.zg_dory_commit_batch_dev, (None,))):
        args = [None, 1, one.ctypes.data_as(C.c_void_p), None, None, one.ctypes.data_as(C.c_void_p), None, None, *extra, gt.ctypes.data_as(C.c_void_p), None, None]
        assert fn(*args) == lib.ERR_NO_DEVICE
    assert not gt.any()
