"""Big-integer restatement of DoryCommitmentScheme.commit and setup (src/poly/commitment/dory.zig:931-1042, 1675-1712) and of the three
polynomial kinds of zg_dory_commit_batch, for tests/test_dory_commit_model.py (CPU) and tests/test_gpu_dory_commit.py.

Two routes to a commitment: `commit` does what the reference does — row MSMs in G1, then tests/pairing_model.multi_pairing against g2_vec —
and is affordable at a handful of rows; `commit_closed_form` needs the discrete logarithms of the key (g1_vec[c] = a_c G1, g2_vec[r] =
b_r G2, which is how setup makes its generators) and is e(G1, G2)^(sum_r b_r sum_c a_c M[r][c] mod r): one model pairing (cached) and one
power, whatever the size."""
import functools
import hashlib

import numpy as np

from tests import g2_model as g2m
from tests import pairing_model as pm

R = g2m.R
URS_SEED = b"Jolt Dory URS seed"
KIND_FR, KIND_U64, KIND_CHUNK64, KIND_CHUNK128 = 0, 1, 2, 3


def layout(n):
    """(num_vars, sigma, nu, entries read) of a polynomial of n > 0 entries (:1002-1010)"""
    num_vars = 1 if n <= 1 else n.bit_length() - 1
    sigma = (num_vars + 1) // 2
    return num_vars, sigma, num_vars - sigma, (n if n <= 1 else 1 << num_vars)


def values_fr(ints):
    return [v % R for v in ints]


def values_u64(words, signs=None):
    """F.fromU64(word), negated where the sign byte is 1 (buildRdIncPolynomial / buildRamIncPolynomial); a negative zero is zero"""
    return [(-int(w)) % R if signs is not None and signs[i] else int(w) % R for i, w in enumerate(words)]


def values_chunk(entries, shift, bits):
    """(entry >> shift) & (2^bits - 1) of integer entries (64 or 128 bits wide)"""
    return [(int(e) >> shift) & ((1 << bits) - 1) for e in entries]


def matrix(values):
    """the rows the reference walks (:1015-1021): [] for an empty polynomial"""
    if not values:
        return []
    _, sigma, nu, read = layout(len(values))
    cols = 1 << sigma
    return [values[r * cols:min((r + 1) * cols, read)] for r in range(1 << nu) if r * cols < read]


def row_commitments(g1_vec, values):
    """[row MSM] as affine points or None; g1_vec: affine points or None"""
    out = []
    for row in matrix(values):
        acc = None
        for g, s in zip(g1_vec, row):
            if g is not None and s % R:
                acc = pm.g1_add(acc, pm.g1_mul(g, s % R))
        out.append(acc)
    return out


def commit(g1_vec, g2_vec, values):
    """commit (:989-1042): rows past g2_vec are left out (:1030)"""
    rows = row_commitments(g1_vec, values)
    n = min(len(rows), len(g2_vec))
    return pm.multi_pairing(rows[:n], g2_vec[:n])


@functools.lru_cache(maxsize=1)
def e_gen():
    return pm.pairing(pm.G1_GEN, g2m.G)


def exponent(a, b, values):
    """sum_r b_r sum_c a_c M[r][c] mod r over the rows that have a g2 generator"""
    total = 0
    for r, row in enumerate(matrix(values)):
        if r < len(b):
            total += b[r] * sum(ac * v for ac, v in zip(a, row))
    return total % R


def row_exponents(a, values):
    return [sum(ac * v for ac, v in zip(a, row)) % R for row in matrix(values)]


def commit_closed_form(a, b, values):
    return pm.power(e_gen(), exponent(a, b, values))


def setup_scalars(max_num_vars):
    """(sigma, nu, [a_c], [b_r]) of setup (:931-979): Fr.fromBytes(SHA3-256(seed || u64le(index) || tag)), G2 indices offset by 2^sigma"""
    sigma = (max_num_vars + 1) // 2
    nu = max_num_vars - sigma
    seed = hashlib.sha3_256(URS_SEED).digest()

    def scalar(index, tag):
        return int.from_bytes(hashlib.sha3_256(seed + index.to_bytes(8, "little") + tag).digest(), "little") % R

    cols = 1 << sigma
    return sigma, nu, [scalar(i, b"G1") for i in range(cols)], [scalar(i + cols, b"G2") for i in range(1 << nu)]


def setup(max_num_vars):
    """-> (g1_vec, g2_vec) as affine points"""
    _, _, a, b = setup_scalars(max_num_vars)
    return [pm.g1_mul(pm.G1_GEN, s) for s in a], [g2m.scalar_mul(g2m.G, s) for s in b]


def g1_from_scalars(a):
    return [pm.g1_mul(pm.G1_GEN, s % R) if s % R else None for s in a]


def g2_from_scalars(b):
    return [g2m.scalar_mul(g2m.G, s % R) if s % R else None for s in b]


def fr_pack(ints):
    return np.array([g2m.fr_limbs(v % R) for v in ints], dtype=np.uint64).reshape(-1, 4)


def u128_pack(entries):
    m = (1 << 64) - 1
    return np.array([[int(e) & m, int(e) >> 64] for e in entries], dtype=np.uint64).reshape(-1, 2)
