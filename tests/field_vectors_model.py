"""The model of the section "field vectors (device)" (include/zolt_gpu.h): field.BatchOps (src/field/mod.zig:1164-1280) over Python
integers mod r and mod p, the vectors the CPU and GPU tests share, and the host harness of the lane functions
(tests/cpp/field_vec_host.cpp, zolt_amd/csrc/field_vec.hip.h). Used by tests/test_field_vectors_model.py and
tests/test_gpu_field_vectors.py."""
import os
import random
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
FR, FP = 0, 1
MODS = (R, P)
NAMES = ("fr", "fp")
MONT = 1 << 256
_M64 = (1 << 64) - 1


def internal_constants():
    """ZG_FV_E and ZG_FV_TILE as include/zolt_gpu_internal.h states them (the tests take their sizes from there)"""
    text = open(os.path.join(ROOT, "include", "zolt_gpu_internal.h")).read()
    e = int(re.search(r"#define ZG_FV_E (\d+)", text).group(1))
    tile = int(re.search(r"#define ZG_FV_TILE (\d+)", text).group(1))
    assert tile == 256 * e
    return e, tile


E, TILE = internal_constants()


# ---- representation: canonical integers <-> (n, 4) uint64 Montgomery limbs
def to_limbs(values, mod):
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = v % mod * MONT % mod
        out[i] = [(m >> (64 * k)) & _M64 for k in range(4)]
    return out


def from_limbs(limbs, mod):
    rinv = pow(MONT, -1, mod)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) * rinv % mod for row in np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)]


# ---- BatchOps on integers
def inner_product(a, b, mod):
    assert len(a) == len(b)
    return sum(x * y for x, y in zip(a, b)) % mod


def horner(coeffs, x, mod):
    """hornerEval (:1217-1227)"""
    if not coeffs:
        return 0
    result = coeffs[-1]
    for c in reversed(coeffs[:-1]):
        result = (result * x + c) % mod
    return result


def batch_inverse(a, mod):
    """what the entry points compute: the element-wise value, zero only where the input is zero"""
    return [pow(v, -1, mod) if v else 0 for v in a]


def reference_batch_inverse(a, mod):
    """BatchOps.batchInverse (:1232-1273) restated line by line"""
    n = len(a)
    results = [None] * n
    if n == 0:                                                   # :1234
        return results
    products = [None] * n
    products[0] = a[0]                                           # :1241 (no zero guard)
    for i in range(1, n):                                        # :1242
        if a[i] == 0:                                            # :1243
            products[i] = products[i - 1]                        # :1245
        else:
            products[i] = products[i - 1] * a[i] % mod           # :1247
    all_inv = pow(products[n - 1], -1, mod) if products[n - 1] else 0  # :1252 inverse() orelse zero
    running_inv = all_inv                                        # :1255
    i = n                                                        # :1256
    while i > 1:                                                 # :1257
        i -= 1
        if a[i] == 0:                                            # :1259
            results[i] = 0
        else:
            results[i] = running_inv * products[i - 1] % mod     # :1263
            running_inv = running_inv * a[i] % mod               # :1264
    results[0] = 0 if a[0] == 0 else running_inv                 # :1268-1272
    return results


# ---- the generator: vectors by name, the same for every test that names them
def edge_values(mod):
    return [1, mod - 1, 2, (mod + 1) // 2, 3, mod - 2, (1 << 255) % mod,(1 << 64) - 1]


def random_values(mod, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, mod) for _ in range(n)]


def zero_patterns(n, e=None):
    """name -> positions of zeros in a vector of n elements: none, the first, the last, one in every position of a lane's group, a whole
    group, alternating, every element"""
    e = e or E
    pats = {"none": [], "first": [0], "last": [n - 1], "alternating": list(range(0, n, 2)), "odd": list(range(1, n, 2)), "all": list(range(n)),
            "all_but_first": list(range(1, n)), "all_but_last": list(range(n - 1))}
    for k in range(min(e, n)):
        pats[f"slot{k}"] = [k]
    if n >= 2 * e:
        pats["group"] = list(range(e, 2 * e))
        pats["first_group"] = list(range(e))
    return pats


def generator_vectors(mod, seed=2028, lengths=(1, 2, 3, 5, 8, 9, 17)):
    """[(name, values)]: random and edge values under every zero pattern, at a few lengths"""
    out = []
    for n in lengths:
        base = (edge_values(mod) + random_values(mod, n, seed + n))[:n] if n >= 8 else random_values(mod, n, seed + n)
        for name, zeros in zero_patterns(n).items():
            v = list(base)
            for z in zeros:
                v[z] = 0
            out.append((f"n{n}_{name}", v))
    return out


# ---- the host harness of the lane functions
OP_INV_GROUPS, OP_HORNER_CHUNKS, OP_HORNER = 0, 1, 2


def compile_host(exe, extra=()):
    """tests/cpp/field_vec_host.cpp built for the CPU -> run(field, op, limbs, x=None) -> (m, 4) uint64"""
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *extra, "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "field_vec_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)

    def run(field, op, limbs, x=None):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
        xw = np.zeros(4, dtype=np.uint64) if x is None else np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
        res = subprocess.run([exe], input=f"{field} {op} {len(limbs)}\n".encode() + xw.tobytes() + limbs.tobytes(), capture_output=True, check=True)
        return np.frombuffer(res.stdout, dtype=np.uint64).reshape(-1, 4)

    return run
