"""The launch shapes that the library chooses from the problem size, at sizes the suite can afford.

Several kernels pick workgroup template, rows per workgroup, grid cap or window width from the size, and a suite of small sizes runs the
small-size shapes only. Here every size-gated shape runs at the smallest size that still has it:

  * eq table, expanding eq table, fused Spartan open, fold / sums and the 256-thread pair-sum kernels, the Stage-4 and product-form
    sessions: under the switches of docs/design/08_switches.md, which are read once per process — a fresh child per switch set,
    tests/launch_shapes_check.py (it has the sets, the shapes and the checks);
  * the G1 fixed base at every window width, in this process (ZG_FB_WINDOW_BITS is read per call).

Every case asserts through zg_selftest_launch_shape that the library would launch the shape it was written for before it compares
results; the comparisons are bit for bit against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import launch_shapes_check as child
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(child.SETS))
def test_shapes_forced_by_switches(name):
    env = dict(os.environ, PYTHONPATH=ROOT, **child.SETS[name]["env"])
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_shapes_check.py"), name], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    print(res.stdout[-6000:])  # one line per check
    assert res.returncode == 0 and "launch shapes ok" in res.stdout, res.stdout[-3000:] + res.stderr[-4000:]


@pytest.fixture(scope="module")
def env():
    from oracle import binding as ob
    from zolt_amd import api, lib
    lib.init()
    return api, lib, ob


FB_WIDTHS = [4, 5, 8, 10, 11, 14]


def _fb_scalars(api):
    """the integers whose windows go wrong first: the ends of the field, every single bit and every run of low bits, every digit at its
    largest for each width, only the top window populated, and 64 uniform ones"""
    R = api.R_MOD
    ks = [0, 1, R - 1, R - 2, (1 << 253) - 1]
    ks += [1 << k for k in range(254)] + [(1 << k) - 1 for k in range(254)]
    for c in FB_WIDTHS:
        W = (254 + c - 1) // c
        top_bits = 254 - c * (W - 1)  # bits of r that the top window holds
        v = (1 << (c * W)) - 1        # every digit 2^c - 1 ...
        while v >= R:                 # ... and the largest such value below r: lower the top digit
            v -= 1 << (c * (W - 1))
        ks += [v, (R >> (c * (W - 1))) << (c * (W - 1)), 1 << (c * (W - 1)), ((1 << (top_bits - 1)) - 1) << (c * (W - 1))]
    ks = [k % R for k in ks]
    uniform = [U.fr_to_int(x) % R for x in U.random_raw256(4300, 64)]
    return ks + uniform


@pytest.fixture(scope="module")
def fb_reference(env):
    """the scalars and, once for every width, their products with the generator by the per-pair scalarMul kernel (pinned on the oracle
    in tests/test_gpu_g2.py), 16 of them by the oracle itself"""
    api, lib, ob = env
    g = api.generator()
    ks = _fb_scalars(api)
    sc = np.stack([api.fr_from_int(k) for k in ks])
    n = len(ks)
    want = lib.g1_scalar_mul_batch(np.repeat(g[None, :], n, axis=0), np.zeros(n, dtype=np.uint8), sc)
    picks = [0, 1, 2, 3, 4, 5 + 253, 5 + 254 + 253, 5 + 508, 5 + 508 + 1, 5 + 508 + 4 * 3, 5 + 508 + 4 * 4 + 3, 5 + 508 + 4 * 5, n - 64, n - 1, 100, 400]
    for i in picks:
        o, oi = ob.g1_scalar_mul(g, 0, sc[i])
        assert want[1][i] == oi and (oi or np.array_equal(want[0][i], o)), i
    assert want[1][0] == 1 and want[1][1:5].sum() == 0
    return g, sc, want


@pytest.mark.parametrize("c", FB_WIDTHS)
def test_fixed_base_at_every_window_width(env, fb_reference, c, monkeypatch):
    """zg_g1_fixed_base_mul_batch under every accepted window width — 4 (64 windows, the widest launch of the window-base kernel), 8,
    10 and 11 (the widths of real keys; for 10 and 11 the top window shifts in past the scalar's last limb), 14 (the widest) — all
    outputs and flags against zg_g1_scalar_mul_batch; once with a base other than the generator"""
    api, lib, ob = env
    g, sc, (wxy, winf) = fb_reference
    monkeypatch.setenv("ZG_FB_WINDOW_BITS", str(c))
    W = (254 + c - 1) // c
    assert lib.launch_shape(lib.SHAPE_FB, len(sc))[:3] == (c, W, (1 << c) - 1)
    xy, inf = lib.g1_fixed_base_mul_batch(g, sc)
    assert np.array_equal(inf, winf) and np.array_equal(xy, wxy)
    if c == 11:
        base = wxy[77]
        m = 96
        xy2, inf2 = lib.g1_fixed_base_mul_batch(base, sc[:m])
        w2, wi2 = lib.g1_scalar_mul_batch(np.repeat(base[None, :], m, axis=0), np.zeros(m, dtype=np.uint8), sc[:m])
        assert np.array_equal(inf2, wi2) and np.array_equal(xy2, w2)


@pytest.mark.parametrize("c", [10, 11])
def test_hyperkzg_setup_at_the_window_widths_of_real_keys(env, c, monkeypatch):
    """zg_hyperkzg_setup of 257 powers with the 10- and 11-bit windows that keys of more than 2^15 and 2^18 powers get: every point
    against the oracle's generateMockSRS restatement"""
    api, lib, ob = env
    n = 257
    monkeypatch.setenv("ZG_FB_WINDOW_BITS", str(c))
    assert lib.launch_shape(lib.SHAPE_FB, n)[:2] == (c, (254 + c - 1) // c)
    h, xy, inf = lib.Bases.hyperkzg_setup(api.generator(), api.fr_from_int(api.HyperKZG.TAU), n)
    h.free()
    want, winf = ob.hyperkzg_setup(n)
    assert np.array_equal(xy, want) and not inf.any() and not np.asarray(winf).any()


def test_default_window_widths_by_batch_size(env):
    """without the switch: 8 bits up to 2^15 outputs, 10 up to 2^18, 11 beyond"""
    api, lib, ob = env
    assert "ZG_FB_WINDOW_BITS" not in os.environ
    for n, c in ((1, 8), (1 << 15, 8), ((1 << 15) + 1, 10), (1 << 18, 10), ((1 << 18) + 1, 11), (1 << 24, 11)):
        assert lib.launch_shape(lib.SHAPE_FB, n)[:2] == (c, (254 + c - 1) // c), n
