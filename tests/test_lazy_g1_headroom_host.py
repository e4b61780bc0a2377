"""The un-carried linear forms of the mixed addition on the CPU: tests/cpp/lazy_g1_headroom_host.cpp compiles the kernels' own headers
for the host (hipcc --offload-host-only, ZG_F29_SERIAL: the compiler forms of the products) and runs every record twice from one
binary — the addition with P, R and 4p - Y1 un-carried, as the accumulate loop has it, and the carried form it replaces. Required: the
two agree limb for limb, and both agree with the big-integer model (tests/lazy_model.py). The records are
tests/lazy_headroom_records.py, the ones the device test (tests/test_gpu_lazy_g1_headroom.py) uses. Run plain, and once more as a
stand-alone program under -fsanitize=address,undefined.

    python -m pytest tests/test_lazy_g1_headroom_host.py -q -s --durations=0        # about half a minute, the two compiles included"""
import os

import numpy as np
import pytest

from tests import lazy_headroom_records as hr
from tests import lazy_model as lm

pytestmark = pytest.mark.skipif(not os.path.exists(hr.HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

SEED = 20261


_compile = hr.host_harness


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("lazy_g1_headroom") / "host"))


@pytest.fixture(scope="module")
def madd():
    items = hr.madd_items(SEED, 3072)
    lm.assert_in_class(lm.MADD, items)
    return items


@pytest.fixture(scope="module")
def lin():
    return hr.lin_items(SEED, 2048)


def test_edge_records_are_what_they_claim(madd):
    kinds = {it[0] for it in madd}
    for want in ("x-limbs-max+", "x-limbs-max-", "x-limbs-max-double+", "x-limbs-max-double-", "x-limbs-max-infinity+", "row-x-all-ones+",
                 "row-y-all-ones-", "u2-all-ones+", "s2-all-ones-", "class-top+", "run-start-negated-", "run-start-y-2p+", "class-top-double-",
                 "regular+", "regular-", "double+", "double-", "infinity+", "infinity-", "forced-zz+", "forced-zzz-", "forced-y-2p+"):
        assert want in kinds, (want, sorted(kinds))
    for it in madd:
        rec = [int(x) for x in it[1]]
        if it[0].startswith("x-limbs-max"):
            assert rec[0] == lm.MASK and rec[1:8] == [lm.NEAR - 1] * 7
        if it[0].startswith("row-x-all-ones"):
            assert rec[36:44] == [lm.MASK] * 8
        if it[0].startswith("row-y-all-ones"):
            assert rec[45:53] == [lm.MASK] * 8
        if it[0].startswith(("u2-all-ones", "s2-all-ones")):
            w = 1 if it[0].startswith("s2") else 0
            prod = lm.val(rec[9 * (4 + w):9 * (5 + w)]) * lm.val(rec[9 * (2 + w):9 * (3 + w)]) * lm.MONT_INV % lm.P
            assert lm.limbs(prod)[:8] == [lm.MASK] * 8


def test_madd_uncarried_is_the_carried_addition(harness, madd):
    new, ref = harness(lm.MADD, madd)
    mx = hr.check_madd(madd, new, ref, device=False)
    exc = [int(o[144]) for o in new]
    print(f"madd: {len(madd)} records ({exc.count(2)} doublings, {exc.count(1)} to infinity), largest outputs / p: {dict(mx)}")
    assert exc.count(2) >= 20 and exc.count(1) >= 20


def test_start_uncarried_is_the_carried_addition(harness):
    items = lm.start_records(SEED + 2, 256)
    new, ref = harness(lm.START, items)
    assert np.array_equal(new, ref)
    lm.check(lm.START, items, new, device=False)


def test_raw_linear_forms_and_the_zero_test(harness, lin):
    new, ref = harness(lm.LIN, lin)
    hr.check_lin(lin, new, ref)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, madd, lin):
    """the same program built with -fsanitize=address,undefined: a signed overflow, a shift past a word's width or an index past an
    array in the un-carried path ends the run with a report"""
    run = _compile(str(tmp_path / "host_san"), extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    new, ref = run(lm.MADD, madd)
    hr.check_madd(madd, new, ref, device=False)
    new, ref = run(lm.LIN, lin)
    hr.check_lin(lin, new, ref)


def test_the_checks_can_fail(harness, madd, lin):
    new, ref = harness(lm.MADD, madd[:64])
    bad = new.copy()
    bad[3, 9] ^= np.uint32(1)
    with pytest.raises(AssertionError):
        hr.check_madd(madd[:64], bad, ref, device=False)
    new, ref = harness(lm.LIN, lin)
    bad = new.copy()
    row = next(i for i, it in enumerate(lin) if it[0] == "raw-random")
    bad[row, 9 * lm.LIN_SUB7 + 1] += np.uint32(1 << 29)  # a carry moved without its counterpart: another integer
    with pytest.raises(AssertionError):
        hr.check_lin(lin, bad, ref)
    bad = new.copy()
    row = next(i for i, it in enumerate(lin) if it[0].startswith("raw-zero"))
    bad[row, 144] = 0
    with pytest.raises(AssertionError):
        hr.check_lin(lin, bad, ref)
