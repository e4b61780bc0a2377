"""The vectors of tests/xyzz_model.py must notice a group law that is subtly wrong — on the CPU. For every entry of MUTANTS this copies one
header of zolt_amd/csrc into a temporary directory, changes ONE place of its text, compiles tests/cpp/xyzz_host.cpp with that directory
first on the include path and runs the records: the checker has to raise. A mutant that no record can tell from the original is listed as
equivalent with the reason, and the test holds it to that: every record still passes. Nothing here is built for, or run on, a device.

What the list settled:
  * xyzz_dbl without its identity test is EQUIVALENT under the header's contract "identity <=> zz == 0": the formulas give
    zz' = V * zz = 0 and zzz' = W * zzz, so the result is an identity whose x, y and zzz are other garbage than the input's. Nothing that
    reads an XyzzT looks at x, y or zzz before it has tested zz (xyzz_add, xyzz_madd, xyzz_dbl, xyzz_to_affine, xyzz_to_jacobian), and
    the records feed identities with non-zero garbage on purpose, so the coordinates under zz == 0 do not matter and the checker does not
    compare them.
  * fe_inv_safegcd's first conditional add of the modulus (the normalisation after the loop) IS needed: d leaves the loop anywhere in
    (-2 MOD, MOD), so the bound is reached on its lower side: 83 of the 2^16 uniform Fp values (about one in 800) and the raw pattern
    (p - 1) / 2 of the structured list end below -MOD with f = +1, where the second add alone leaves d negative. Those records kill
    the mutant (with f = -1 the negation lands in (MOD, 2 MOD), which the final product by R^3 reduces anyway).
  * the loop bound `batch < 40` lowered to 20 is equivalent: 590 division steps bound the loop for 256-bit inputs (the comment in
    field.hip.h), 20 batches of 30 are 600. Lowered to 12 it is killed.

    python -m pytest tests/test_xyzz_mutants_host.py -q --durations=0"""
import os
import shutil

import pytest

from tests import xyzz_model as xm

pytestmark = pytest.mark.skipif(not os.path.exists(xm.HIPCC), reason="hipcc is absent: the host harness compiles the kernels' own HIP headers")

SEED = 2027  # the records of tests/test_xyzz_group_law_host.py
CSRC = os.path.join(xm.ROOT, "zolt_amd", "csrc")
X, FLD = "xyzz.hip.h", "field.hip.h"
IDENT = "XyzzT<F>::identity()"

# (id, header, old text, new text, the op whose records must notice — None: equivalent, reason)
MUTANTS = [
    ("madd-drops-acc-identity", X, "    if (a.is_identity()) return XyzzT<F>::from_affine(p);\n", "", xm.MADD, None),
    ("madd-same-point-gives-identity", X, "if (R.is_zero()) return xyzz_dbl_affine(p);", f"if (R.is_zero()) return {IDENT};", xm.MADD, None),
    ("madd-opposite-gives-p", X, f"return {IDENT};                 // opposite points", "return XyzzT<F>::from_affine(p);", xm.MADD, None),
    ("add-drops-identity-a", X, "    if (a.is_identity()) return b;\n", "", xm.ADD, None),
    ("add-drops-identity-b", X, "    if (b.is_identity()) return a;\n", "", xm.ADD, None),
    ("add-same-point-gives-identity", X, "if (R.is_zero()) return xyzz_dbl(a);", f"if (R.is_zero()) return {IDENT};", xm.ADD, None),
    ("add-opposite-gives-a", X, f"return xyzz_dbl(a);\n        return {IDENT};", "return xyzz_dbl(a);\n        return a;", xm.ADD, None),
    ("dbl-drops-identity-test", X, "    if (p.is_identity()) return p;\n", "", None,
     "zz' = V * zz = 0 either way: an identity over other garbage, and the contract is identity <=> zz == 0"),
    ("neg-keeps-y", X, "r.y = fe_neg(a.y);", "r.y = a.y;", xm.NEG, None),
    ("to-affine-x-by-iz", X, "out.x = fe_mul(p.x, izz);", "out.x = fe_mul(p.x, iz);", xm.TO_AFFINE, None),
    ("scalar-mul-skips-bit-0", X, "bit >= 0", "bit > 0", xm.SCALAR_MUL, None),
    ("scalar-mul-limb-select-off-by-one", X, "(k == limb) ? s.l[k]", "(k + 1 == limb) ? s.l[k]", xm.SCALAR_MUL, None),
    ("axpy-ignores-b-inf", X, "if (!(b_inf && b_inf[i])) acc", "acc", xm.AXPY, None),
    ("axpy-ignores-a-inf", X, "a_inf && a_inf[i], s)", "false, s)", xm.AXPY, None),
    ("dbl-affine-zzz-is-v", X, "    r.zz = V;\n    r.zzz = W;", "    r.zz = V;\n    r.zzz = V;", xm.DBL_AFFINE, None),
    ("inv-drops-first-conditional-add", FLD, "            d.v[k] += mod.v[k] & cond_add;\n            d.v[k] = (d.v[k] ^ cond_neg) - cond_neg;",
     "            d.v[k] = (d.v[k] ^ cond_neg) - cond_neg;", xm.INV, None),
    ("inv-drops-second-conditional-add", FLD, "for (int k = 0; k < 9; k++) d.v[k] += mod.v[k] & cond_add;", "for (int k = 0; k < 9; k++) d.v[k] += 0;", xm.INV, None),
    ("inv-drops-negation", FLD, "d.v[k] = (d.v[k] ^ cond_neg) - cond_neg;", "d.v[k] = d.v[k] + 0;", xm.INV, None),
    ("inv-12-batches", FLD, "batch < 40", "batch < 12", xm.INV, None),
    ("inv-20-batches", FLD, "batch < 40", "batch < 20", None, "590 division steps bound the loop for 256-bit inputs; 20 batches run 600"),
]


def _mutated_harness(tmp_path, header, old, new):
    text = open(os.path.join(CSRC, header)).read()
    assert text.count(old) == 1, f"{header}: {text.count(old)} places hold {old!r}"
    changed = text.replace(old, new)
    assert changed != text and len(changed) == len(text) - len(old) + len(new)
    # a quoted #include looks in the includer's own directory before any -I: the headers that lead from the harness to the changed one
    # have to sit beside it, so the directory holds a copy of every header and is the only one of the project's on the include path
    inc = tmp_path / "inc"
    inc.mkdir()
    for h in os.listdir(CSRC):
        if h.endswith(".h"):
            shutil.copy(os.path.join(CSRC, h), inc / h)
    (inc / header).write_text(changed)
    return xm.compile_host(str(tmp_path / "xyzz_host_mutant"), include_first=str(inc))


def _items(gid, op):
    return xm.records_for(gid, op, SEED, xm.inv_total(gid) if op == xm.INV else xm.COUNTS[op])


@pytest.mark.parametrize("name,header,old,new,op,reason", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant(tmp_path, name, header, old, new, op, reason):
    run = _mutated_harness(tmp_path, header, old, new)
    for gid in (xm.G1, xm.G2):
        grp = xm.GROUPS[gid]
        if op is not None:
            items = _items(gid, op)
            with pytest.raises(AssertionError):
                xm.check(grp, op, items, run(gid, op, items))
        else:
            assert reason
            for o in ((xm.INV,) if header == FLD else xm.ALL_OPS):
                items = _items(gid, o)
                xm.check(grp, o, items, run(gid, o, items))
