"""Static guard on the three carry passes the mixed addition no longer runs (no GPU needed: hipcc cross-compiles for gfx950).

xyzz29_madd_nz (zolt_amd/csrc/g1_29.hip.h) hands P = U2 + 7p - X1, R = +-S2 + 4p|5p - Y1 and 4p - Y1 to the multiplier un-carried
(fp29.hip.h: f29_sub7_raw, f29_pmsub45_raw, f29_neg4_raw). Each f29_carry was one and + shift + add per limb, about 25 vector
instructions. The steady path of msm_accumulate_chunk_kernel<false> — found from the control-flow graph as in
tests/test_msm_accumulate_loop_isa.py, whose fixture this file uses — had 2156 vector instructions with the three passes; the expected
cut is about 75, and the ceiling below leaves 15 of them for the compiler fusing a carry's and / shift differently than counted.
Read from the build this test was written against: 2086 (docs/design/04_kernels.md, section 4a'').
"""
from tests.test_msm_accumulate_loop_isa import loop  # noqa: F401  (the module-scoped fixture: one compile of msm.hip, the loop's CFG)

PARENT_PATH_VALU = 2156
PATH_VALU_MAX = PARENT_PATH_VALU - 60


def test_steady_path_lost_the_three_carry_passes(loop):  # noqa: F811
    blocks, path = loop["blocks"], loop["path"]
    total = sum(blocks[i].valu() for i in path)
    mads = sum(blocks[i].ops()["v_mad_u64_u32"] for i in path)
    print("steady path:", total, "vector instructions,", mads, "of them v_mad_u64_u32; parent", PARENT_PATH_VALU)
    assert mads == 1467, mads  # the ten products are what they were
    assert total <= PATH_VALU_MAX, total
