// CPU driver of tests/test_lane_tail_map.py: the index map of msm_rowcol_lane_kernel (zolt_amd/csrc/msm_lane_map.h) replayed thread by
// thread, as the kernel walks it, for the three shapes the planner can choose (6 x 6, 6 x 8, 8 x 8):
//   - every bucket index 1 .. 2^(lb+hb) - 1 is read exactly once by the row pass and exactly once by the column pass, index 0 (no
//     bucket) is met once by each and skipped, and no read leaves the bucket array;
//   - every LDS slot a stage reads was written exactly once, by the stage before it, and a slot written in a stage is read in that stage
//     by its writer alone (results are stored in place, over the unit's first input);
//   - every rc slot is written exactly once, by line L of its workgroup into slot L.
// Also the planner's rule (msm_plan.h: plan_tail) on the shapes it is meant to split. Prints "lane map ok" and exits 0, or the first
// failures and exits 1.
#include <stdio.h>

#include <string>
#include <vector>

#include "msm_plan.h"

namespace zg {
void set_error(const std::string &msg) { fprintf(stderr, "planner error: %s\n", msg.c_str()); }
}  // namespace zg

using namespace zg;
namespace lm = zg::lane_map;

static int g_fail = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            if (g_fail++ < 20) {           \
                fprintf(stderr, "FAIL %s: ", #cond); \
                fprintf(stderr, __VA_ARGS__);        \
                fprintf(stderr, "\n");     \
            }                              \
        }                                  \
    } while (0)

static void check_shape(int lb, int hb) {
    CHECK(lm::line_bits_ok(lb) && lm::line_bits_ok(hb), "%d x %d", lb, hb);
    const uint32_t NB = 1u << (lb + hb), nrow = 1u << hb, ncol = 1u << lb;
    std::vector<int> row_reads(NB, 0), col_reads(NB, 0), rc_writes(nrow + ncol, 0);
    CHECK(lm::workgroups(lb, hb) * lm::LINES == nrow + ncol, "%d x %d", lb, hb);
    for (uint32_t wg = 0; wg < lm::workgroups(lb, hb); wg++) {
        const uint32_t line0 = wg * lm::LINES;
        const int m = lm::line_bits(lb, hb, line0), S = lm::stages(m);
        for (uint32_t r = 0; r < lm::LINES; r++)  // the four lines are all rows or all columns
            CHECK(lm::line_bits(lb, hb, line0 + r) == m, "wg %u line %u", wg, r);
        CHECK(S >= 3 && lm::units(m, S) == lm::LINES && lm::units(m, 1) <= 256, "m=%d", m);
        std::vector<int> written_in(lm::SLOTS, 0), writes(lm::SLOTS, 0);  // stage of the last write, writes in that stage
        // stage 1: threads 0 .. 255, the active ones read four elements each
        CHECK(!lm::quad_stage(m, 1), "m=%d", m);
        for (uint32_t t = 0; t < 256; t++) {
            if (t >= lm::units(m, 1)) continue;
            const uint32_t line = line0 + lm::first_line(m, t), e0 = lm::first_element(m, t);
            CHECK(lm::first_line(m, t) < lm::LINES && e0 + 3 < (1u << m), "t=%u", t);
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t k = lm::element(lb, hb, line, e0 + i);
                CHECK(k < NB, "wg %u t %u element %u -> %u", wg, t, i, k);
                if (k < NB) (line < nrow ? row_reads : col_reads)[k]++;
            }
            const uint32_t o = lm::out_slot(1, t);
            CHECK(o < lm::SLOTS, "slot %u", o);
            if (o < lm::SLOTS) written_in[o] = 1, writes[o]++;
        }
        for (int s = 2; s <= S; s++) {
            const bool quad = lm::quad_stage(m, s);
            CHECK(quad == (lm::units(m, s) <= 16), "m=%d s=%d", m, s);  // 16 and 4 units: 64 and 16 lanes as quads
            const uint32_t nu = lm::units(m, s);
            CHECK(nu * (quad ? 4u : 1u) <= 256, "m=%d s=%d", m, s);
            std::vector<int> reader(lm::SLOTS, -1);
            for (uint32_t u = 0; u < nu; u++)
                for (uint32_t i = 0; i < 4; i++) {
                    const uint32_t in = lm::in_slot(s, u, i);
                    CHECK(in < lm::SLOTS, "slot %u", in);
                    if (in >= lm::SLOTS) continue;
                    CHECK(written_in[in] == s - 1 && writes[in] == 1, "m=%d s=%d u=%u reads slot %u written in stage %d x%d", m, s, u, in,
                          written_in[in], writes[in]);
                    CHECK(reader[in] == -1, "slot %u read twice in stage %d", in, s);
                    reader[in] = (int)u;
                }
            for (uint32_t u = 0; u < nu; u++) {
                if (s == S) {
                    rc_writes[line0 + u]++;
                    // the unit's inputs descend from line u's elements alone: 4^(s-1) consecutive stage-1 units each
                    CHECK(lm::first_line(m, lm::in_slot(s, u, 0)) == u && lm::first_line(m, lm::in_slot(s, u, 3) + (1u << (2 * (s - 2))) - 1) == u,
                          "m=%d unit %u", m, u);
                    continue;
                }
                const uint32_t o = lm::out_slot(s, u);
                CHECK(o < lm::SLOTS, "slot %u", o);
                if (o >= lm::SLOTS) continue;
                CHECK(reader[o] == -1 || reader[o] == (int)u, "m=%d s=%d slot %u written by %u, read by %d", m, s, o, u, reader[o]);
                if (written_in[o] != s) writes[o] = 0;
                written_in[o] = s;
                writes[o]++;
            }
        }
    }
    CHECK(row_reads[0] == 1 && col_reads[0] == 1, "%d x %d: index 0 met %d / %d times", lb, hb, row_reads[0], col_reads[0]);
    for (uint32_t k = 1; k < NB; k++)
        CHECK(row_reads[k] == 1 && col_reads[k] == 1, "%d x %d: bucket %u read %d / %d times", lb, hb, k, row_reads[k], col_reads[k]);
    for (uint32_t L = 0; L < nrow + ncol; L++) CHECK(rc_writes[L] == 1, "%d x %d: rc slot %u written %d times", lb, hb, L, rc_writes[L]);
}

// plan of a full-table handle of 2^logn bases with forced window bits c (0 = the planner's) under ZG_MSM_LANE_TAIL = sw ("" = unset)
static MsmPlan plan(int logn, int c, const char *sw) {
    if (*sw) setenv("ZG_MSM_LANE_TAIL", sw, 1); else unsetenv("ZG_MSM_LANE_TAIL");
    const zg_msm_config cfg{c, 0, 0};
    MsmPlan p;
    CHECK(plan_msm((size_t)1 << logn, &cfg, 1, (size_t)1 << logn, p) == ZG_OK, "plan 2^%d c=%d", logn, c);
    return p;
}

static void check_planner() {
    for (const char *sw : {"", "auto"}) {
        MsmPlan p = plan(20, 0, sw);  // the headline plan
        CHECK(p.c == 17 && p.tail == MsmTail::LANE && p.lb == 8 && p.hb == 8 && p.NT <= 2 * p.NK, "2^20 %s", sw);
        p = plan(17, 0, sw);  // c = 16: 8 x 7
        CHECK(p.tail == MsmTail::QUAD && p.lb == 8 && p.hb == 7, "2^17 %s", sw);
        p = plan(15, 13, sw);  // 2^16 chunks over 2^12 buckets
        CHECK(p.tail == MsmTail::QUAD && p.lb == 6 && p.hb == 6, "2^15 c=13 %s", sw);
        p = plan(15, 15, sw);  // auto never moves lb / hb
        CHECK(p.tail == MsmTail::QUAD && p.lb == 7 && p.hb == 7, "2^15 c=15 %s", sw);
    }
    MsmPlan p = plan(20, 0, "0");
    CHECK(p.tail == MsmTail::QUAD && p.lb == 8 && p.hb == 8, "2^20 off");
    p = plan(12, 13, "1");
    CHECK(p.tail == MsmTail::LANE && p.lb == 6 && p.hb == 6, "2^12 c=13 forced");
    p = plan(15, 15, "1");
    CHECK(p.tail == MsmTail::LANE && p.lb == 6 && p.hb == 8, "2^15 c=15 forced");
    p = plan(17, 0, "1");
    CHECK(p.tail == MsmTail::QUAD && p.lb == 8 && p.hb == 7, "2^17 forced");
    p = plan(12, 11, "1");  // 5 x 5 would split as 4 x 6: rows of 16 are no lane stage
    CHECK(p.tail == MsmTail::QUAD && p.lb == 5 && p.hb == 5, "c=11 forced");
    p = plan(20, 19, "1");  // 9 x 9
    CHECK(p.tail == MsmTail::QUAD && p.lb == 9 && p.hb == 9, "c=19 forced");
    // several bucket sets never take the lane form: a table-less handle (G > 1), a fused batch (K > 1)
    setenv("ZG_MSM_LANE_TAIL", "1", 1);
    const zg_msm_config one_shot{13, 1, 0}, table{13, 0, 0};
    CHECK(plan_msm(4096, &one_shot, 1, 4096, p) == ZG_OK && p.G > 1 && p.tail == MsmTail::QUAD, "table-less");
    CHECK(plan_msm(4096, &table, 2, 4096, p) == ZG_OK && p.K == 2 && p.tail == MsmTail::QUAD, "batch");
    setenv("ZG_MSM_REDUCE_2D", "0", 1);
    CHECK(plan_msm(4096, &table, 1, 4096, p) == ZG_OK && p.lb == 0 && p.tail == MsmTail::QUAD, "1-D reduction");
    unsetenv("ZG_MSM_REDUCE_2D");
    unsetenv("ZG_MSM_LANE_TAIL");
}

int main() {
    check_shape(6, 6);
    check_shape(6, 8);
    check_shape(8, 8);
    check_planner();
    if (g_fail) {
        fprintf(stderr, "%d failure(s)\n", g_fail);
        return 1;
    }
    printf("lane map ok\n");
    return 0;
}
