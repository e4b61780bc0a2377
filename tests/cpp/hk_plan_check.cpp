// CPU driver of tests/test_hk_plan.py: the level plan of HyperKZG.open (zolt_amd/csrc/hk_plan.h) compiled by plain g++.
//   hk_plan_check grid                          invariants of every plan over a grid of table sizes, points, SRS lengths, modes, fork
//   hk_plan_check plan N_EVALS VARS SRS MODE FORK   one plan as a line of text:
//       computed=C small=FIRST+ROWSxLEN@OFF long=FIRST+ROWSxLEN@OFF own=LEVEL@OFF:COUNT,... rowlens=N,... arena=N   ("-": none)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "hk_plan.h"

using namespace zg;

static long failures = 0, checks = 0;
#define CHECK(cond, ...)                               \
    do {                                               \
        checks++;                                      \
        if (!(cond)) {                                 \
            if (failures++ < 20) {                     \
                printf("FAIL %s: ", #cond);            \
                printf(__VA_ARGS__);                   \
                printf("\n");                          \
            }                                          \
        }                                              \
    } while (0)

// The sizing pre-pass of hk_open_device as it stood before the plan existed (restated from the parent commit of hk_plan.h): the
// matrix geometry, and the entries of its two quotient buffers d_small and d_qall.
struct Parent {
    size_t levels = 0, small_rows = 0, small_len = 0, long_rows = 0, long_len = 0, long_len2 = 0;
    bool fuse_long = false, split_first = false;
    size_t fl_len = 0, fl_rows = 0, fl_off = 0, entries = 0;
};
static Parent parent_sizing(size_t n_evals, size_t num_vars, size_t srs_len, unsigned mode, bool fork) {
    Parent q;
    size_t len = n_evals;
    for (size_t i = 0; i < num_vars; i++) {
        size_t half = len / 2;
        if (half == 0) break;
        size_t nc = half < srs_len ? half : srs_len;
        if (nc <= 16384) {
            if (q.small_rows == 0) q.small_len = nc;
            q.small_rows++;
        } else {
            if (q.long_rows == 0) q.long_len = nc;
            if (q.long_rows == 1) q.long_len2 = nc;
            q.long_rows++;
        }
        q.levels++;
        len = half;
    }
    if (q.small_rows < 2) q.small_rows = 0;
    q.fuse_long = fork && mode && q.long_rows >= 2;
    q.split_first = q.fuse_long && mode == 2 && q.long_rows >= 3;
    q.fl_len = q.split_first ? q.long_len2 : q.long_len;
    q.fl_rows = q.split_first ? q.long_rows - 1 : q.long_rows;
    q.fl_off = q.split_first ? q.long_len : 0;
    q.entries = (q.small_rows * q.small_len + 1) + ((q.fuse_long ? q.fl_off + q.fl_rows * q.fl_len : 0) + n_evals + 1);
    return q;
}

static void check_plan(size_t n, size_t v, size_t srs, unsigned mode, bool fork) {
#define AT "n=%zu v=%zu srs=%zu mode=%u fork=%d", n, v, srs, mode, (int)fork
    const HkPlan p = hk_plan(n, v, srs, mode, fork);
    const Parent q = parent_sizing(n, v, srs, mode, fork);
    CHECK(p.computed == q.levels && p.computed <= (size_t)HK_MAX_LEVELS && p.computed <= v, AT);
    // the same classification as the parent
    CHECK(p.small.rows == q.small_rows && (!q.small_rows || p.small.len == q.small_len), AT);
    CHECK(p.lng.rows == (q.fuse_long ? q.fl_rows : 0) && (!q.fuse_long || p.lng.len == q.fl_len), AT);
    CHECK(p.lng.first == (q.split_first ? 1u : 0u), AT);
    // a matrix only where there is something to fuse
    CHECK(p.small.rows != 1 && p.lng.rows != 1, AT);
    CHECK(fork || p.lng.rows == 0, AT);
    CHECK(mode || p.lng.rows == 0, AT);
    size_t n_long = 0;
    for (size_t i = 0; i < p.computed; i++) n_long += p.level[i].nc > HK_SMALL;
    CHECK(p.lng.rows == 0 || p.lng.first + p.lng.rows == n_long, AT);
    CHECK(p.lng.first == 0 || (mode == 2 && n_long >= 3), AT);
    CHECK(!(fork && mode == 2 && n_long >= 3) || p.lng.first == 1, AT);
    size_t len = n, rows[2] = {0, 0};
    for (size_t i = 0; i < p.computed; i++) {
        const HkLevel &l = p.level[i];
        CHECK(l.half == len / 2 && l.half > 0 && l.nc == (l.half < srs ? l.half : srs), AT);
        len = l.half;
        // the destination the parent's main loop chose for this level
        const HkDest want = q.small_rows && l.nc <= 16384                          ? HkDest::SHORT_ROW
                            : q.fuse_long && l.nc > 16384 && !(q.split_first && i == 0) ? HkDest::LONG_ROW
                                                                                   : HkDest::OWN;
        CHECK(l.dest == want, AT);
        size_t region = l.count;
        if (l.dest != HkDest::OWN) {  // rows are consecutive levels, tile the matrix, and hold nc live entries before the padding
            const HkMatrix &m = l.dest == HkDest::SHORT_ROW ? p.small : p.lng;
            const size_t r = rows[l.dest == HkDest::LONG_ROW]++;
            CHECK(i == m.first + r && r < m.rows, AT);
            CHECK(l.off == m.off + r * m.len && l.count == l.nc && l.nc <= m.len, AT);
            CHECK(r > 0 || l.nc == m.len, AT);
            if (l.dest == HkDest::LONG_ROW) {
                CHECK(p.long_row_len[r] == l.nc && (r == 0 || p.long_row_len[r] <= p.long_row_len[r - 1]), AT);
                CHECK(l.nc > HK_SMALL, AT);
            }
            region = m.len;
        } else {
            CHECK(l.count == l.half, AT);
        }
        CHECK(l.count <= region && l.off + region <= p.arena && l.off + region >= l.off, AT);
        for (size_t j = 0; j < i; j++) {
            const HkLevel &o = p.level[j];
            const size_t o_region = o.dest == HkDest::OWN ? o.count : (o.dest == HkDest::SHORT_ROW ? p.small : p.lng).len;
            CHECK(l.off + region <= o.off || o.off + o_region <= l.off, AT);
        }
    }
    CHECK(rows[0] == p.small.rows && rows[1] == p.lng.rows, AT);
    // what is zeroed before the folds is the matrices, exactly: the padding is what makes a padded row's commit equal the unpadded one
    CHECK(p.small.entries() == p.small.rows * p.small.len && p.lng.entries() == p.lng.rows * p.lng.len, AT);
    CHECK(p.small.off + p.small.entries() <= p.arena && p.lng.off + p.lng.entries() <= p.arena, AT);
    CHECK(p.small.off + p.small.entries() <= p.lng.off || p.lng.off + p.lng.entries() <= p.small.off || !p.small.rows || !p.lng.rows, AT);
    CHECK(p.arena <= q.entries, "arena=%zu parent=%zu", p.arena, q.entries);
#undef AT
}

static void print_matrix(const char *name, const HkMatrix &m) {
    if (m.rows) printf(" %s=%zu+%zux%zu@%zu", name, m.first, m.rows, m.len, m.off);
    else printf(" %s=-", name);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "grid")) {
        size_t ns[64], n_ns = 0;
        for (size_t x : {0, 1, 2, 3, 40000, 70000, (1 << 20) + 1, (1 << 24) - 1, 12345678}) ns[n_ns++] = x;
        for (int k = 2; k <= 24; k++) ns[n_ns++] = (size_t)1 << k;
        const size_t srss[] = {1, 1000, 16384, 16385, 1 << 15, 1 << 17, 1 << 20, (1 << 24) + 256};
        for (size_t i = 0; i < n_ns; i++)
            for (size_t v = 0; v <= 34; v++)
                for (size_t srs : srss)
                    for (unsigned mode = 0; mode <= 2; mode++)
                        for (int fork = 0; fork <= 1; fork++) check_plan(ns[i], v, srs, mode, fork != 0);
        if (failures) {
            printf("%ld of %ld checks failed\n", failures, checks);
            return 1;
        }
        printf("grid ok: %ld checks\n", checks);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const HkPlan p = hk_plan(strtoull(argv[2], nullptr, 0), strtoull(argv[3], nullptr, 0), strtoull(argv[4], nullptr, 0), (unsigned)atoi(argv[5]),
                                 atoi(argv[6]) != 0);
        printf("computed=%zu", p.computed);
        print_matrix("small", p.small);
        print_matrix("long", p.lng);
        const char *sep = " own=";
        for (size_t i = 0; i < p.computed; i++)
            if (p.level[i].dest == HkDest::OWN) {
                printf("%s%zu@%zu:%zu", sep, i, p.level[i].off, p.level[i].count);
                sep = ",";
            }
        if (sep[0] == ' ') printf(" own=-");
        sep = " rowlens=";
        for (size_t r = 0; r < p.lng.rows; r++) {
            printf("%s%zu", sep, p.long_row_len[r]);
            sep = ",";
        }
        if (sep[0] == ' ') printf(" rowlens=-");
        printf(" arena=%zu\n", p.arena);
        return 0;
    }
    fprintf(stderr, "usage: hk_plan_check grid | plan N_EVALS VARS SRS MODE FORK\n");
    return 2;
}
