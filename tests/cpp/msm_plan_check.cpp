// CPU driver of tests/test_msm_plan.py: the MSM planner (zolt_amd/csrc/msm_plan.h) compiled by plain g++, run under the switch set of
// its environment.
//   msm_plan_check grid                 invariants of every plan over a grid of handles, launches and fused batches
//   msm_plan_check fuse HN N K WIDE     the fuse verdict for K vectors of N scalars on a default handle of HN bases: "kc sort"
//   msm_plan_check table                default plans of table and one-shot handles, 2^10 .. 2^24 bases
//   msm_plan_check plan N C L USES [M]  one handle's plan for N bases under zg_msm_config{C, L, USES}, and the launch of M scalars on it
//                                       (M = N if omitted): point slices, scalars per slice, accumulate chunks of a launch made alone
#include <stdio.h>
#include <string.h>

#include <vector>

#include "msm_plan.h"

namespace zg {
void set_error(const std::string &) {}
}  // namespace zg
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

// what one sort launch over m scalars under plan q touches of the sort buffers
static SortWords launch_words(const MsmPlan &q, size_t m) {
    SortWords w;
    const size_t nblk = sort_blocks(q, m);
    if (q.sort == MsmSort::TWO_PASS) {
        w.blockhist = nblk * q.NCB;
        w.tmp = (size_t)q.W * m + 4 * (size_t)q.NCB + 4;  // entries, each coarse bin rounded up to 4
        w.cstarts = 4 * ((size_t)q.NCB + 1);
        w.fine = (fine_max_items(q, m) + q.NCB) << q.fb;
    } else if (q.sort == MsmSort::LDS) {
        w.blockhist = nblk * q.NK;
    }
    return w;
}

static void check_sort(const MsmPlan &p, size_t table_rows, const char *what, size_t n) {
    if (p.sort == MsmSort::LDS) {
        CHECK((size_t)p.NK * 4 <= 128 * 1024, "%s n=%zu NK=%u", what, n, p.NK);
        CHECK(p.nblk >= 1 && p.nblk <= 256, "%s n=%zu nblk=%u", what, n, p.nblk);
    }
    if (p.sort == MsmSort::TWO_PASS) {
        const int fb_min = env_int("ZG_MSM_FINE_BITS_MIN", 5);
        CHECK(p.fb + p.rb == 31, "%s n=%zu fb=%d rb=%d", what, n, p.fb, p.rb);
        CHECK(table_rows <= ((size_t)1 << p.rb), "%s n=%zu rows=%zu rb=%d", what, n, table_rows, p.rb);
        CHECK(p.NCB <= 3000 && p.NCB == (p.NK + (1u << p.fb) - 1) >> p.fb, "%s n=%zu NCB=%u", what, n, p.NCB);
        CHECK(p.W <= 32, "%s n=%zu W=%d", what, n, p.W);
        CHECK(p.fb >= fb_min && p.fb <= 7, "%s n=%zu fb=%d", what, n, p.fb);
    }
    if (p.sort == MsmSort::ATOMIC) CHECK(p.fb == 0 && p.nblk == 0, "%s n=%zu", what, n);
}

// every launch a set of n_total scalars under p makes fits the workspace sized for it (msm_enqueue_lane: point slices included)
static void check_launches(const MsmPlan &p, size_t n_total, const SortWords &cap, const char *what) {
    for (size_t m : {n_total, n_total / 3 + 1, (size_t)1, (size_t)1025, (size_t)40000}) {
        if (m > n_total || !m) continue;
        const LaunchCut cut = launch_cut(p, m, cap);
        const size_t S = cut.S, per = cut.per;
        const MsmPlan &q = cut.sort;
        const size_t last = m - (S - 1) * per;
        CHECK(S >= 1 && S <= DEV_SLICES_MAX && per * (S - 1) < m && last >= 1 && last <= per, "%s m=%zu S=%zu per=%zu", what, m, S, per);
        for (size_t cnt : {per * (size_t)p.K, last * (size_t)p.K}) {
            CHECK(launch_words(q, cnt).fit_in(cap), "%s m=%zu cnt=%zu sort=%d", what, m, cnt, (int)q.sort);
            if (q.sort != MsmSort::ATOMIC) CHECK(sort_blocks(q, cnt) >= 1, "%s m=%zu cnt=%zu", what, m, cnt);
        }
    }
}

static int grid() {
    const std::vector<size_t> ns = {1, 2, 3, 63, 64, 100, 1000, 2047, 2048, 4096, 6000, 8191, 8192, 16384, 16385, 20000, 32767, 32768, 65536,
                                    100000, 131072, 131073, 262144, 300000, 524288, 900000, 1 << 20, 1594323, 1 << 21, 1 << 22, 4400000,
                                    1 << 23, 1 << 24, 1 << 25, 1 << 26, (1 << 27) - 1};
    std::vector<zg_msm_config> cfgs;
    for (int c = 0; c <= 19; c++)
        if (c != 1)
            for (int L : {0, 1, 2})
                for (int u : {0, 1, 2}) cfgs.push_back(zg_msm_config{c, L, u});
    char what[160];
    for (size_t hn : ns)
        for (const auto &cfg : cfgs) {
            MsmPlan p;
            snprintf(what, sizeof what, "handle %d/%d/%d", cfg.window_bits, cfg.precompute_levels, cfg.expected_uses);
            if (plan_msm(hn, &cfg, 1, hn, p) != ZG_OK) continue;
            CHECK(p.K == 1 && p.NK == p.NB * (uint32_t)p.G && p.NT >= 1 && p.G * p.L >= p.W, "%s n=%zu", what, hn);
            check_sort(p, (size_t)p.L * hn, what, hn);
            check_launches(p, hn, workspace_sort_words(p, hn), what);
            if (hn > ((size_t)1 << 22)) continue;
            for (size_t n : {hn, hn / 2, hn / 5 + 3, (size_t)1000, (size_t)16385})
                for (int wide = 0; wide < 2 && n && n <= hn; wide++)
                    for (size_t k = 1; k <= 32; k++) {
                        MsmPlan set;
                        const size_t kc = fuse_set_size(p, hn, n, k, wide, set);
                        snprintf(what, sizeof what, "fused %d/%d/%d hn=%zu wide=%d k=%zu", cfg.window_bits, cfg.precompute_levels, cfg.expected_uses, hn, wide, k);
                        if (!kc) continue;
                        CHECK(kc >= 2 && kc <= k && kc * n <= ((size_t)1 << 22) && (size_t)set.K == kc, "%s n=%zu kc=%zu", what, n, kc);
                        CHECK(set.sort != MsmSort::ATOMIC && set.c == p.c && set.L == p.L && set.G == p.G, "%s n=%zu kc=%zu", what, n, kc);
                        check_sort(set, (size_t)p.L * hn, what, n);
                        const SortWords cap = workspace_sort_words(set, n * kc);
                        check_launches(set, n, cap, what);
                        const zg_msm_config scfg{p.c, p.L, 0};
                        for (size_t kk = 1; kk < kc; kk++) {  // a shorter last set in the same workspace
                            MsmPlan pl;
                            CHECK(plan_msm(n, &scfg, kk, hn, pl, &set) == ZG_OK && pl.sort == set.sort && pl.nblk == set.nblk, "%s kk=%zu", what, kk);
                            CHECK(launch_words(pl, n * kk).fit_in(cap) && pl.NT <= set.NT && pl.NK <= set.NK, "%s kk=%zu", what, kk);
                        }
                    }
        }
    printf("grid %s: %ld checks, %ld failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "grid")) return grid();
    if (argc == 6 && !strcmp(argv[1], "fuse")) {
        const size_t hn = strtoull(argv[2], nullptr, 0), n = strtoull(argv[3], nullptr, 0), k = strtoull(argv[4], nullptr, 0);
        MsmPlan p, set;
        if (plan_msm(hn, nullptr, 1, hn, p) != ZG_OK) return 2;
        const size_t kc = fuse_set_size(p, hn, n, k, atoi(argv[5]) != 0, set);
        printf("%zu %d\n", kc, kc ? (int)set.sort : -1);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "table")) {
        for (int e = 10; e <= 24; e++)
            for (int uses : {0, 1}) {
                const zg_msm_config cfg{0, 0, uses};
                MsmPlan p;
                if (plan_msm((size_t)1 << e, &cfg, 1, (size_t)1 << e, p) != ZG_OK) return 2;
                printf("%d %d c=%d W=%d L=%d G=%d sort=%d fb=%d NCB=%u nblk=%u NT=%u\n", e, uses, p.c, p.W, p.L, p.G, (int)p.sort, p.fb, p.NCB, p.nblk, p.NT);
            }
        return 0;
    }
    if ((argc == 6 || argc == 7) && !strcmp(argv[1], "plan")) {
        const size_t hn = strtoull(argv[2], nullptr, 0);
        const zg_msm_config cfg{atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
        const size_t m = argc == 7 ? strtoull(argv[6], nullptr, 0) : hn;
        MsmPlan p;
        if (m > hn || plan_msm(hn, &cfg, 1, hn, p) != ZG_OK) return 2;
        size_t S, per;
        slice_counts(p, m, S, per);
        const uint32_t nt = launch_chunks(p, per, true);  // one accumulate launch over `per` scalars with no other MSM in flight
        printf("n=%zu c=%d W=%d L=%d G=%d NB=%u NK=%u NT=%u GS=%d lb=%d hb=%d sort=%d tail=%d fb=%d NCB=%u nblk=%u m=%zu S=%zu per=%zu launch_NT=%u\n", hn, p.c,
               p.W, p.L, p.G, p.NB, p.NK, p.NT, p.GS, p.lb, p.hb, (int)p.sort, (int)p.tail, p.fb, p.NCB, p.nblk, m, S, per, nt);
        return 0;
    }
    fprintf(stderr, "usage: msm_plan_check grid | fuse HN N K WIDE | table | plan N C L USES [M]\n");
    return 2;
}
