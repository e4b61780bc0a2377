// msm_plan.h — the MSM planner: what one launch set computes and how it sorts (host only, no HIP header).
//
// A launch set is K scalar vectors of n scalars over one handle's bases (msm.hip: msm_enqueue_lane). Its plan fixes the windows
// and table levels, the buckets, the accumulate chunk grid, the reduction shape, and which counting sort orders its digits:
//   ATOMIC    global-atomic histogram and scatter (msm_digits_kernel / msm_scatter_kernel): any bucket count
//   LDS       single pass, all K * G * NB bucket counters of a block in LDS (msm_digits_lds_kernel / msm_scatter_lds_kernel)
//   TWO_PASS  coarse bins, then the fine key bits of each bin (msm_partition_kernel / msm_fine_*): many buckets
// and which form the bucket tail (partial sums per bucket, then row / column sums) takes:
//   QUAD      a quad of lanes per addition, binary trees (msm_bucket_combine_kernel / msm_rowcol_kernel): the shortest dependency chain
//   LANE      one lane per addition, radix-4 stages (msm_bucket_combine_lane_kernel / msm_rowcol_lane_kernel): the fewest instructions
// plan_msm below decides all of it; the launches switch on MsmPlan::sort and MsmPlan::tail, and the workspace is sized by sort_words.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/zolt_gpu.h"
#include "msm_lane_map.h"

namespace zg {

void set_error(const std::string &msg);

static constexpr int MAX_GROUPS = 64;
static constexpr uint64_t MAX_BUCKETS = (uint64_t)1 << 21;  // K * G * NB of one launch set
static constexpr size_t LDS_SORT_BYTES = 128 * 1024;        // the single-pass sort's per-block bucket counters, 4 bytes each
// two-pass sort: a coarse-bin entry holds sign | fine key << rb | row reference in 32 bits (fb + rb = 31)
static constexpr int ENTRY_BITS = 31;
static constexpr int FINE_BITS_MAX = 7;           // 2^7 fine keys: msm_fine_place_kernel's LDS counters
static constexpr int FINE_BITS_MIN = 5;           // fewer fine bits mean more coarse bins than the two passes pay for
static constexpr uint32_t COARSE_BINS_MAX = 3000;  // pass 1 keeps 2 * NCB counters + 1024 scan partials next to 128 KiB of staged entries in 156 KiB of LDS
static constexpr uint32_t TWO_PASS_MIN_BUCKETS = 8192;
static constexpr uint32_t FINE_SLICE = 32768;     // entries of one pass-2 work item (see msm_coarse_base_kernel)
static constexpr size_t DEV_SLICES_MAX = 128;     // point slices of one launch set: 2^27 bases (the most a handle takes) / 2^20
// a fused set is priced by LDS counters or coarse bins (fuse_set_size): it can never exceed the bucket limit, so probing one cannot fail
static_assert((uint64_t)COARSE_BINS_MAX << FINE_BITS_MAX <= MAX_BUCKETS && LDS_SORT_BYTES / 4 <= MAX_BUCKETS, "fused sets stay plannable");

enum class MsmSort { ATOMIC, LDS, TWO_PASS };
enum class MsmTail { QUAD, LANE };

struct MsmPlan {
    int c;         // window bits
    int W;         // windows = ceil(255 / c)
    int L;         // precompute levels stored in the table
    int G;         // bucket groups = ceil(W / L); window w -> group w % G, level w / G
    uint32_t NB;   // buckets per group = 2^(c-1)
    uint32_t NK;   // total buckets = K * G * NB
    int K;         // MSMs sharing one launch set (scalar vectors over the same bases); bucket group = batch * G + w % G
    int PB;        // bit-sum partial blocks per (group, bit)
    int lb, hb;    // two-dimensional bucket reduction: low / high bits of a digit magnitude (0 = one-dimensional bit sums)
    uint32_t NT;   // chunk-scheduled accumulate: the most threads (chunks) a launch uses
    int GS;        // lanes per bucket in the combine pass
    MsmSort sort;  // the counting sort of the digits
    MsmTail tail;  // the form of the bucket tail (plan_tail)
    int fb;        // TWO_PASS: low key bits resolved by the second pass (0 otherwise)
    int rb;        // TWO_PASS: bits of a row reference inside an intermediate entry (= 31 - fb)
    uint32_t NCB;  // TWO_PASS: coarse bins = ceil(NK / 2^fb)
    uint32_t nblk; // LDS: sort blocks of the full set (shorter launches use fewer: sort_blocks); TWO_PASS: partition blocks of the full set
};

static inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

static inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// ZG_MSM_CHUNK_THREADS: a fixed accumulate chunk count (0 = auto, the default; read per call)
static inline uint32_t forced_chunk_threads() {
    int v = env_int("ZG_MSM_CHUNK_THREADS", 0);
    return v < 1 ? 0u : (uint32_t)v;
}

// scalars per block of the single-pass LDS sort: with few buckets the per-block histogram is cheap, and a short input spread over
// more blocks is less of a dependent load -> LDS atomic -> store chain per thread (1024 points: scatter 30 -> 10 us)
static inline uint32_t sort_span(uint32_t NK) {
    int v = env_int("ZG_MSM_SORT_SPAN", 0);
    if (v > 0) return (uint32_t)v;
    return NK <= 4096 ? 256u : 2048u;
}

// scalars per block of the two-pass sort's first pass: a partition block stages per_block * W entries in LDS and keeps them in 32
// registers per thread as ceil(per_block / 1024) rows per window (msm_partition_kernel): <= 2048 scalars for W <= 16 windows, <= 1024
// up to 32 windows
static inline uint32_t two_pass_span(int W) {
    uint32_t cap = W <= 16 ? 2048u : 1024u;
    uint32_t v = (uint32_t)env_int("ZG_MSM_TWO_PASS_SPAN", 2048);
    v = v < 256 ? 256 : v;
    return v > cap ? cap : v;
}

// chunks (threads, or quads of lanes) of the chunk-scheduled accumulate for a launch set of `digits` entries
// alone: no other MSM of the handle is in flight — nothing needs the spare registers, the kernel takes every slot (2^20 points:
// 1.26 -> 1.18 ms)
static inline uint32_t chunk_threads(uint64_t digits, bool alone = false) {
    static const uint64_t per_chunk = [] {
        int v = env_int("ZG_MSM_CHUNK_ENTRIES", 16);  // sorted entries per chunk a launch aims for (each chunk also emits >= 1 partial)
        return (uint64_t)(v < 1 ? 1 : v);
    }();
    uint64_t want = digits / per_chunk;
    uint32_t nt = 1024;
    while (nt < want && nt < 131072u) nt <<= 1;
    // full size = 2 waves per SIMD on 256 CUs (512 workgroups). With other MSMs in flight a launch takes 7/8 of it (448 workgroups: a
    // quarter of the CUs hold one workgroup instead of two): the spare registers let another stream's latency-bound kernels (bit sums,
    // final) run under this kernel, and the NEXT accumulation's first workgroups start at once on the half-filled CUs, so that the
    // equal-length chunks of consecutive launches stop draining and refilling the chip in step. Round 2 measured 15/16 against the
    // full grid (+4-6 % MSM/s); round 4 swept the count (tools/exp/archive/run_nt_sweep.sh, profiles/r4h_accumulate_slots_sweep.txt, three
    // streams at 2^20): 512 / 496 / 480 / 464 / 448 / 440 / 432 / 416 / 384 workgroups = 793 / 790 / 800 / 790 / 816 / 810 / 800 /
    // 809 / 792 MSM/s — 448 held +2 % over 480 in three separate runs.
    static const uint32_t inflight = [] {
        int v = env_int("ZG_MSM_INFLIGHT_CHUNKS", 114688);
        return (uint32_t)(v < 1024 ? 1024 : (v > 131072 ? 131072 : v));
    }();
    return nt == 131072u && !alone ? inflight : nt;
}

// The shape of a launch set of `batch` vectors of n scalars: windows, levels, buckets, chunk grid, reduction. The sort is plan_sort's.
static int plan_shape(size_t n, const zg_msm_config *cfg, size_t batch, MsmPlan &p) {
    int c = cfg ? cfg->window_bits : 0;
    if (c == 0) c = env_int("ZG_MSM_WINDOW_BITS", 0);
    int L = cfg ? cfg->precompute_levels : 0;
    if (L == 0) L = env_int("ZG_MSM_PRECOMPUTE", 0);
    // a handle that will serve only a few MSMs (MSM.compute on a temporary slice) skips the table: its build costs about as
    // much as twenty MSMs save (2^20 points: 41 ms against 2 ms per MSM)
    if (L == 0 && cfg && cfg->expected_uses > 0 && cfg->expected_uses < 16) L = 1;
    if (c == 0 && L == 1) {
        // table-less plan (one bucket set per window): the windows cost buckets, not table rows, so the choice differs from the table
        // plan's. Measured (tools/exp/archive/run_noprecomp_sweep.sh, profiles/r4_noprecomp_sweep.txt): at 2^20 points c = 15 runs 559 MSM/s
        // pipelined / 3.0 ms alone, c = 13 553 / 3.3, and the table plan's c = 16 347 / 4.4 (2^19 buckets overflow the LDS sort:
        // digits 0.03 -> 0.64 ms, sort 0.26 -> 0.93); at 2^16 points c = 13 is 0.55 / 1.42 ms against 0.90 / 1.63 for c = 16.
        // What remains alone is the window combine: (W - 1) c = 240 dependent doublings (msm_groups_kernel, 0.86 ms) that a table
        // would have removed and nothing else can.
        c = n >= ((size_t)1 << 19) ? 15 : (n >= 8192 ? 13 : (n >= 2048 ? 8 : (n >= 64 ? 7 : 5)));
    }
    if (c == 0) {
        // measured on MI355X (tools/bench_window.py): window sizes whose last window covers only a couple of the 254
        // scalar bits (c = 9, 12, 14) waste a window and pile its digits into a handful of buckets; 16 wins from
        // 2^15 points up (fewest windows; the rest of the pipeline is latency), 8 / 7 below.
        c = n >= 32768 ? 16 : (n >= 8192 ? 10 : (n >= 2048 ? 8 : (n >= 64 ? 7 : 5)));  // 2^13 points: 0.40 ms with c = 8, 0.32 with 10
        // 17 bits = 15 windows instead of 16 (6 % fewer bucket additions) for twice the buckets: pays from about 2^20 points,
        // as long as the 15 n table rows leave the two-pass sort at least 5 fine key bits beside the 26-bit reference of an
        // intermediate entry (n <= 4.4 M: 2^22 points run 177 instead of 172 MSM/s, accumulate 5.98 -> 5.61 ms)
        if (batch == 1 && n >= (size_t)env_int("ZG_MSM_C17_MIN", 900000) && (uint64_t)n * 15 <= ((uint64_t)1 << (ENTRY_BITS - FINE_BITS_MIN))) c = 17;
        // 18 / 19 bits exist (window_bits, ZG_MSM_WINDOW_BITS) and are NOT chosen: 19 bits = 14 windows take 8 % off the accumulate kernel
        // (1.18 -> 1.09 ms at 2^20) and put more than that back into the per-bucket work of 2^18 buckets (sort 0.13 -> 0.22 ms, combine +
        // row / column sums 0.27 -> 0.49 ms): 781 -> 735 MSM/s pipelined, 1.65 -> 1.95 ms alone (round 4, tools/exp/archive/run_c19.sh)
    }
    if (c < 2 || c > 19) {
        set_error("msm: window_bits must be in [2,19]");
        return ZG_ERR_INVALID;
    }
    p.c = c;
    p.W = (255 + c - 1) / c;
    if (L == 0) L = p.W;  // 288 GB of HBM: full precompute is 64*W bytes per base
    if (L < 1) L = 1;
    if (L > p.W) L = p.W;
    p.G = (p.W + L - 1) / L;
    p.L = (p.W + p.G - 1) / p.G;
    if (p.G > MAX_GROUPS) {
        set_error("msm: too many bucket groups for this window size");
        return ZG_ERR_INVALID;
    }
    p.NB = 1u << (c - 1);
    p.K = (int)batch;
    if ((uint64_t)p.NB * p.G * batch > MAX_BUCKETS) {
        set_error("msm: too many buckets");
        return ZG_ERR_INVALID;
    }
    p.NK = p.NB * (uint32_t)p.G * (uint32_t)batch;
    // chunk-scheduled accumulate: enough threads to fill 2 waves per SIMD on 256 CUs, fewer for small inputs
    const uint32_t forced = forced_chunk_threads();
    p.NT = forced ? forced : chunk_threads((uint64_t)n * batch * p.W, true);  // the most a launch uses
    // combine lanes per bucket: a bucket expects about NT/NK + 1 partials; about 4 per quad (every tree level costs the whole
    // wave one more addition; ZG_MSM_COMBINE_PER_QUAD = 8 halves the quads, measured equal)
    p.GS = 1;
    const uint64_t nt_usual = forced ? p.NT : chunk_threads((uint64_t)n * batch * p.W);  // with other MSMs in flight
    while (p.GS < 16 && (uint64_t)p.GS * (uint64_t)env_int("ZG_MSM_COMBINE_PER_QUAD", 4) < nt_usual / p.NK + 1) p.GS <<= 1;  // GS quads of lanes per bucket: 4 * GS <= 64
    // bit-sum partial blocks: ~4 buckets per thread, at most 16 (the final kernel reduces 16 lanes per bit)
    int pb = (int)(p.NB / 2 / (256 * 4));
    p.PB = pb < 1 ? 1 : (pb > 16 ? 16 : pb);
    if (c > 16 && p.PB > 8) p.PB = 8;  // msm_final_kernel holds 256 partial sums: 17 bit rows need a stride of at most 8
    // wide windows: row / column sums first (msm_rowcol_kernel); rows and columns of at most 256 buckets
    p.lb = p.hb = 0;
    if (c >= 11 && env_int("ZG_MSM_REDUCE_2D", 1)) {
        p.lb = c / 2;  // c - 1 = lb + hb, lb >= hb
        p.hb = c - 1 - p.lb;
    }
    return ZG_OK;
}

// Fine key bits left beside a reference to one of table_rows rows in a two-pass entry, at most fb_max.
static inline int fine_bits(size_t table_rows, int fb_max) {
    int need = 1;
    while (((size_t)1 << need) < table_rows) need++;
    return ENTRY_BITS - need < fb_max ? ENTRY_BITS - need : fb_max;
}

// The sort of a launch set of n_total scalars under shape p over table_rows rows. Two passes are worth it when the per-(block, bucket)
// runs of the single-pass scatter are a few bytes, i.e. many buckets; the row reference shares a 32-bit intermediate entry with the
// sign and the fine key bits. Otherwise the single pass in LDS if the counters fit, else the global-atomic sort. fused: a set of
// several vectors (zg_msm_g1_batch and its kin) sorts in LDS whenever the counters fit, whatever ZG_MSM_LDS_SORT says — a fused set is
// only formed when it sorts in LDS or in two passes (fuse_set_size).
static void plan_sort(MsmPlan &p, size_t table_rows, size_t n_total, bool fused) {
    p.fb = p.rb = 0;
    p.NCB = 0;
    if (env_int("ZG_MSM_TWO_PASS_SORT", 1) && p.NK >= TWO_PASS_MIN_BUCKETS && p.W <= 32 && (uint64_t)n_total * p.W >= (1u << 17)) {  // W: see two_pass_span
        int fb_max = env_int("ZG_MSM_FINE_BITS", FINE_BITS_MAX);
        const int fb = fine_bits(table_rows, fb_max > FINE_BITS_MAX ? FINE_BITS_MAX : fb_max);
        // fewer than 7 fine bits mean >= 512 coarse bins; down to 5 bits (2^22 points, 1024 bins) the two passes still beat the
        // single-pass sort there (0.67 vs 1.3 ms alone, +2-3 % pipelined); below that the single pass is used
        const uint32_t ncb = fb >= env_int("ZG_MSM_FINE_BITS_MIN", FINE_BITS_MIN) ? (p.NK + (1u << fb) - 1) >> fb : 0;
        if (ncb && ncb <= COARSE_BINS_MAX) {
            p.sort = MsmSort::TWO_PASS;
            p.fb = fb;
            p.rb = ENTRY_BITS - fb;
            p.NCB = ncb;
            const uint32_t nblk = (uint32_t)ceil_div(n_total, two_pass_span(p.W));
            p.nblk = nblk < 1 ? 1 : nblk;
            return;
        }
    }
    if ((size_t)p.NK * 4 <= LDS_SORT_BYTES && (fused || env_int("ZG_MSM_LDS_SORT", 1))) {
        p.sort = MsmSort::LDS;
        const uint32_t nblk = (uint32_t)(n_total / (size_t)sort_span(p.NK));
        p.nblk = nblk < 1 ? 1 : (nblk > 256 ? 256 : nblk);
        return;
    }
    p.sort = MsmSort::ATOMIC;
    p.nblk = 0;
}

static inline void plan_tail(MsmPlan &p, size_t n);

// The plan of one launch set: k scalar vectors of n scalars over a handle of table_n bases planned with cfg (a fused set: cfg =
// the handle's c and L). within: the plan of the workspace the set runs in — a shorter last set of a batch keeps that set's sort,
// fine bits and block count.
static int plan_msm(size_t n, const zg_msm_config *cfg, size_t k, size_t table_n, MsmPlan &p, const MsmPlan *within = nullptr) {
    const int rc = plan_shape(n ? n : 1, cfg, k, p);
    if (rc != ZG_OK) return rc;
    plan_tail(p, n);
    if (!within) {
        plan_sort(p, (size_t)p.L * table_n, n * k, k > 1);
        return ZG_OK;
    }
    p.sort = within->sort;
    p.fb = within->fb;
    p.rb = within->rb;
    p.NCB = p.fb ? (p.NK + (1u << p.fb) - 1) >> p.fb : 0;
    p.nblk = within->nblk;
    return ZG_OK;
}

// ---- point slices: how a launch set of n_pts points under plan p is cut, and the sort plan of one slice (launch_cut below puts the two
// together for msm.hip's msm_enqueue_lane)
static inline size_t table_span_points(int L) {
    const size_t span_mb = (size_t)env_int("ZG_MSM_TABLE_SPAN_MB", 1024);  // 0 = never slice
    if (!span_mb) return 0;
    const size_t pts = (span_mb << 20) / (64 * (size_t)L), least = (size_t)env_int("ZG_MSM_TABLE_SPAN_MIN_POINTS", 65536);  // tests lower it
    return pts < least ? least : pts;
}
static inline void slice_counts(const MsmPlan &p, size_t n_pts, size_t &S, size_t &per) {
    S = 1;
    per = n_pts;
    if (p.K != 1) return;
    const size_t sp = table_span_points(p.L);
    if (!sp || n_pts < 2 * sp) return;  // slices only pay when there are at least two full ones
    S = (n_pts + sp - 1) / sp;
    if (S > DEV_SLICES_MAX) S = DEV_SLICES_MAX;
    per = (n_pts + S - 1) / S;
    S = (n_pts + per - 1) / per;  // no empty slice
}
// ZG_MSM_LANE_TAIL: auto (the default) / 0 never / 1 wherever the lane kernels can run (read per plan)
static inline int lane_tail_switch() {
    const char *v = getenv("ZG_MSM_LANE_TAIL");
    if (!v || !*v || !strcmp(v, "auto")) return -1;
    return atoi(v) != 0;
}
// The tail form of a launch set of n points under shape p. LANE takes about half the instructions of QUAD for a chain of six lane
// and six quad additions in the row / column sums against one and seven, and one lane addition per extra partial of a bucket
// against one quad addition: it pays where instruction issue is the limit and the chain of partials is short, i.e. never on a
// latency-bound plan. One static rule, no in-flight state:
//   - one bucket set: a single scalar vector over a full table (K = G = 1) whose points are not sliced (nothing left to fold);
//   - the two-dimensional reduction is on, and its rows and columns tile the radix-4 stages exactly (lane_map::line_bits_ok);
//   - at most two accumulate chunks per bucket (NT <= 2 NK: three to four partials in a bucket) — the 2^20-point plan, in flight
//     and alone. Shorter MSMs have fewer buckets per chunk (2^17 points: five to six partials in lockstep) and keep QUAD.
// ZG_MSM_LANE_TAIL=1 drops the last condition, and splits an odd square (c = 15: 7 x 7) as lb - 1, hb + 1 (6 x 8) so that small
// shapes and unequal rows and columns can be tested; auto never moves lb / hb.
static inline void plan_tail(MsmPlan &p, size_t n) {
    p.tail = MsmTail::QUAD;
    const int sw = lane_tail_switch();
    if (sw == 0 || p.K != 1 || p.G != 1 || !p.lb) return;
    size_t S, per;
    slice_counts(p, n, S, per);
    if (S > 1) return;
    int lb = p.lb, hb = p.hb;
    if (sw == 1 && lb == hb && (lb & 1)) lb--, hb++;
    if (!lane_map::line_bits_ok(lb) || !lane_map::line_bits_ok(hb)) return;
    if (sw < 0 && p.NT > 2 * (uint64_t)p.NK) return;
    p.tail = MsmTail::LANE;
    p.lb = lb;
    p.hb = hb;
}

// A slice's sorted references need not be table rows (L * n of them): level << shift | point-of-the-slice takes fewer bits, which
// leaves more fine-key bits in a 32-bit intermediate entry and therefore fewer coarse bins — at 2^22 points the slices then sort under
// the 2^20 plan (7 fine bits, 512 bins: 130 us) instead of the handle's (5 bits, 2048 bins: 181 us). The second pass writes table rows
// into the final list (msm_fine_place_kernel). Returns false when the slice plan is no finer than the handle's (ps = p then).
static bool slice_sort_plan(const MsmPlan &p, size_t per, MsmPlan &ps, int &shift) {
    shift = 0;
    ps = p;
    if (!env_int("ZG_MSM_SLICE_LOCAL_REFS", 1)) return false;
    int k = 1;
    while (((size_t)1 << k) < per) k++;
    plan_sort(ps, (size_t)p.L << k, per, false);
    if (ps.sort != MsmSort::TWO_PASS || ps.fb <= p.fb) {
        ps = p;
        return false;
    }
    shift = k;
    return true;
}

// ---- workspace. Blocks of a sort launch over n scalars under plan q (n <= the scalars q was planned for).
static inline uint32_t sort_blocks(const MsmPlan &q, size_t n) {
    if (q.sort == MsmSort::TWO_PASS) return (uint32_t)ceil_div(n, two_pass_span(q.W));  // per_block * W <= STAGE_ENTRIES
    uint32_t nblk = q.nblk;
    while (nblk > 1 && (size_t)(nblk - 1) * 1024 >= n) nblk--;  // LDS: no empty blocks for short sub-range MSMs
    return nblk;
}
static inline size_t fine_max_items(const MsmPlan &p, size_t n_total) { return (size_t)p.NCB + (size_t)p.W * n_total / FINE_SLICE + 1; }
// Words of the sort buffers a launch set of n_total scalars under plan p needs (0 = not used by its sort).
struct SortWords {
    size_t blockhist = 0;  // LDS: nblk * NK per-block histograms / offsets; TWO_PASS: nblk * NCB
    size_t tmp = 0;        // TWO_PASS: entries partitioned by coarse bin
    size_t cstarts = 0;    // TWO_PASS: cstarts | totals | tstarts | istarts, NCB + 1 each
    size_t fine = 0;       // TWO_PASS: slicecnt[max items][2^fb] then fbase[NCB][2^fb]
    bool fit_in(const SortWords &w) const { return blockhist <= w.blockhist && tmp <= w.tmp && cstarts <= w.cstarts && fine <= w.fine; }
};
static inline SortWords sort_words(const MsmPlan &p, size_t n_total) {
    SortWords w;
    if (p.sort == MsmSort::TWO_PASS) {
        w.blockhist = (size_t)p.nblk * p.NCB;
        w.tmp = (size_t)p.W * n_total + 4 * (size_t)p.NCB + 4;
        w.cstarts = 4 * (size_t)p.NCB + 8;
        w.fine = (fine_max_items(p, n_total) + (size_t)p.NCB) * ((size_t)1 << p.fb);
    } else if (p.sort == MsmSort::LDS) {
        w.blockhist = (size_t)p.nblk * p.NK;
    }
    return w;
}
// The sort buffers of a workspace for n_total scalars under p: the set's own sort and the sort of a point slice (a handle whose own
// launch sets sort in one pass — 2^23 points and up, where a table row index leaves fewer than 5 fine bits — still sorts its slices
// in two), every buffer the larger of the two needs.
static inline SortWords workspace_sort_words(const MsmPlan &p, size_t n_total) {
    SortWords w = sort_words(p, n_total);
    size_t S, per;
    MsmPlan ps;
    int shift;
    slice_counts(p, n_total, S, per);
    if (S > 1 && slice_sort_plan(p, per, ps, shift)) {
        const SortWords ws = sort_words(ps, per);
        w = SortWords{std::max(w.blockhist, ws.blockhist), std::max(w.tmp, ws.tmp), std::max(w.cstarts, ws.cstarts), std::max(w.fine, ws.fine)};
    }
    return w;
}
// How one launch of n_pts points under the handle's plan p is cut and sorted in a workspace whose sort buffers hold `cap`: S slices of
// `per` points (the last may be shorter), each sorted under `sort` — the finer slice plan with slice-local references
// (local_shift > 0), or p itself with table-row references (local_shift = 0) when there is no finer plan or the workspace was sized
// under another slice setting and does not hold it.
struct LaunchCut {
    size_t S, per;
    MsmPlan sort;
    int local_shift;
};
static inline LaunchCut launch_cut(const MsmPlan &p, size_t n_pts, const SortWords &cap) {
    LaunchCut cut;
    slice_counts(p, n_pts, cut.S, cut.per);
    cut.sort = p;
    cut.local_shift = 0;
    if (cut.S > 1 && slice_sort_plan(p, cut.per, cut.sort, cut.local_shift) && !sort_words(cut.sort, cut.per).fit_in(cap)) {
        cut.sort = p;
        cut.local_shift = 0;
    }
    return cut;
}
// Chunks of one accumulate launch over n scalars under p: as many as ITS digits warrant (a short prefix, the last set of a batch, a
// point slice), never more than the workspace was sized for. alone: see chunk_threads.
static inline uint32_t launch_chunks(const MsmPlan &p, size_t n, bool alone) {
    const uint32_t NT = chunk_threads((uint64_t)n * p.W, alone);
    return NT > p.NT || forced_chunk_threads() ? p.NT : NT;
}
// Per-group words of the bit sums: one-dimensional c * PB partial sums; the two-dimensional form keeps rows + columns + c sums.
static inline size_t bitsum_per_group(const MsmPlan &p) {
    const size_t one_d = (size_t)p.c * p.PB, two_d = ((size_t)1 << p.lb) + ((size_t)1 << p.hb) + p.c;
    return p.lb && two_d > one_d ? two_d : one_d;
}

// ---- fused batches. How many of k scalar vectors of n scalars one launch set takes (0: none; one launch set per vector). Fusing pays
// when the MSMs are short (a lone short MSM is pure launch/dependency latency, ~0.4 ms whatever its size): the vectors become K times the
// bucket groups of ONE sort / accumulate / reduce pass. Its size is priced by the single-pass sort's LDS counters; for wide_ok
// (HyperKZG.open's long levels, zero-padded rows) on a wide-window handle by the two-pass sort's coarse bins at the most fine bits the
// table allows. At most 2^22 scalars per set. The set of that size is then planned: it is fused only if it sorts in LDS or in two
// passes under the current switches (a set that would fall back to the global-atomic sort is not fused at all). hp: the handle's plan.
static size_t fuse_set_size(const MsmPlan &hp, size_t table_n, size_t n, size_t k, bool wide_ok, MsmPlan &set) {
    if (n == 0 || k < 2 || !env_int("ZG_MSM_BATCH_FUSE", 1)) return 0;
    const size_t set_buckets = (size_t)hp.NB * hp.G;
    size_t cap = LDS_SORT_BYTES / 4 / set_buckets;
    if (cap < 2 && wide_ok) {
        const int fb = fine_bits((size_t)hp.L * table_n, FINE_BITS_MAX);
        if (fb >= FINE_BITS_MIN) cap = ((size_t)COARSE_BINS_MAX << fb) / set_buckets;
    }
    const size_t by_size = ((size_t)1 << 22) / n;
    if (cap > by_size) cap = by_size;
    if (cap < 2) return 0;
    const size_t kc = k < cap ? k : cap;
    const zg_msm_config cfg{hp.c, hp.L, 0};
    if (plan_msm(n, &cfg, kc, table_n, set) != ZG_OK || set.sort == MsmSort::ATOMIC) return 0;
    return kc;
}

}  // namespace zg
