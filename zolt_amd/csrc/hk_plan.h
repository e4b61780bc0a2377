// hk_plan.h — the level plan of HyperKZG.open (host only, no HIP header): which levels the fold reaches, where each level's quotient
// goes and how the quotients are grouped into commits. hk_open_device (hyperkzg.hip) sizes its arena, folds and commits from this one
// plan; tests/cpp/hk_plan_check.cpp checks it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zg {

// Levels whose quotient has at most HK_SMALL entries are committed TOGETHER at the end: their quotients are written
// into rows of one zero-padded matrix (a zero scalar contributes no digit, so commit(q) over bases[0..row length) is
// unchanged) and handed to zg_msm_g1_batch_dev, which fuses short vectors into one launch set — a lone short MSM is
// ~0.4 ms of launch latency, and there are log2(HK_SMALL) + 1 of them.
static constexpr size_t HK_SMALL = 16384;  // = the narrow-window side table of a wide-window handle (msm.hip)
static constexpr int HK_MAX_LEVELS = 64;   // the table halves at every level

enum class HkDest : uint8_t { SHORT_ROW, LONG_ROW, OWN };  // a row of the short matrix, a row of the long matrix, a buffer of its own

struct HkLevel {
    size_t half;   // pairs folded = entries of the quotient
    size_t nc;     // entries committed: commit() takes min(evals.len, srs.len)
    HkDest dest;
    size_t off;    // of the quotient in the arena, in entries
    size_t count;  // entries the fold writes there: nc into a matrix row (zeros stay behind them), half into an own buffer
};

// `rows` consecutive levels from `first`, zero-padded to `len` = the first row's nc (the longest), at `off` in the arena; rows == 0: none.
// The matrix is zeroed as a whole before the folds, and row r's result is result first + r.
struct HkMatrix {
    size_t first, rows, len, off;
    size_t entries() const { return rows * len; }
};

struct HkPlan {
    HkLevel level[HK_MAX_LEVELS];
    size_t computed;  // levels folded; the reference stops at half == 0 and leaves the remaining quotients unset: identity
    HkMatrix small, lng;
    size_t long_row_len[HK_MAX_LEVELS];  // live entries of lng's rows: the fused commit's sort skips the padding behind them
    size_t arena;                        // entries in all
};

// The long levels go out the same way as the short ones: rows of one zero-padded matrix, committed by ONE fused launch set on a helper
// stream (msm_batch_dev_wide) — one sort, one accumulation over all levels' digits (as many as a single MSM of twice the first level's
// size has) and one reduction, instead of five or six launch sets that overlap badly.
// fuse_mode (ZG_HK_FUSE_LONG) 0: one launch set per long level. 1 (default): all long levels in one matrix. 2: the first long level —
// half of all live scalars — keeps a buffer and a launch set of its own, and the matrix starts at the second long level with its row
// length (the padding that the digit and sort kernels walk shrinks from 2.6 M to 1.5 M scalars at 2^20 evaluations). Mode 2 was the
// default until a kernel trace of round 4 showed what "side by side" means on the device: the second set's sort kernels (whole-CU
// workgroups) crawl while the first set's accumulation owns the register files (colscan 12 -> 360 us, fine_place 77 -> 290 us), so its
// accumulation starts when the first one ends and two reduction chains are exposed instead of one — 2^20 evaluations from a host table:
// mode 2 3.30-3.41 ms, mode 1 3.08-3.13 ms, mode 0 3.72 ms (tools/ab_open.py, profiles/r4h_open_modes.txt).
// A matrix needs two rows (nothing to fuse otherwise), mode 2 three long levels (with two it is mode 1), and the long matrix helper
// streams (`fork`): its commit must not sit on the caller's stream behind everything else.
static inline HkPlan hk_plan(size_t n_evals, size_t num_vars, size_t srs_len, unsigned fuse_mode, bool fork) {
    HkPlan p{};
    // nc never grows from one level to the next: the long levels come first, the short ones follow, each run consecutive
    size_t n_long = 0;
    for (size_t len = n_evals; p.computed < num_vars && len / 2; len /= 2) {
        HkLevel &l = p.level[p.computed++];
        l.half = len / 2;
        l.nc = l.half < srs_len ? l.half : srs_len;
        if (l.nc > HK_SMALL) n_long++;
    }
    const size_t n_short = p.computed - n_long, lone = fuse_mode == 2 && n_long >= 3 ? 1 : 0;
    if (n_short >= 2) p.small = HkMatrix{n_long, n_short, p.level[n_long].nc, 0};
    if (fork && fuse_mode && n_long >= 2) p.lng = HkMatrix{lone, n_long - lone, p.level[lone].nc, p.small.entries()};
    p.arena = p.small.entries() + p.lng.entries();  // the matrices, then one buffer per level outside them
    for (size_t i = 0; i < p.computed; i++) {
        HkLevel &l = p.level[i];
        const HkMatrix *m = i - p.small.first < p.small.rows ? &p.small : i - p.lng.first < p.lng.rows ? &p.lng : nullptr;
        if (m) {
            l.dest = m == &p.small ? HkDest::SHORT_ROW : HkDest::LONG_ROW;
            l.off = m->off + (i - m->first) * m->len;
            l.count = l.nc;
            if (m == &p.lng) p.long_row_len[i - m->first] = l.nc;
        } else {
            l.dest = HkDest::OWN;
            l.off = p.arena;
            l.count = l.half;
            p.arena += l.count;
        }
    }
    return p;
}

}  // namespace zg
