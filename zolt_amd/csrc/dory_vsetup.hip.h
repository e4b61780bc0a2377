// dory_vsetup.hip.h — which pair index i of the verifier setup's pair set (DvPairs) is which pair, and where the segments of its Miller values start
// (dory_vsetup.hip). Pure integer code without a HIP type, so that the same text compiles for the host with any C++ compiler
// (tests/cpp/dory_vsetup_host.cpp).
//
// DoryVerifierSetup.fromSRS (src/zkvm/preprocessing.zig:889-973) pairs, for k = 1..K and h = 2^(k-1), three families of index pairs
// (g1 index, g2 index) over the first N = 2^K generators:
//   diagonal  (i, i)          i < N           chi[k]'s new factor is the product over h <= i < 2h (:935), chi[0] the pair (0, 0) (:914)
//   upper     (h + j, j)      j < h           delta_1r[k] (:929)
//   lower     (j, h + j)      j < h           delta_2r[k] (:932)
// N + (N - 1) + (N - 1) = 3N - 2 pairs. The lanes are numbered segment-major — the diagonal first, then the upper family level by
// level, then the lower — so that every product fromSRS forms is a contiguous range of lanes:
//   lane i                    i < N           diagonal (i, i); segment 0 = {0}, segment k = [h, 2h)
//   lane N + t                t < N - 1       upper: t + 1 = h + j with h the top bit of t + 1, i.e. the pair (t + 1, t + 1 - h)
//   lane 2N - 1 + t           t < N - 1       lower: the pair (t + 1 - h, t + 1)
// and the 3K + 1 segments are the 3K + 2 ascending offsets of dv_seg: K + 1 diagonal, K upper, K lower.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZG_DV_FN __host__ __device__ static inline
#else
#define ZG_DV_FN static inline
#endif

namespace zg {

enum : uint32_t { DV_DIAGONAL = 0, DV_UPPER = 1, DV_LOWER = 2 };

struct DvPair {
    uint32_t family, level, offset;  // level k (0 only for the pair (0, 0)), offset j < h within the level
    uint32_t i1, i2;                 // the generators: g1_vec[i1] against g2_vec[i2]
};

ZG_DV_FN uint32_t dv_log2(uint32_t x) {  // floor(log2 x), x >= 1
    uint32_t r = 0;
    while (x >> (r + 1)) r++;
    return r;
}

// K = floor(log2 n_g1) <= 16
ZG_DV_FN size_t dv_lanes(uint32_t K) { return 3 * ((size_t)1 << K) - 2; }
ZG_DV_FN size_t dv_segments(uint32_t K) { return 3 * (size_t)K + 1; }

// offset s of the segment table, s <= 3K + 1: segment s is [dv_seg(K, s), dv_seg(K, s + 1)). Segments 0..K are the diagonal levels,
// K + k the upper family of level k, 2K + k the lower family of level k (k = 1..K).
ZG_DV_FN size_t dv_seg(uint32_t K, uint32_t s) {
    const size_t N = (size_t)1 << K;
    if (s <= K) return s ? (size_t)1 << (s - 1) : 0;
    if (s <= 2 * K) return N + ((size_t)1 << (s - K - 1)) - 1;
    return 2 * N - 1 + ((size_t)1 << (s - 2 * K - 1)) - 1;
}

// lane < dv_lanes(K)
ZG_DV_FN DvPair dv_decode(uint32_t K, uint32_t lane) {
    const uint32_t N = 1u << K;
    DvPair p;
    if (lane < N) {
        p.family = DV_DIAGONAL;
        p.level = lane ? dv_log2(lane) + 1 : 0;
        p.offset = lane ? lane - (1u << (p.level - 1)) : 0;
        p.i1 = p.i2 = lane;
        return p;
    }
    const bool upper = lane < 2 * N - 1;
    const uint32_t i = lane - (upper ? N : 2 * N - 1) + 1;  // 1 <= i < N: h + j
    p.family = upper ? DV_UPPER : DV_LOWER;
    p.level = dv_log2(i) + 1;
    p.offset = i - (1u << (p.level - 1));
    p.i1 = upper ? i : p.offset;
    p.i2 = upper ? p.offset : i;
    return p;
}

}  // namespace zg
