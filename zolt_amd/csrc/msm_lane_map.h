// msm_lane_map.h — the index map of msm_rowcol_lane_kernel (msm.hip): which bucket, which LDS slot and which output every lane, quad
// and stage of the radix-4 row / column sums touches. Plain constexpr functions (host and device, no HIP header): the kernel calls
// them, and tests/cpp/lane_tail_map_check.cpp replays them on the CPU.
//
// The buckets of one set are a 2^hb x 2^lb matrix, digit magnitude k = h * 2^lb + l (k = 0 has no bucket). Its 2^hb rows and 2^lb
// columns are the set's LINES: line L < 2^hb is row L (2^lb elements), line 2^hb + l is column l (2^hb elements), and the sum of line
// L goes to slot L of the set's rc array — the layout msm_rowcol_kernel writes. A workgroup of 256 threads sums LINES = 4 consecutive
// lines (all rows or all columns: both counts are multiples of four) of 2^m elements each, m = lb or hb, in m / 2 stages. Every
// unit of a stage adds four inputs with three additions:
//   stage 1         unit = lane  t < 4 * 2^m / 4: four consecutive elements of one line, read from the buckets
//   stage s >= 2    unit u reads the four stage-(s-1) results 4u .. 4u+3
//   the last two stages' units are quads of lanes (16 and 4 of them), every earlier stage's are single lanes
// A result lives in the LDS slot of its unit's FIRST input (unit u of stage s: slot u * 4^(s-1)), so a slot written in a stage is
// read in that stage by its writer alone, and the four units of the last stage are the four lines of the workgroup.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define ZG_LANE_MAP_FN __attribute__((host)) __attribute__((device)) constexpr
#else
#define ZG_LANE_MAP_FN constexpr
#endif

namespace zg {
namespace lane_map {

static constexpr uint32_t LINES = 4;    // rows or columns per workgroup
static constexpr uint32_t SLOTS = 256;  // LDS slots of 144 bytes (36 KiB, as block_sum_xyzz29)

// line lengths the stages tile exactly: 64 (lane, quad, quad) and 256 (lane, lane, quad, quad) elements
ZG_LANE_MAP_FN bool line_bits_ok(int m) { return m == 6 || m == 8; }

ZG_LANE_MAP_FN uint32_t workgroups(int lb, int hb) { return ((1u << hb) + (1u << lb)) / LINES; }
ZG_LANE_MAP_FN int line_bits(int lb, int hb, uint32_t line) { return line < (1u << hb) ? lb : hb; }
// digit magnitude of element e of a line (0: no bucket; bucket k is stored at index k - 1)
ZG_LANE_MAP_FN uint32_t element(int lb, int hb, uint32_t line, uint32_t e) {
    return line < (1u << hb) ? ((line << lb) | e) : ((e << lb) | (line - (1u << hb)));
}

ZG_LANE_MAP_FN int stages(int m) { return m / 2; }
ZG_LANE_MAP_FN uint32_t units(int m, int s) { return (LINES << m) >> (2 * s); }
ZG_LANE_MAP_FN bool quad_stage(int m, int s) { return s + 2 > stages(m); }

// stage 1, unit u: its line within the workgroup and the first of its four consecutive elements
ZG_LANE_MAP_FN uint32_t first_line(int m, uint32_t u) { return u >> (m - 2); }
ZG_LANE_MAP_FN uint32_t first_element(int m, uint32_t u) { return (u & ((1u << (m - 2)) - 1u)) * 4u; }

// LDS slots: input i = 0 .. 3 of unit u in stage s >= 2, and the slot a unit's result is written to (stages before the last)
ZG_LANE_MAP_FN uint32_t in_slot(int s, uint32_t u, uint32_t i) { return (4u * u + i) << (2 * (s - 2)); }
ZG_LANE_MAP_FN uint32_t out_slot(int s, uint32_t u) { return u << (2 * (s - 1)); }

}  // namespace lane_map
}  // namespace zg
