// fp12_wave_map.hip.h — which lane of a wavefront multiplies which coefficients of a cooperative Fp12 product, which lanes are summed
// into which output, and which lanes take the Fp2 products of a Miller step (fp12_wave.hip.h, pairing_wave.hip.h). Pure integer code
// without a HIP type, so that the same text compiles for the host with any C++ compiler (tests/cpp/pairing_wave_host.cpp).
//
// An Fp12 is sum c_k w^k, k < 6, over Fp2 with w^6 = xi. Lane L of the 64 HOLDS the coefficient of column L % 6 — every column is held
// by ten or eleven lanes, all with the same bits — so an element costs a lane one Fp2 (16 registers). For a product a * b the 36 BUSY
// lanes L = 6 i + j form a_i * b_j: b_j is what the lane holds, a_i is fetched from lane i (which holds column i). The partial product
// is multiplied by xi where i + j >= 6, and every lane of column k then sums the six busy lanes (t, (k - t) mod 6), t < 6. Lanes 36..63
// run the same instructions on a row of their own ((L / 6) % 6, so that their fetch has a source) and nobody reads what they form.
//
// The Fp2 products of a Miller step (double_in_place, add_in_place, the line's two scalings) are independent within a LEVEL; product s
// of a level is formed by lane 36 + s — outside the busy 36, so that a level can run in the same instructions as an Fp12 product — and
// read back by all lanes from there. The point R, P and Q are replicated: every lane holds them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZG_FPW_FN __host__ __device__ static inline
#else
#define ZG_FPW_FN static inline
#endif

namespace zg {

enum : int { FPW_LANES = 64, FPW_DEG = 6, FPW_BUSY = 36, FPW_SIDE0 = 36, FPW_SIDE_MAX = FPW_LANES - FPW_SIDE0 };

ZG_FPW_FN int fpw_col(int lane) { return lane % FPW_DEG; }                    // the coefficient a lane holds, and its b_j
ZG_FPW_FN int fpw_row(int lane) { return (lane / FPW_DEG) % FPW_DEG; }        // its a_i: fetched from lane fpw_row(lane)
ZG_FPW_FN bool fpw_busy(int lane) { return lane < FPW_BUSY; }                 // its partial product is read by somebody
ZG_FPW_FN bool fpw_xi(int lane) { return fpw_row(lane) + fpw_col(lane) >= FPW_DEG; }  // w^(i + j) = xi w^(i + j - 6)
ZG_FPW_FN int fpw_src(int col, int t) { return FPW_DEG * t + (col + FPW_DEG - t) % FPW_DEG; }  // term t of column col's sum: lane (t, col - t)

// the sparse operand of mul_by_034 — c0 at w^0, c3 at w^1, c4 at v w = w^3 — as the column form of an Fp12 whose other columns are
// zero: which of (c0, c3, c4) a column holds, or -1 for zero. The product is then the general one: 18 lanes multiply by zero.
ZG_FPW_FN int fpw_sparse_slot(int col) { return col == 0 ? 0 : col == 1 ? 1 : col == 3 ? 2 : -1; }

// memory order of fp12_load / fp12_store (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> the Fp2 slot of column k: c_{k & 1}.c_{k >> 1}
ZG_FPW_FN int fpw_mem_slot(int col) { return (col & 1) * 3 + (col >> 1); }

// the levels of the Miller steps and how many independent Fp2 products each has (pairing_wave.hip.h names them)
enum : int { PW_DBL_LEVELS = 3, PW_ADD_LEVELS = 4 };
ZG_FPW_FN int pw_dbl_products(int level) { return level == 0 ? 5 : level == 1 ? 3 : 4; }
ZG_FPW_FN int pw_add_products(int level) { return level == 0 ? 2 : level == 1 ? 6 : level == 2 ? 3 : 4; }
ZG_FPW_FN int pw_side_lane(int s) { return FPW_SIDE0 + s; }  // product s of a level

}  // namespace zg
