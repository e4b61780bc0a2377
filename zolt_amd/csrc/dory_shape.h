// dory_shape.h — the lengths of one reduce-and-fold round of DoryCommitmentScheme.open (src/poly/commitment/dory.zig:1211-1214,
// :1236-1252, :1291-1304, :1343-1344), in one place: the session (dory.hip) launches by it and a host program (tests/cpp/
// dory_shape_host.cpp) prints it. Plain C++, no HIP.
//
// setup makes 2^sigma G1 and 2^nu G2 generators, nu <= sigma, and open carries two live lengths: current_col_len halves from 2^sigma
// and current_row_len from 2^nu, the latter staying at 1 once it gets there. With nu <= sigma the working length of round t is the
// column length, and everything on the G2 side is cut to the rows that are left:
//   cur  2^(sigma - t)         v1, s2 and g1_vec are live over [0, cur)
//   n2   cur / 2               the halves are [0, n2) and [n2, cur): every "right half" starts at n2, whatever its length
//   row  max(2^nu >> t, 1)     g2_vec, e2_beta and the v2 update run over [0, row)
//   h    min(n2, row)          d1_left/right, c_plus/minus, e2_plus/minus and the folds of v2 and s1 run over h entries of a half
// A session whose generator vectors are both 2^sigma long (openWithTranscript, :1404-1669) is the case nu = sigma: row = cur, h = n2.
#pragma once
#include <stdint.h>

struct DoryRoundShape {
    uint32_t cur, n2, row, h;
};

// round t < sigma of an opening with nu <= sigma <= 31
static inline DoryRoundShape dory_round_shape(uint32_t nu, uint32_t sigma, uint32_t t) {
    DoryRoundShape r;
    r.cur = 1u << (sigma - t);
    r.n2 = r.cur / 2;
    r.row = t < nu ? 1u << (nu - t) : 1u;
    r.h = r.n2 < r.row ? r.n2 : r.row;
    return r;
}
