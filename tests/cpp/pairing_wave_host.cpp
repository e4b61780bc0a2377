// pairing_wave_host.cpp — the lane map of the wave pairing engine on the CPU: compiles the kernels' own header
// (zolt_amd/csrc/fp12_wave_map.hip.h, pure integer code) with any C++ compiler. tests/test_pairing_wave_model.py builds it, also with
// -fsanitize=address,undefined, and reads its output.
//   pairing_wave_host   prints one "L lane row col busy xi mem_slot sparse_slot" per lane of the 64, one "S col t lane" per term of a
//                       column's sum, one "D level products" / "A level products" per level of a doubling / an addition step, and one
//                       "P s lane" per product slot of a level
#include <stdio.h>

#include <vector>

#include "fp12_wave_map.hip.h"

int main() {
    using namespace zg;
    struct Lane {
        int row, col, busy, xi, mem, sparse;
    };
    std::vector<Lane> lanes(FPW_LANES);  // (held in arrays so that a sanitizer sees every index the map yields)
    for (int l = 0; l < FPW_LANES; l++) lanes[l] = Lane{fpw_row(l), fpw_col(l), fpw_busy(l), fpw_xi(l), fpw_mem_slot(fpw_col(l)), fpw_sparse_slot(fpw_col(l))};
    for (int l = 0; l < FPW_LANES; l++) printf("L %d %d %d %d %d %d %d\n", l, lanes[l].row, lanes[l].col, lanes[l].busy, lanes[l].xi, lanes[l].mem, lanes[l].sparse);
    std::vector<int> hits(FPW_LANES, 0);
    for (int c = 0; c < FPW_DEG; c++)
        for (int t = 0; t < FPW_DEG; t++) {
            const int s = fpw_src(c, t);
            hits[s]++;  // out of bounds here is the sanitizer's to report
            printf("S %d %d %d\n", c, t, s);
        }
    for (int k = 0; k < PW_DBL_LEVELS; k++) printf("D %d %d\n", k, pw_dbl_products(k));
    for (int k = 0; k < PW_ADD_LEVELS; k++) printf("A %d %d\n", k, pw_add_products(k));
    for (int s = 0; s < FPW_SIDE_MAX; s++) {
        hits[pw_side_lane(s)]++;
        printf("P %d %d\n", s, pw_side_lane(s));
    }
    return 0;
}
