// dory_vsetup_host.cpp — the lane decode and the segment table of the Dory verifier-setup kernels on the CPU: compiles the kernels' own
// header (zolt_amd/csrc/dory_vsetup.hip.h, pure integer code) with any C++ compiler. tests/test_dory_vsetup_model.py builds it, also with
// -fsanitize=address,undefined, and reads its output.
//   dory_vsetup_host K   prints "L lanes segments", one "S s offset" per offset of the table (segments + 1 of them), and one
//                        "P lane family level offset i1 i2" per lane
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dory_vsetup.hip.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const uint32_t K = (uint32_t)strtoul(argv[1], nullptr, 10);
    if (K > 16) return 2;
    const size_t lanes = zg::dv_lanes(K), segs = zg::dv_segments(K);
    printf("L %zu %zu\n", lanes, segs);
    std::vector<size_t> seg(segs + 1);
    for (size_t s = 0; s <= segs; s++) {
        seg[s] = zg::dv_seg(K, (uint32_t)s);
        printf("S %zu %zu\n", s, seg[s]);
    }
    std::vector<zg::DvPair> pairs(lanes);  // (held in an array so that a sanitizer sees every index the decode yields)
    for (size_t i = 0; i < lanes; i++) pairs[i] = zg::dv_decode(K, (uint32_t)i);
    for (size_t i = 0; i < lanes; i++)
        printf("P %zu %u %u %u %u %u\n", i, pairs[i].family, pairs[i].level, pairs[i].offset, pairs[i].i1, pairs[i].i2);
    return 0;
}
