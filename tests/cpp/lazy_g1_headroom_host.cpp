// lazy_g1_headroom_host.cpp — the un-carried linear forms of the mixed addition (zolt_amd/csrc/fp29.hip.h: f29_sub7_raw,
// f29_pmsub45_raw, f29_neg4_raw; g1_29.hip.h: xyzz29_madd_nz) against the carried forms they replace, on the CPU: the kernels' own
// headers compiled for the host, every record run TWICE from one binary through the record format of zg_selftest_lazy_g1
// (lazy_selftest.hip.h). tests/test_lazy_g1_headroom_host.py builds it with
//     hipcc -x hip --offload-host-only -DZG_F29_SERIAL -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/lazy_g1_headroom_host.cpp
// and once more with -fsanitize=address,undefined (a stand-alone program: an unsigned wrap is not a report, a signed overflow or a
// shift past the word is).
//
// stdin:  "<op> <n>\n" (op = MADD, START or LIN) then n records of ZG_LAZY_IN_WORDS u32, binary.
// stdout: 2 n records of ZG_LAZY_OUT_WORDS u32: record i as given (MADD / START: the un-carried addition; LIN: whatever its flags ask
//         for), then record i in the carried reference form (MADD / START: flags | LAZY_MADD_CARRY_ALL; LIN: flags & ~LAZY_LIN_RAW).
// Exit status 3 if the two forms of an addition differ in any word: they must agree limb for limb, not only mod p.
#define ZG_DEV __host__ __device__ inline
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lazy_selftest.hip.h"

int main() {
    int op = -1;
    unsigned long n = 0;
    if (scanf("%d %lu", &op, &n) != 2 || fgetc(stdin) != '\n' || (op != zg::LAZY_MADD && op != zg::LAZY_START && op != zg::LAZY_LIN) || n == 0 ||
        n > (1ul << 20)) {
        fprintf(stderr, "lazy_g1_headroom_host: bad header (op 0, 1 or 6, 1 <= n <= 2^20)\n");
        return 2;
    }
    std::vector<uint32_t> in(n * ZG_LAZY_IN_WORDS), out(2 * n * ZG_LAZY_OUT_WORDS, 0u);
    if (fread(in.data(), sizeof(uint32_t), in.size(), stdin) != in.size()) {
        fprintf(stderr, "lazy_g1_headroom_host: short input\n");
        return 2;
    }
    unsigned long differ = 0;
    for (unsigned long i = 0; i < n; i++) {
        uint32_t rec[ZG_LAZY_IN_WORDS];
        memcpy(rec, &in[i * ZG_LAZY_IN_WORDS], sizeof rec);
        uint32_t *o_new = &out[2 * i * ZG_LAZY_OUT_WORDS], *o_ref = o_new + ZG_LAZY_OUT_WORDS;
        zg::lazy_record(op, rec, o_new);
        if (op == zg::LAZY_LIN) rec[90] &= ~zg::LAZY_LIN_RAW;
        else rec[90] |= zg::LAZY_MADD_CARRY_ALL;
        zg::lazy_record(op, rec, o_ref);
        if (op != zg::LAZY_LIN && memcmp(o_new, o_ref, ZG_LAZY_OUT_WORDS * sizeof(uint32_t)) != 0) {
            if (differ++ == 0) fprintf(stderr, "lazy_g1_headroom_host: record %lu: the un-carried addition differs from the carried one\n", i);
        }
    }
    if (fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) != out.size()) return 1;
    return differ ? 3 : 0;
}
