// dory_commit_host.cpp — the lane functions of the Dory commitment kernels (zolt_amd/csrc/dory_commit.hip.h) run on the CPU: the same
// header, the same functions, compiled for the host. tests/test_dory_commit_host.py builds it with
//     hipcc -x hip --offload-host-only -DZG_F29_SERIAL -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/dory_commit_host.cpp
// and checks what it prints against tests/dory_commit_model.py. The digit table is built by dc_table_column, a row by dc_lane_sum per
// lane and the kernel's tree order of xyzz29_add, a 64-bit polynomial by dc_horner over its eight byte sums.
//
// stdin (text, numbers in hex):
//   <ncols>                                   then ncols lines   <inf> <x: 4 words> <y: 4 words>      (Montgomery, 64-bit words)
//   any number of queries   <words> <shift> <bits> <lanes> <nvirt> <has_aux> <n>   then n lines   <lo> <hi> <sign>
//     nvirt = 1: the digit (entry >> shift) & (2^bits - 1);  nvirt = 8: the eight bytes of the 64-bit entry (shift, bits ignored)
// stdout per query:   D <digit of every entry, virtual polynomial 0>     P <flag> <x: 4 words> <y: 4 words>
#define ZG_DEV __host__ __device__ inline
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dory_commit.hip.h"

using namespace zg;

template <class T>
static T *aligned(size_t n) {
    return reinterpret_cast<T *>(aligned_alloc(64, (n * sizeof(T) + 63) / 64 * 64));
}

int main() {
    unsigned ncols = 0;
    if (scanf("%x", &ncols) != 1 || ncols < 1 || ncols > 64) return 2;
    uint64_t *g1 = aligned<uint64_t>(8 * (size_t)ncols);
    std::vector<uint8_t> g1_inf(ncols);
    char *table = aligned<char>((size_t)ncols * DC_DIGITS * 64), *rec = aligned<char>(DC_DIGITS * 144), *pref = aligned<char>(DC_DIGITS * 48);
    for (unsigned c = 0; c < ncols; c++) {
        unsigned inf = 0;
        if (scanf("%x", &inf) != 1) return 2;
        for (int w = 0; w < 8; w++)
            if (scanf("%lx", (unsigned long *)&g1[8 * c + w]) != 1) return 2;
        g1_inf[c] = (uint8_t)inf;
        dc_table_column(affine_load(g1 + 8 * c), inf != 0, table + 64 * (size_t)DC_DIGITS * c, rec, 144, pref, 48);
    }
    unsigned words, shift, bits, lanes, nvirt, has_aux, n;
    while (scanf("%x %x %x %x %x %x %x", &words, &shift, &bits, &lanes, &nvirt, &has_aux, &n) == 7) {
        if (words < 1 || words > 2 || n < 1 || n > ncols || lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) || (nvirt != 1 && nvirt != 8)) return 2;
        std::vector<uint64_t> data((size_t)words * n);
        std::vector<uint8_t> aux(n);
        for (unsigned i = 0; i < n; i++) {
            unsigned long lo, hi;
            unsigned sign;
            if (scanf("%lx %lx %x", &lo, &hi, &sign) != 3) return 2;
            data[(size_t)words * i] = lo;
            if (words == 2) data[2 * (size_t)i + 1] = hi;
            aux[i] = (uint8_t)sign;
        }
        DcVirt v = {};
        v.data = data.data();
        v.aux = has_aux ? aux.data() : nullptr;
        v.len = n;
        v.words = words;
        v.sigma = 0;
        while ((1u << v.sigma) < n) v.sigma++;
        v.rows = 1;
        char *sums = aligned<char>(8 * 144);
        for (unsigned w = 0; w < nvirt; w++) {
            v.shift = nvirt == 8 ? 8 * w : shift;
            v.mask = nvirt == 8 ? 255u : (1u << bits) - 1u;
            if (w == 0) {
                printf("D");
                for (unsigned i = 0; i < n; i++) printf(" %x", dc_digit(v.data, v.words, i, v.shift, v.mask));
                printf("\n");
            }
            std::vector<XYZZ29> val(lanes);
            for (unsigned l = 0; l < lanes; l++) val[l] = dc_lane_sum(table, g1_inf.data(), v, 0, l, lanes);
            for (unsigned s = 32; s >= 1; s >>= 1)  // the kernel's tree: lane i takes lane i + s
                if (s < lanes)
                    for (unsigned i = 0; i + s < lanes; i++) val[i] = xyzz29_add(val[i], val[i + s]);
            xyzz29_store(sums + 144 * (size_t)w, val[0]);
        }
        alignas(16) uint64_t out[10];
        dc_store_record(out, nvirt == 8 ? dc_horner(sums, 144) : xyzz29_load(sums));
        printf("P %lx", (unsigned long)out[8]);
        for (int w = 0; w < 8; w++) printf(" %lx", (unsigned long)out[w]);
        printf("\n");
        free(sums);
    }
    return 0;
}
