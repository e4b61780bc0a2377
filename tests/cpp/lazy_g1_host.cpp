// lazy_g1_host.cpp — the record format of zg_selftest_lazy_g1 (zolt_amd/csrc/lazy_selftest.hip.h) run on the CPU: the same headers,
// the same functions, compiled for the host. tests/test_lazy_group_law_host.py builds it with
//     hipcc -x hip --offload-host-only -DZG_F29_SERIAL -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/lazy_g1_host.cpp
// ZG_F29_SERIAL takes the compiler forms of the products (the inline-assembly forms exist on the device only), and the quad ops are left
// out (they move data with DPP). Everything else — the biased subtractions, the carry step, the zero test, the exceptional finish, the
// class arithmetic — is the code the kernels run.
//
// stdin:  "<op> <n>\n" then n records of ZG_LAZY_IN_WORDS u32, binary.   stdout: n records of ZG_LAZY_OUT_WORDS u32, binary.
#define ZG_DEV __host__ __device__ inline
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lazy_selftest.hip.h"

int main() {
    int op = -1;
    unsigned long n = 0;
    if (scanf("%d %lu", &op, &n) != 2 || fgetc(stdin) != '\n' || op < 0 || op >= zg::LAZY_MADD4 || n == 0 || n > (1ul << 20)) {
        fprintf(stderr, "lazy_g1_host: bad header (op 0..6, 1 <= n <= 2^20)\n");
        return 2;
    }
    std::vector<uint32_t> in(n * ZG_LAZY_IN_WORDS), out(n * ZG_LAZY_OUT_WORDS, 0u);
    if (fread(in.data(), sizeof(uint32_t), in.size(), stdin) != in.size()) {
        fprintf(stderr, "lazy_g1_host: short input\n");
        return 2;
    }
    for (unsigned long i = 0; i < n; i++) zg::lazy_record(op, &in[i * ZG_LAZY_IN_WORDS], &out[i * ZG_LAZY_OUT_WORDS]);
    return fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
