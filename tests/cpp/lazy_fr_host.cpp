// lazy_fr_host.cpp — the record format of zg_selftest_lazy_fr (zolt_amd/csrc/lazy_fr_selftest.hip.h) run on the CPU: the same headers,
// the same functions, compiled for the host. tests/test_lazy_fr_host.py builds it with
//     hipcc -x hip --offload-host-only -DZG_F29_SERIAL -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/lazy_fr_host.cpp
// and once more with -fsanitize=address,undefined (a stand-alone program: nothing here is loaded into another process).
// Every op except FR_BLOCKSUM, whose lane movements exist on the device only.
//
// stdin:  "<op> <n>\n" then n records of ZG_LAZY_FR_IN_WORDS u32, binary.   stdout: n records of ZG_LAZY_FR_OUT_WORDS u32, binary.
#define ZG_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// acc9_reduce's quotient estimate: the device intrinsic's host counterpart
__host__ inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b) {
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
}

#include "lazy_fr_selftest.hip.h"

int main() {
    int op = -1;
    unsigned long n = 0;
    if (scanf("%d %lu", &op, &n) != 2 || fgetc(stdin) != '\n' || op < 0 || op >= zg::FR_BLOCKSUM || n == 0 || n > (1ul << 20)) {
        fprintf(stderr, "lazy_fr_host: bad header (op 0..7, 1 <= n <= 2^20)\n");
        return 2;
    }
    std::vector<uint32_t> in(n * ZG_LAZY_FR_IN_WORDS), out(n * ZG_LAZY_FR_OUT_WORDS, 0u);
    if (fread(in.data(), sizeof(uint32_t), in.size(), stdin) != in.size()) {
        fprintf(stderr, "lazy_fr_host: short input\n");
        return 2;
    }
    for (unsigned long i = 0; i < n; i++) zg::lazy_fr_record(op, &in[i * ZG_LAZY_FR_IN_WORDS], &out[i * ZG_LAZY_FR_OUT_WORDS]);
    return fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
