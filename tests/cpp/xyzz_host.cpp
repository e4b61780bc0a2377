// xyzz_host.cpp — the record format of zg_selftest_xyzz (zolt_amd/csrc/xyzz_selftest.hip.h) run on the CPU: the same headers, the same
// functions (xyzz.hip.h over Fp and over Fp2, fe_inv_safegcd), compiled for the host. tests/test_xyzz_group_law_host.py builds it with
//     hipcc -x hip --offload-host-only -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/xyzz_host.cpp
// once as it is and once with -fsanitize=address,undefined (a stand-alone program: nothing here is loaded into another process), and
// tests/test_xyzz_mutants_host.py builds it with a directory that holds ONE changed header first on the include path. The function
// qualifiers are the only things replaced.
//
// stdin:  "<group> <op> <n>\n" then n records of 8 W + 6 u64, binary (W = 4: group 0, Fp; W = 8: group 1, Fp2).
// stdout: n records of 4 W + 2 u64, binary.
#define ZG_DEV __host__ __device__ inline
#define ZG_DEV_CALL static __host__ __device__ __attribute__((noinline))
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xyzz_selftest.hip.h"

template <class F>
static int run(int op, unsigned long n) {
    constexpr int IN = zg::XyzzRec<F>::IN_WORDS, OUT = zg::XyzzRec<F>::OUT_WORDS;
    std::vector<uint64_t> in(n * IN), out(n * OUT, 0);
    if (fread(in.data(), sizeof(uint64_t), in.size(), stdin) != in.size()) {
        fprintf(stderr, "xyzz_host: short input\n");
        return 2;
    }
    for (unsigned long i = 0; i < n; i++) zg::xyzz_record<F>(op, &in[i * IN], &out[i * OUT]);
    return fwrite(out.data(), sizeof(uint64_t), out.size(), stdout) == out.size() ? 0 : 1;
}

int main() {
    int group = -1, op = -1;
    unsigned long n = 0;
    if (scanf("%d %d %lu", &group, &op, &n) != 3 || fgetc(stdin) != '\n' || group < 0 || group > 1 || op < 0 || op >= zg::XS_NOPS || n == 0 ||
        n > (1ul << 16)) {
        fprintf(stderr, "xyzz_host: bad header (group 0..1, op 0..8, 1 <= n <= 2^16)\n");
        return 2;
    }
    return group == 0 ? run<zg::Fp>(op, n) : run<zg::Fp2>(op, n);
}
