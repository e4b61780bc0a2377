// field_vec_host.cpp — the lane functions of the field-vector kernels (zolt_amd/csrc/field_vec.hip.h) run on the CPU: the same header,
// compiled for the host. tests/test_field_vectors_model.py builds it with
//     hipcc -x hip --offload-host-only -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/field_vec_host.cpp
// once as it is and once with -fsanitize=address,undefined (a stand-alone program: nothing here is loaded into another process). The
// function qualifiers are the only things replaced.
//
// stdin:  "<field> <op> <n>\n", four u64 (x; unused by op 0), then n elements of four u64, binary. field 0 = Fr, 1 = Fp.
// stdout: op 0: n elements — fv_inv_group over every group of E consecutive elements (n a multiple of E)
//         op 1: n / E elements — fv_horner_chunk of every chunk of E consecutive elements at x (n a multiple of E)
//         op 2: one element — Horner's rule over all n coefficients as fv_horner_kernel composes it: chunk values weighed by
//               fv_chunk_weight from fv_ladder_fill's ladder, coefficients past n zero, summed with fe_add
#define ZG_DEV __host__ __device__ inline
#define ZG_DEV_CALL static __host__ __device__ __attribute__((noinline))
#include <stdio.h>

#include <vector>

#include "field_vec.hip.h"

template <class P>
static int run(int op, unsigned long n) {
    using F = zg::Fe<P>;
    constexpr int E = zg::FV_E;
    alignas(16) uint64_t xw[4];  // fe_load reads two 16-byte vectors
    std::vector<uint64_t> in(4 * n), out;
    if (fread(xw, sizeof(uint64_t), 4, stdin) != 4 || fread(in.data(), sizeof(uint64_t), in.size(), stdin) != in.size()) {
        fprintf(stderr, "field_vec_host: short input\n");
        return 2;
    }
    const F x = zg::fe_load<P>(xw);
    if (op == 0 || op == 1) {
        if (n % E) {
            fprintf(stderr, "field_vec_host: n must be a multiple of %d\n", E);
            return 2;
        }
        out.assign(op == 0 ? 4 * n : 4 * (n / E), 0);
        for (unsigned long g = 0; g < n / E; g++) {
            F v[E];
            for (int k = 0; k < E; k++) v[k] = zg::fe_load<P>(&in[4 * (g * E + k)]);
            if (op == 0) {
                zg::fv_inv_group<P, E>(v);
                for (int k = 0; k < E; k++) zg::fe_store(&out[4 * (g * E + k)], v[k]);
            } else {
                zg::fe_store(&out[4 * g], zg::fv_horner_chunk<P, E>(v, x));
            }
        }
    } else {
        out.assign(4, 0);
        std::vector<F> ladder(zg::FV_LADDER);
        const unsigned long chunks = (n + E - 1) / E;
        const int nbits = zg::fv_index_bits(chunks ? chunks : 1);
        zg::fv_ladder_fill<P, E>(x, ladder.data(), nbits);
        F sum = F::zero();
        for (unsigned long j = 0; j < chunks; j++) {
            F v[E];
            for (int k = 0; k < E; k++) v[k] = j * E + k < n ? zg::fe_load<P>(&in[4 * (j * E + k)]) : F::zero();
            sum = zg::fe_add(sum, zg::fe_mul(zg::fv_horner_chunk<P, E>(v, x), zg::fv_chunk_weight<P>(ladder.data(), j, nbits)));
        }
        zg::fe_store(out.data(), sum);
    }
    return fwrite(out.data(), sizeof(uint64_t), out.size(), stdout) == out.size() ? 0 : 1;
}

int main() {
    int field = -1, op = -1;
    unsigned long n = 0;
    if (scanf("%d %d %lu", &field, &op, &n) != 3 || fgetc(stdin) != '\n' || field < 0 || field > 1 || op < 0 || op > 2 || n > (1ul << 20)) {
        fprintf(stderr, "field_vec_host: bad header (field 0..1, op 0..2, n <= 2^20)\n");
        return 2;
    }
    return field == 0 ? run<zg::FrParams>(op, n) : run<zg::FpParams>(op, n);
}
