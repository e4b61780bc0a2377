// pairing_host.cpp — the pairing as ONE lane of the device computes it (zolt_amd/csrc/fp12.hip.h, pairing.hip.h), run on the CPU: the same
// headers, the same functions, compiled for the host. tests/test_pairing_host.py builds it with
//     hipcc -x hip --offload-host-only -std=c++17 -O1 -I zolt_amd/csrc -I include tests/cpp/pairing_host.cpp
// and holds it to tests/pairing_model.py. The function qualifiers and the constant tables' address space are the only things replaced.
//
// stdin:  "<op> <n>\n" then n records of 192 u32 (two Fp12 operands a, b; for the Miller loop a G1 point in words 0..15 and a G2 point in
//         words 16..47), binary.   stdout: n records of 96 u32 (one Fp12), binary.
// op:     17..24 = the ZG_OP_FP12_* codes, 100 = pair_miller, 101 = pair_final_exp, 102 = fp12_mul_by_034 (b's first three Fp2 are c0, c3, c4)
#define ZG_DEV __host__ __device__ inline
#define ZG_DEV_CALL static __host__ __device__ __attribute__((noinline))
#define ZG_PAIR_CONST static const
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pairing.hip.h"
#include "zolt_gpu_internal.h"

static constexpr int IN_WORDS = 192, OUT_WORDS = 96;

int main() {
    int op = -1;
    unsigned long n = 0;
    if (scanf("%d %lu", &op, &n) != 2 || fgetc(stdin) != '\n' || n == 0 || n > (1ul << 16)) {
        fprintf(stderr, "pairing_host: bad header\n");
        return 2;
    }
    std::vector<uint4> in(n * IN_WORDS / 4), out(n * OUT_WORDS / 4);  // 16-byte aligned: the element loads are vector loads
    if (fread(in.data(), sizeof(uint4), in.size(), stdin) != in.size()) {
        fprintf(stderr, "pairing_host: short input\n");
        return 2;
    }
    for (unsigned long i = 0; i < n; i++) {
        const uint64_t *rec = reinterpret_cast<const uint64_t *>(in.data() + i * IN_WORDS / 4);
        zg::Fp12 r;
        if (op == 100) {
            const zg::Affine p = zg::affine_load(rec);
            const zg::G2Affine q = zg::affine_load<zg::Fp2>(rec + 8);
            zg::pair_miller(r, p, q);
        } else {
            zg::Fp12 a = zg::fp12_load(rec);
            const zg::Fp12 b = zg::fp12_load(rec + 48);
            switch (op) {
            case ZG_OP_FP12_MUL: zg::fp12_mul(r, a, b); break;
            case ZG_OP_FP12_SQR: zg::fp12_sqr(r, a); break;
            case ZG_OP_FP12_INV: zg::fp12_inv(r, a); break;
            case ZG_OP_FP12_CONJ: r = zg::fp12_conj(a); break;
            case ZG_OP_FP12_FROB1: zg::fp12_frobenius(r, a, 1); break;
            case ZG_OP_FP12_FROB2: zg::fp12_frobenius(r, a, 2); break;
            case ZG_OP_FP12_FROB3: zg::fp12_frobenius(r, a, 3); break;
            case ZG_OP_FP12_EXP_X: zg::fp12_exp_by_x(r, a); break;
            case 101: zg::pair_final_exp(r, a); break;
            case 102:
                zg::fp12_mul_by_034(a, b.c0.c0, b.c0.c1, b.c0.c2);
                r = a;
                break;
            default: fprintf(stderr, "pairing_host: unknown op %d\n", op); return 2;
            }
        }
        zg::fp12_store(reinterpret_cast<uint64_t *>(out.data() + i * OUT_WORDS / 4), r);
    }
    return fwrite(out.data(), sizeof(uint4), out.size(), stdout) == out.size() ? 0 : 1;
}
