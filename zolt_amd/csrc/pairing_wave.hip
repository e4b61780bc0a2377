// pairing_wave.hip — the second pairing engine (zolt_gpu.h, "Pairings (engine)"): a WAVEFRONT per Miller loop and per final
// exponentiation, where pairing.hip runs a lane. Its Miller kernel is pair_set.hip.h's pair_set_millerw_kernel, instantiated where a
// pair set is launched; here are
//   pairw_final_exp_kernel  a wave per product
//   fp12w_op_kernel         the ZG_OP_FP12W_* self-test hooks: a wave per element
// One wave per workgroup: the wave's element is blockIdx.x, a scalar, so every branch on it is uniform. What a wave computes is
// pairing_wave.hip.h over fp12_wave.hip.h; the values are canonical field elements, so both engines give the same bits.
// The engine setting lives here too: one atomic integer, no device behind it.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "common.hip.h"
#include "pairing_wave.hip.h"

namespace zg {

__global__ void __launch_bounds__(64) pairw_final_exp_kernel(const uint64_t *in, size_t n, uint64_t *out) {
    const size_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = fpw_lane();
    fpw_store(out + 48 * i, pairw_final_exp(fpw_load(in + 48 * i, lane)), lane);
}

__global__ void __launch_bounds__(64) fp12w_op_kernel(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    const size_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = fpw_lane();
    const Fp2 x = fpw_load(a + 48 * i, lane);
    Fp2 r;
    switch (op) {  // uniform: a launch argument
    case ZG_OP_FP12W_MUL: r = fpw_mul(x, fpw_load(b + 48 * i, lane)); break;
    case ZG_OP_FP12W_SQR: r = fpw_sqr(x); break;
    case ZG_OP_FP12W_INV: r = fpw_inv(x); break;
    case ZG_OP_FP12W_CONJ: r = fpw_conj(x, lane); break;
    case ZG_OP_FP12W_FROB1: r = fpw_frobenius(x, 1); break;
    case ZG_OP_FP12W_FROB2: r = fpw_frobenius(x, 2); break;
    case ZG_OP_FP12W_FROB3: r = fpw_frobenius(x, 3); break;
    case ZG_OP_FP12W_EXP_X: r = fpw_exp_by_x(x); break;
    default: {  // ZG_OP_FP12W_MUL_034: the first three Fp2 of b are c0, c3, c4
        const uint64_t *s = b + 48 * i;
        r = fpw_mul_by_034(x, Fp2::load(s), Fp2::load(s + 8), Fp2::load(s + 16), lane);
        break;
    }
    }
    fpw_store(out + 48 * i, r, lane);
}

int fp12w_selftest_enqueue(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n_elems, hipStream_t st) {
    hipLaunchKernelGGL(fp12w_op_kernel, dim3((unsigned)n_elems), dim3(64), 0, st, op, d_a, d_b, d_out, n_elems);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

void pairw_final_exp_enqueue(const uint64_t *d_in, size_t n, hipStream_t st, uint64_t *d_out) {
    if (n) hipLaunchKernelGGL(pairw_final_exp_kernel, dim3((unsigned)n), dim3(64), 0, st, d_in, n, d_out);
}

// LANE unless ZG_PAIRING_ENGINE=wave is in the environment when the setting is first read
static std::atomic<int> &engine_state() {
    static std::atomic<int> e{[] {
        const char *v = getenv("ZG_PAIRING_ENGINE");
        return v && !strcmp(v, "wave") ? ZG_PAIRING_ENGINE_WAVE : ZG_PAIRING_ENGINE_LANE;
    }()};
    return e;
}
int pairing_engine() { return engine_state().load(std::memory_order_relaxed); }

}  // namespace zg

extern "C" {

int zg_pairing_engine_set(int engine) {
    if (engine != ZG_PAIRING_ENGINE_LANE && engine != ZG_PAIRING_ENGINE_WAVE) return zg::invalid("zg_pairing_engine_set: unknown engine");
    zg::engine_state().store(engine, std::memory_order_relaxed);
    return ZG_OK;
}

int zg_pairing_engine_get(void) { return zg::pairing_engine(); }

}  // extern "C"
