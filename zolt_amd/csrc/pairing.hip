// pairing.hip — the optimal ate pairing of BN254 for the Dory prover's multi-pairings (src/poly/commitment/dory.zig:673-690: multiPairG1G2,
// six times a reduce-and-fold round, once per commit) as three launches:
//   pair_set_miller_kernel<PlainPairs>  pair_set.hip.h's, a lane per (P, Q) pair of two plain arrays: the value of millerLoopArkworks
//                                       (src/field/pairing.zig:1561-1628); pair_set_millerw_kernel<PlainPairs>, a wavefront per pair,
//                                       under the wave engine
//   pair_product_kernel                 a workgroup per multi-pairing: the Fp12 product of its segment of Miller values
//   pair_final_exp_kernel               a lane per product: finalExponentiation (:1653-1681) with hardPartExponentiationArkworks (:1812-1880);
//                                       pairing_wave.hip's pairw_final_exp_kernel, a wavefront per product, under the wave engine
// The reference pays a final exponentiation per PAIR and multiplies the results; the final exponentiation is a homomorphism of Fp12*, and
// field values are canonical, so one exponentiation of the product of the Miller values has the same bits. What a lane computes is
// pairing.hip.h over the tower of fp12.hip.h: out-of-line products on canonical Montgomery values, latency-bound like the G2 section
// (docs/design/05_msm.md, "Pairings"). Both engines use the same layouts and give the same bits, so pair_product_kernel serves both.
// The product and the final-exponentiation launch of every pair set in the library are the two helpers below.
#include "common.hip.h"
#include "pair_set.hip.h"

namespace zg {

// two plain arrays, pair i = (g1_xy[i], g2_xy[i]); either flag array may be null
struct PlainPairs {
    const uint64_t *g1_xy;
    const uint8_t *g1_inf;
    const uint64_t *g2_xy;
    const uint8_t *g2_inf;
    ZG_DEV PairOperands operator()(uint32_t i) const {
        return {g1_xy + 8 * (size_t)i, g2_xy + 16 * (size_t)i, (g1_inf && g1_inf[i]) || (g2_inf && g2_inf[i])};
    }
};

// One workgroup of 64 lanes per segment [seg[j], seg[j + 1]) of Miller values (both ends clamped to n; an empty or inverted range gives
// one): lane t multiplies the entries t, t + 64, ... of its segment, then a tree over the 64 partial products through LDS. The value does
// not depend on the grouping — Fp12 is commutative and results are canonical — and no length is assumed.
__global__ void __launch_bounds__(64) pair_product_kernel(const uint64_t *vals, size_t n, const size_t *seg, uint64_t *out /* gridDim.x * 48 */) {
    __shared__ uint32_t lds[Fp12::WORDS32 * 64];  // word-major: lds[w * 64 + t], no bank conflicts
    const uint32_t t = threadIdx.x;
    size_t lo = seg[blockIdx.x], hi = seg[blockIdx.x + 1];
    if (hi > n) hi = n;
    if (lo > hi) lo = hi;
    Fp12 acc = fp12_one();
#pragma unroll 1
    for (size_t i = lo + t; i < hi; i += 64) {
        const Fp12 v = fp12_load(vals + 48 * i);
        fp12_mul(acc, acc, v);
    }
    uint32_t *aw = reinterpret_cast<uint32_t *>(&acc);
#pragma unroll 1
    for (uint32_t s = 32; s >= 1; s >>= 1) {
        if (t >= s && t < 2 * s)
            for (int w = 0; w < Fp12::WORDS32; w++) lds[w * 64 + t] = aw[w];
        __syncthreads();
        if (t < s) {
            Fp12 other;
            uint32_t *ow = reinterpret_cast<uint32_t *>(&other);
            for (int w = 0; w < Fp12::WORDS32; w++) ow[w] = lds[w * 64 + t + s];
            fp12_mul(acc, acc, other);
        }
        __syncthreads();
    }
    if (t == 0) fp12_store(out + 48 * (size_t)blockIdx.x, acc);
}

__global__ void __launch_bounds__(64) pair_final_exp_kernel(const uint64_t *in, size_t n, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp12 f = fp12_load(in + 48 * i);
    Fp12 r;
    pair_final_exp(r, f);
    fp12_store(out + 48 * i, r);
}

// the self-test hooks ZG_OP_FP12_* of zg_field_op: one lane per element of 12 Fp
__global__ void __launch_bounds__(64) fp12_op_kernel(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp12 x = fp12_load(a + 48 * i);
    Fp12 r;
    switch (op) {
    case ZG_OP_FP12_MUL: {
        const Fp12 y = fp12_load(b + 48 * i);
        fp12_mul(r, x, y);
        break;
    }
    case ZG_OP_FP12_SQR: fp12_sqr(r, x); break;
    case ZG_OP_FP12_INV: fp12_inv(r, x); break;
    case ZG_OP_FP12_CONJ: r = fp12_conj(x); break;
    case ZG_OP_FP12_FROB1: fp12_frobenius(r, x, 1); break;
    case ZG_OP_FP12_FROB2: fp12_frobenius(r, x, 2); break;
    case ZG_OP_FP12_FROB3: fp12_frobenius(r, x, 3); break;
    default: fp12_exp_by_x(r, x); break;  // ZG_OP_FP12_EXP_X
    }
    fp12_store(out + 48 * i, r);
}

// runtime.hip's zg_field_op forwards the ZG_OP_FP12_* codes here: n_elems Fp12 elements at device pointers, one launch on st
int fp12_selftest_enqueue(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n_elems, hipStream_t st) {
    hipLaunchKernelGGL(fp12_op_kernel, dim3(div_up(n_elems, 64)), dim3(64), 0, st, op, d_a, d_b, d_out, n_elems);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

static constexpr size_t PAIR_MAX_N = (size_t)1 << 24;  // a round has 2^10 pairs; longer vectors are correct, not tuned

static const char *const PAIR_ARGS = "invalid argument (at most 2^24 pairs or products)";

// The product launch and the final-exponentiation launch of every pair set (common.hip.h). `engine` is what the entry point read from
// pairing_engine() when it was called: LANE exponentiates with the kernel above, WAVE with pairing_wave.hip's.
void pair_product_enqueue(const uint64_t *d_miller, size_t n, const size_t *d_seg, size_t k, hipStream_t st, uint64_t *d_prod) {
    hipLaunchKernelGGL(pair_product_kernel, dim3((unsigned)k), dim3(64), 0, st, d_miller, n, d_seg, d_prod);
}
void pair_final_exp_enqueue(const uint64_t *d_in, size_t n, hipStream_t st, uint64_t *d_out, int engine) {
    if (engine == ZG_PAIRING_ENGINE_WAVE) return pairw_final_exp_enqueue(d_in, n, st, d_out);
    if (n) hipLaunchKernelGGL(pair_final_exp_kernel, dim3(div_up(n, 64)), dim3(64), 0, st, d_in, n, d_out);
}
void pair_product_final_enqueue(const uint64_t *d_miller, size_t n, const size_t *d_seg, size_t k, hipStream_t st, uint64_t *d_prod, uint64_t *d_out, int engine) {
    pair_product_enqueue(d_miller, n, d_seg, k, st, d_prod);
    pair_final_exp_enqueue(d_prod, k, st, d_out, engine);
}

// k > 0; d_miller holds n values (n may be 0: every product is then one), d_prod k products of scratch
static void multi_pairing_enqueue(const PlainPairs &pairs, size_t n, const size_t *d_seg, size_t k, hipStream_t st, uint64_t *d_miller, uint64_t *d_prod,
                                  uint64_t *d_out, int engine) {
    pair_set_miller_enqueue(pairs, n, st, d_miller, engine);
    pair_product_final_enqueue(d_miller, n, d_seg, k, st, d_prod, d_out, engine);
}

// the two per-pair batches: Miller values only, or Miller values and their final exponentiations
static int pair_batch(const char *who, bool final_exp, const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n,
                      uint64_t *out_gt) {
    const int engine = pairing_engine();
    ZG_INIT();
    if (n > PAIR_MAX_N || (n && (!g1_xy || !g2_xy || !out_gt))) return invalid(who, PAIR_ARGS);
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const uint64_t *d_g1 = sg.in(g1_xy, n * 64), *d_g2 = sg.in(g2_xy, n * 128);
    const uint8_t *d_g1i = sg.in(g1_inf, n), *d_g2i = sg.in(g2_inf, n);
    uint64_t *d_m = sg.out<uint64_t>(n * Fp12::BYTES), *d_out = final_exp ? sg.out<uint64_t>(n * Fp12::BYTES) : d_m;
    if (sg.ok()) {
        pair_set_miller_enqueue(PlainPairs{d_g1, d_g1i, d_g2, d_g2i}, n, sg.st, d_m, engine);
        if (final_exp) pair_final_exp_enqueue(d_m, n, sg.st, d_out, engine);
        sg.launched();
    }
    sg.fetch(out_gt, d_out, n * Fp12::BYTES);
    return sg.finish();
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_miller_loop_batch(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n, uint64_t *out_gt) {
    return pair_batch("zg_miller_loop_batch", false, g1_xy, g1_inf, g2_xy, g2_inf, n, out_gt);
}

int zg_pairing_batch(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n, uint64_t *out_gt) {
    return pair_batch("zg_pairing_batch", true, g1_xy, g1_inf, g2_xy, g2_inf, n, out_gt);
}

int zg_final_exponentiation_batch(const uint64_t *in_gt, size_t n, uint64_t *out_gt) {
    const int engine = pairing_engine();
    ZG_INIT();
    if (n > PAIR_MAX_N || (n && (!in_gt || !out_gt))) return invalid("zg_final_exponentiation_batch", PAIR_ARGS);
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const uint64_t *d_in = sg.in(in_gt, n * Fp12::BYTES);
    uint64_t *d_out = sg.out<uint64_t>(n * Fp12::BYTES);
    if (sg.ok()) {
        pair_final_exp_enqueue(d_in, n, sg.st, d_out, engine);
        sg.launched();
    }
    sg.fetch(out_gt, d_out, n * Fp12::BYTES);
    return sg.finish();
}

int zg_multi_pairing(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n, const size_t *seg, size_t k,
                     uint64_t *out_gt) {
    const int engine = pairing_engine();
    ZG_INIT();
    if (n > PAIR_MAX_N || k > PAIR_MAX_N || (n && (!g1_xy || !g2_xy)) || (k && (!seg || !out_gt))) return invalid("zg_multi_pairing", PAIR_ARGS);
    for (size_t j = 0; j < k; j++)
        if (seg[j] > seg[j + 1] || seg[j + 1] > n) return invalid("zg_multi_pairing", PAIR_ARGS);
    if (k == 0) return ZG_OK;
    Staging sg(lib_stream());
    const uint64_t *d_g1 = sg.in(g1_xy, n * 64), *d_g2 = sg.in(g2_xy, n * 128);
    const uint8_t *d_g1i = sg.in(g1_inf, n), *d_g2i = sg.in(g2_inf, n);
    const size_t *d_seg = sg.in(seg, (k + 1) * sizeof(size_t));
    uint64_t *d_m = sg.out<uint64_t>((n ? n : 1) * Fp12::BYTES), *d_prod = sg.out<uint64_t>(k * Fp12::BYTES), *d_out = sg.out<uint64_t>(k * Fp12::BYTES);
    if (sg.ok()) {
        multi_pairing_enqueue(PlainPairs{d_g1, d_g1i, d_g2, d_g2i}, n, d_seg, k, sg.st, d_m, d_prod, d_out, engine);
        sg.launched();
    }
    sg.fetch(out_gt, d_out, k * Fp12::BYTES);
    return sg.finish();
}

int zg_multi_pairing_dev(const uint64_t *d_g1_xy, const uint8_t *d_g1_inf, const uint64_t *d_g2_xy, const uint8_t *d_g2_inf, size_t n, const size_t *d_seg, size_t k,
                         void *stream, uint64_t *d_out_gt) {
    const int engine = pairing_engine();
    ZG_INIT();
    if (n > PAIR_MAX_N || k > PAIR_MAX_N || (n && (!d_g1_xy || !d_g2_xy)) || (k && (!d_seg || !d_out_gt))) return invalid("zg_multi_pairing_dev", PAIR_ARGS);
    if (k == 0) return ZG_OK;
    Staging sg(pick_stream(stream));  // the scratch goes back to the pool on return: the launch set has to be complete by then
    uint64_t *d_m = sg.out<uint64_t>((n ? n : 1) * Fp12::BYTES), *d_prod = sg.out<uint64_t>(k * Fp12::BYTES);
    if (sg.ok()) {
        multi_pairing_enqueue(PlainPairs{d_g1_xy, d_g1_inf, d_g2_xy, d_g2_inf}, n, d_seg, k, sg.st, d_m, d_prod, d_out_gt, engine);
        sg.launched();
    }
    return sg.finish();
}

}  // extern "C"
