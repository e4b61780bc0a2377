// field_vec.hip — the section "field vectors (device)" of zolt_gpu.h: field.BatchOps (src/field/mod.zig:1164-1280) on device pointers.
// Element-wise ops and the scale, the batch inverse by Montgomery's trick (field_vec.hip.h), the inner product and Horner's rule as one
// grid-stride pass that leaves a partial per workgroup and a one-workgroup finish. Fr sums are lazy (Acc9, block_sum_pair9,
// sc_finish_kernel); Fp sums are canonical Fe<FpParams> values added with fe_add. Every output is a canonical field element, so its
// bits do not depend on the grouping. Scratch comes from Staging; ZG_FV_BLOCKS caps every grid of this unit.
#include "common.hip.h"
#include "sc_common.hip.h"
#include "field_vec.hip.h"

namespace zg {

constexpr unsigned FV_MAX_BLOCKS = 4096;
constexpr size_t FV_MAX_N = (size_t)1 << 36;              // elements a call accepts (2 TiB a vector)
constexpr size_t FV_LAZY_TERMS = (size_t)1 << 29;          // terms a workgroup adds up lazily at most (Acc9's bound is 2^30)
constexpr size_t FV_RESULT_OFF = 4 * (size_t)FV_MAX_BLOCKS;  // scratch of a reduction (u64 words): block partials | the result | the ladder
constexpr size_t FV_LADDER_OFF = FV_RESULT_OFF + 4;
constexpr size_t FV_SCRATCH_BYTES = (FV_LADDER_OFF + 4 * (size_t)FV_LADDER) * 8;

static unsigned fv_block_cap() { return env_uint("ZG_FV_BLOCKS", 2048, 1, FV_MAX_BLOCKS); }
// workgroups for `items` units of work at `per_block` a trip; a reducing grid never gives a workgroup more than FV_LAZY_TERMS terms
static unsigned fv_blocks(size_t items, size_t per_block) {
    const unsigned cap = fv_block_cap(), need = div_up(items, per_block), least = div_up(items, FV_LAZY_TERMS);
    const unsigned nb = need < cap ? need : cap;
    return nb < least ? least : nb;
}

// ---- element-wise
template <class P>
__global__ void __launch_bounds__(256) fv_op_kernel(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const Fe<P> x = fe_load<P>(a + 4 * i);
        Fe<P> y = Fe<P>::zero(), r;
        if (op <= ZG_OP_SUB) y = fe_load<P>(b + 4 * i);
        switch (op) {
            case ZG_OP_MUL: r = fe_mul(x, y); break;
            case ZG_OP_ADD: r = fe_add(x, y); break;
            case ZG_OP_SUB: r = fe_sub(x, y); break;
            case ZG_OP_NEG: r = fe_neg(x); break;
            case ZG_OP_SQR: r = fe_sqr(x); break;
            case ZG_OP_INV: r = fe_inv(x); break;
            case ZG_OP_FROM_MONT: r = fe_from_mont(x); break;
            default: r = fe_to_mont(x); break;
        }
        fe_store(out + 4 * i, r);
    }
}
template <class P>
__global__ void __launch_bounds__(256) fv_scale_kernel(const uint64_t *a, size_t n, FeArg s_a, uint64_t *out) {
    const Fe<P> s = fe_from_arg<P>(s_a);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) fe_store(out + 4 * i, fe_mul(fe_load<P>(a + 4 * i), s));
}

// ---- sums. FvSum<P>: what a thread adds its terms to, and how the workgroup's total reaches partials[blockIdx] (one barrier)
template <class P>
struct FvSum;
template <>
struct FvSum<FrParams> {  // lazy: nine add-with-carry per term, one reduction per workgroup
    Acc9 acc = acc9_zero();
    ZG_DEV void add(const Fr &v) { acc9_add(acc, v); }
    ZG_DEV void store(u32 *sh, uint64_t *partials) {
        const Fr tot = block_sum_pair9(acc, acc9_zero(), sh);
        if (threadIdx.x == SC_LANE_G0) fe_store(partials + 4 * (size_t)blockIdx.x, tot);
    }
};
template <>
struct FvSum<FpParams> {  // canonical: fe_add per term, a shuffle tree per wave, the waves' totals through LDS
    Fp acc = Fp::zero();
    ZG_DEV void add(const Fp &v) { acc = fe_add(acc, v); }
    ZG_DEV void store(u32 *sh, uint64_t *partials) {
        const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            Fp o;
#pragma unroll
            for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc.l[i], d, 64);
            acc = fe_add(acc, o);
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) sh[wave * 8 + i] = acc.l[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (u32 w = 1; w < nwaves; w++) {
                Fp o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = sh[w * 8 + i];
                acc = fe_add(acc, o);
            }
            fe_store(partials + 4 * (size_t)blockIdx.x, acc);
        }
    }
};
ZG_DEV Fr fv_mul(const Fr &a, const Fr &b) { return fr_mul29v(a, b); }
ZG_DEV Fp fv_mul(const Fp &a, const Fp &b) { return fe_mul(a, b); }

template <class P>
__global__ void __launch_bounds__(256) fv_dot_kernel(const uint64_t *a, const uint64_t *b, size_t n, uint64_t *partials) {
    __shared__ u32 sh[SC_RED_WORDS];
    FvSum<P> sum;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) sum.add(fv_mul(fe_load<P>(a + 4 * i), fe_load<P>(b + 4 * i)));
    sum.store(sh, partials);
}

// Horner's rule: a lane evaluates chunk j = coefficients [E j, E j + E) at x (coefficients past n are zero) and weighs the value by
// x^(E j), chosen from the ladder the prologue left; then the sum as above
template <class P>
__global__ void __launch_bounds__(64) fv_ladder_kernel(FeArg x_a, uint64_t *ladder, int nbits) {
    if (threadIdx.x == 0) fv_ladder_fill<P, FV_E>(fe_from_arg<P>(x_a), reinterpret_cast<Fe<P> *>(ladder), nbits);
}
template <class P>
__global__ void __launch_bounds__(256) fv_horner_kernel(const uint64_t *c, size_t n, size_t chunks, FeArg x_a, const uint64_t *ladder, int nbits,
                                                        uint64_t *partials) {
    __shared__ u32 sh[SC_RED_WORDS];
    const Fe<P> x = fe_from_arg<P>(x_a);
    const Fe<P> *lad = reinterpret_cast<const Fe<P> *>(ladder);
    FvSum<P> sum;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < chunks; j += stride) {
        Fe<P> v[FV_E];
#pragma unroll
        for (int k = 0; k < FV_E; k++) {
            const size_t i = j * FV_E + k;
            v[k] = i < n ? fe_load<P>(c + 4 * i) : Fe<P>::zero();
        }
        sum.add(fe_mul(fv_horner_chunk<P, FV_E>(v, x), fv_chunk_weight<P>(lad, j, nbits)));
    }
    sum.store(sh, partials);
}
// the partials of a canonical sum (Fp) into out: one workgroup
template <class P>
__global__ void __launch_bounds__(256) fv_finish_kernel(const uint64_t *partials, uint32_t nblocks, uint64_t *out) {
    __shared__ u32 sh[SC_RED_WORDS];
    FvSum<P> sum;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256) sum.add(fe_load<P>(partials + 4 * (size_t)b));
    sum.store(sh, out);  // blockIdx.x == 0
}
static void fv_finish_enqueue(FrParams, hipStream_t st, const uint64_t *d_part, unsigned nb, uint64_t *d_out) {
    hipLaunchKernelGGL(sc_finish_kernel<>, dim3(1), dim3(256), 0, st, d_part, nb, 1u, d_out, (uint64_t *)nullptr, (uint64_t)0);
}
static void fv_finish_enqueue(FpParams, hipStream_t st, const uint64_t *d_part, unsigned nb, uint64_t *d_out) {
    hipLaunchKernelGGL(fv_finish_kernel<FpParams>, dim3(1), dim3(256), 0, st, d_part, nb, d_out);
}

// The launch sets on sg.st over device pointers, n > 0. The reductions return where the result will be: four words of sg's scratch
// (nullptr when there was none; sg then says why).
template <class P>
static uint64_t *fv_dot_enqueue(Staging &sg, const uint64_t *d_a, const uint64_t *d_b, size_t n) {
    uint64_t *d_scr = sg.out<uint64_t>(FV_SCRATCH_BYTES);
    if (!d_scr) return nullptr;
    const unsigned nb = fv_blocks(n, 256);
    hipLaunchKernelGGL(fv_dot_kernel<P>, dim3(nb), dim3(256), 0, sg.st, d_a, d_b, n, d_scr);
    fv_finish_enqueue(P(), sg.st, d_scr, nb, d_scr + FV_RESULT_OFF);
    sg.launched();
    return d_scr + FV_RESULT_OFF;
}
template <class P>
static uint64_t *fv_horner_enqueue(Staging &sg, const uint64_t *d_c, size_t n, const uint64_t x[4]) {
    uint64_t *d_scr = sg.out<uint64_t>(FV_SCRATCH_BYTES);
    if (!d_scr) return nullptr;
    const size_t chunks = (n + FV_E - 1) / FV_E;
    const unsigned nb = fv_blocks(chunks, 256);
    const int nbits = fv_index_bits(chunks);
    hipLaunchKernelGGL(fv_ladder_kernel<P>, dim3(1), dim3(64), 0, sg.st, fe_arg(x), d_scr + FV_LADDER_OFF, nbits);
    hipLaunchKernelGGL(fv_horner_kernel<P>, dim3(nb), dim3(256), 0, sg.st, d_c, n, chunks, fe_arg(x), d_scr + FV_LADDER_OFF, nbits, d_scr);
    fv_finish_enqueue(P(), sg.st, d_scr, nb, d_scr + FV_RESULT_OFF);
    sg.launched();
    return d_scr + FV_RESULT_OFF;
}
template <class P>
static void fv_batch_inv_enqueue(const uint64_t *d_a, uint64_t *d_out, size_t n, hipStream_t st) {
    hipLaunchKernelGGL((fv_batch_inv_kernel<P, FV_E>), dim3(fv_blocks(n, FV_TILE)), dim3(FV_THREADS), 0, st, d_a, d_out, n);
}

static bool fv_field_ok(int field) { return field == ZG_FIELD_FR || field == ZG_FIELD_FP; }
// the overlap rule: out == in is in place; any other meeting of out[0, n) and in[0, n) is refused
static bool fv_overlap(const uint64_t *out, const uint64_t *in, size_t n) {
    if (!in || !out || in == out) return false;
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in, bytes = (uintptr_t)n * 32;
    return o < i + bytes && i < o + bytes;
}
// the scalar of a reduction: fetched from sg's scratch, handed out when all went well (zero for an empty vector)
static int fv_scalar_out(Staging &sg, const uint64_t *d_res, uint64_t out[4]) {
    uint64_t h[4] = {0, 0, 0, 0};
    if (d_res) sg.fetch(h, d_res, 32);
    if (sg.finish() != ZG_OK) return sg.rc;
    for (int l = 0; l < 4; l++) out[l] = h[l];
    return ZG_OK;
}
static int fv_zero_out(uint64_t out[4]) {
    for (int l = 0; l < 4; l++) out[l] = 0;
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_field_op_dev(int field, int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n, void *stream) {
    ZG_INIT();
    if (!fv_field_ok(field) || op < ZG_OP_MUL || op > ZG_OP_TO_MONT) return invalid("zg_field_op_dev: unknown field, or an op outside ZG_OP_MUL .. ZG_OP_TO_MONT");
    if (n == 0) return ZG_OK;
    const bool two = op <= ZG_OP_SUB;
    if (!d_a || !d_out || (two && !d_b) || n > FV_MAX_N) return invalid("zg_field_op_dev: null data with n > 0");
    if (fv_overlap(d_out, d_a, n) || (two && d_b != d_a && (d_out == d_b || fv_overlap(d_out, d_b, n))))
        return invalid("zg_field_op_dev: the output overlaps an input (only out == a is in place)");
    hipStream_t st = pick_stream(stream);
    const unsigned nb = fv_blocks(n, 256);
    if (field == ZG_FIELD_FR) hipLaunchKernelGGL(fv_op_kernel<FrParams>, dim3(nb), dim3(256), 0, st, op, d_a, two ? d_b : nullptr, d_out, n);
    else hipLaunchKernelGGL(fv_op_kernel<FpParams>, dim3(nb), dim3(256), 0, st, op, d_a, two ? d_b : nullptr, d_out, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int zg_field_scale_dev(int field, const uint64_t *d_a, size_t n, const uint64_t s_host[4], uint64_t *d_out, void *stream) {
    ZG_INIT();
    if (!fv_field_ok(field)) return invalid("zg_field_scale_dev: unknown field");
    if (n == 0) return ZG_OK;
    if (!d_a || !d_out || !s_host || n > FV_MAX_N) return invalid("zg_field_scale_dev: null data with n > 0");
    if (fv_overlap(d_out, d_a, n)) return invalid("zg_field_scale_dev: the output overlaps the input (only out == a is in place)");
    hipStream_t st = pick_stream(stream);
    const unsigned nb = fv_blocks(n, 256);
    if (field == ZG_FIELD_FR) hipLaunchKernelGGL(fv_scale_kernel<FrParams>, dim3(nb), dim3(256), 0, st, d_a, n, fe_arg(s_host), d_out);
    else hipLaunchKernelGGL(fv_scale_kernel<FpParams>, dim3(nb), dim3(256), 0, st, d_a, n, fe_arg(s_host), d_out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int zg_field_batch_inverse_dev(int field, const uint64_t *d_a, uint64_t *d_out, size_t n, void *stream) {
    ZG_INIT();
    if (!fv_field_ok(field)) return invalid("zg_field_batch_inverse_dev: unknown field");
    if (n == 0) return ZG_OK;
    if (!d_a || !d_out || n > FV_MAX_N) return invalid("zg_field_batch_inverse_dev: null data with n > 0");
    if (fv_overlap(d_out, d_a, n)) return invalid("zg_field_batch_inverse_dev: the output overlaps the input (only out == a is in place)");
    hipStream_t st = pick_stream(stream);
    if (field == ZG_FIELD_FR) fv_batch_inv_enqueue<FrParams>(d_a, d_out, n, st);
    else fv_batch_inv_enqueue<FpParams>(d_a, d_out, n, st);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int zg_field_batch_inverse(int field, const uint64_t *a, uint64_t *out, size_t n) {
    ZG_INIT();
    if (!fv_field_ok(field)) return invalid("zg_field_batch_inverse: unknown field");
    if (n == 0) return ZG_OK;
    if (!a || !out || n > FV_MAX_N) return invalid("zg_field_batch_inverse: null data with n > 0");
    if (fv_overlap(out, a, n)) return invalid("zg_field_batch_inverse: the output overlaps the input (only out == a is in place)");
    Staging sg(lib_stream());
    uint64_t *d = sg.in(a, n * 32);  // inverted in place: a lane writes only what it read
    if (sg.ok()) {
        if (field == ZG_FIELD_FR) fv_batch_inv_enqueue<FrParams>(d, d, n, sg.st);
        else fv_batch_inv_enqueue<FpParams>(d, d, n, sg.st);
        sg.launched();
    }
    sg.fetch(out, d, n * 32);
    return sg.finish();
}

int zg_field_inner_product_dev(int field, const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream, uint64_t out_host[4]) {
    ZG_INIT();
    if (!fv_field_ok(field) || !out_host) return invalid("zg_field_inner_product_dev: unknown field, or no output");
    if (n == 0) return fv_zero_out(out_host);
    if (!d_a || !d_b || n > FV_MAX_N) return invalid("zg_field_inner_product_dev: null data with n > 0");
    Staging sg(pick_stream(stream));
    const uint64_t *d_res = field == ZG_FIELD_FR ? fv_dot_enqueue<FrParams>(sg, d_a, d_b, n) : fv_dot_enqueue<FpParams>(sg, d_a, d_b, n);
    return fv_scalar_out(sg, d_res, out_host);
}

int zg_field_inner_product(int field, const uint64_t *a, const uint64_t *b, size_t n, uint64_t out[4]) {
    ZG_INIT();
    if (!fv_field_ok(field) || !out) return invalid("zg_field_inner_product: unknown field, or no output");
    if (n == 0) return fv_zero_out(out);
    if (!a || !b || n > FV_MAX_N) return invalid("zg_field_inner_product: null data with n > 0");
    Staging sg(lib_stream());
    const uint64_t *d_a = sg.in(a, n * 32), *d_b = b == a ? d_a : sg.in(b, n * 32), *d_res = nullptr;
    if (sg.ok()) d_res = field == ZG_FIELD_FR ? fv_dot_enqueue<FrParams>(sg, d_a, d_b, n) : fv_dot_enqueue<FpParams>(sg, d_a, d_b, n);
    return fv_scalar_out(sg, d_res, out);
}

int zg_field_horner_dev(int field, const uint64_t *d_coeffs, size_t n, const uint64_t x_host[4], void *stream, uint64_t out_host[4]) {
    ZG_INIT();
    if (!fv_field_ok(field) || !out_host) return invalid("zg_field_horner_dev: unknown field, or no output");
    if (n == 0) return fv_zero_out(out_host);
    if (!d_coeffs || !x_host || n > FV_MAX_N) return invalid("zg_field_horner_dev: null data with n > 0");
    Staging sg(pick_stream(stream));
    const uint64_t *d_res = field == ZG_FIELD_FR ? fv_horner_enqueue<FrParams>(sg, d_coeffs, n, x_host) : fv_horner_enqueue<FpParams>(sg, d_coeffs, n, x_host);
    return fv_scalar_out(sg, d_res, out_host);
}

int zg_field_horner(int field, const uint64_t *coeffs, size_t n, const uint64_t x[4], uint64_t out[4]) {
    ZG_INIT();
    if (!fv_field_ok(field) || !out) return invalid("zg_field_horner: unknown field, or no output");
    if (n == 0) return fv_zero_out(out);
    if (!coeffs || !x || n > FV_MAX_N) return invalid("zg_field_horner: null data with n > 0");
    Staging sg(lib_stream());
    const uint64_t *d_c = sg.in(coeffs, n * 32), *d_res = nullptr;
    if (sg.ok()) d_res = field == ZG_FIELD_FR ? fv_horner_enqueue<FrParams>(sg, d_c, n, x) : fv_horner_enqueue<FpParams>(sg, d_c, n, x);
    return fv_scalar_out(sg, d_res, out);
}

int zg_fr_dense_evaluate_dev(const uint64_t *d_evals, size_t num_vars, const uint64_t *point_host, void *stream, uint64_t out_host[4]) {
    ZG_INIT();
    if (!d_evals || !out_host || (num_vars && !point_host) || num_vars > 30) return invalid("zg_fr_dense_evaluate_dev: invalid argument");
    const size_t n = (size_t)1 << num_vars;
    // the eq table's index MSB pairs with r[0]; evaluate() pairs index bit j with point[j]: reverse the point (as zg_fr_dense_evaluate)
    std::vector<uint64_t> rev(4 * (num_vars ? num_vars : 1));
    for (size_t j = 0; j < num_vars; j++)
        for (int l = 0; l < 4; l++) rev[4 * j + l] = point_host[4 * (num_vars - 1 - j) + l];
    Staging sg(pick_stream(stream));
    uint64_t *d_eq = sg.out<uint64_t>(n * 32);
    const uint64_t *d_res = nullptr;
    if (sg.ok() && sg.adopt(eq_table_enqueue(rev.data(), num_vars, nullptr, d_eq, sg.st))) d_res = fv_dot_enqueue<FrParams>(sg, d_evals, d_eq, n);
    return fv_scalar_out(sg, d_res, out_host);
}

}  // extern "C"
