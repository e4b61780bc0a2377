// selftest.hip — zg_selftest_lazy_g1 (include/zolt_gpu_internal.h): the MSM's lazy-limb arithmetic and group law on raw limbs, one
// record per lane (one per quad for the four-lane ops). The record format and the dispatch are lazy_selftest.hip.h, which the host harness
// of tests/test_lazy_group_law_host.py compiles too. This unit is built like msm.hip (no ZG_F29_SERIAL), so xyzz29_madd_nz runs the
// interleaved inline-assembly products here exactly as it does in the accumulate loop.
// zg_selftest_lazy_fr: the same for the sumcheck kernels' lazy Fr arithmetic and 288-bit sums (lazy_fr_selftest.hip.h, shared with the host
// harness of tests/test_lazy_fr_host.py), plus the block reduction of sc_common.hip.h on raw per-thread sums, which only a device can run.
// zg_selftest_xyzz: the canonical XYZZ group law of xyzz.hip.h over Fp and over Fp2 on raw coordinates (xyzz_selftest.hip.h, shared with the
// host harness of tests/test_xyzz_group_law_host.py). zg_selftest_small_msm: the launch set of small_msm.hip.h on its own, for either group
// and with jobs of different lengths — the header's own kernels, compiled into this unit as they are into g2.hip and dory.hip.
#include <string.h>

#include "common.hip.h"
#define ZG_LAZY_DEVICE_FORMS
#include "lazy_selftest.hip.h"
#include "lazy_fr_selftest.hip.h"
#include "sc_common.hip.h"
#include "small_msm.hip.h"
#include "xyzz_selftest.hip.h"

namespace zg {

__global__ void __launch_bounds__(64) lazy_g1_kernel(int op, const u32 *in, size_t n, u32 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lazy_record(op, in + ZG_LAZY_IN_WORDS * i, out + ZG_LAZY_OUT_WORDS * i);
}

// four adjacent lanes per record; a quad is either wholly inside n or wholly outside
__global__ void __launch_bounds__(64) lazy_g1_quad_kernel(int op, const u32 *in, size_t n, u32 *out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2;
    if (i >= n) return;
    u32 *o = out + ZG_LAZY_OUT_WORDS * i;
    const u32 bit = lazy_record4(op, in + ZG_LAZY_IN_WORDS * i, o, (u32)(t & 3));
    if (bit) atomicOr(&o[144], bit);  // the output buffer starts zeroed
}

__global__ void __launch_bounds__(64) lazy_fr_kernel(int op, const u32 *in, size_t n, u32 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lazy_fr_record(op, in + ZG_LAZY_FR_IN_WORDS * i, out + ZG_LAZY_FR_OUT_WORDS * i);
}

template <class F>
__global__ void __launch_bounds__(64) xyzz_selftest_kernel(int op, const u64 *in, size_t n, u64 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyzz_record<F>(op, in + XyzzRec<F>::IN_WORDS * i, out + XyzzRec<F>::OUT_WORDS * i);
}

// FR_BLOCKSUM: one workgroup per case. Thread t of case c reads its raw pair (g0, g1) — 2 x 9 words — at in[18 (c blockDim + t)];
// out[16 c .. 16 c + 7] = what block_sum_pair9 returns on lane SC_LANE_G0 of wave 0, out[16 c + 8 .. 16 c + 15] = on lane SC_LANE_G1.
__global__ void __launch_bounds__(1024) lazy_fr_blocksum_kernel(const u32 *in, u32 *out) {
    __shared__ u32 sh[SC_RED_WORDS];
    const u32 *rec = in + ZG_LAZY_FR_PAIR_WORDS * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
    Acc9 g0, g1;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        g0.l[i] = rec[i];
        g1.l[i] = rec[9 + i];
    }
    const Fr tot = block_sum_pair9(g0, g1, sh);
    if (threadIdx.x == SC_LANE_G0 || threadIdx.x == SC_LANE_G1) {
        u32 *dst = out + 16 * (size_t)blockIdx.x + (threadIdx.x == SC_LANE_G1 ? 8 : 0);
#pragma unroll
        for (int i = 0; i < 8; i++) dst[i] = tot.l[i];
    }
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_selftest_lazy_g1(int op, const uint32_t *in, size_t n, uint32_t *out) {
    ZG_INIT();
    if (op < 0 || op >= LAZY_NOPS || !in || !out || n == 0 || n > (1u << 20))
        return invalid("zg_selftest_lazy_g1: invalid argument (op 0..9, 1 <= n <= 2^20, non-null records)");
    const size_t in_bytes = n * ZG_LAZY_IN_WORDS * sizeof(u32), out_bytes = n * ZG_LAZY_OUT_WORDS * sizeof(u32);
    Staging sg(lib_stream());
    const u32 *din = sg.in(in, in_bytes);
    u32 *dout = sg.out<u32>(out_bytes);
    if (sg.ok() && ZG_STAGE(sg, hipMemsetAsync(dout, 0, out_bytes, sg.st))) {
        if (op >= LAZY_MADD4)
            hipLaunchKernelGGL(lazy_g1_quad_kernel, dim3(div_up(4 * n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        else
            hipLaunchKernelGGL(lazy_g1_kernel, dim3(div_up(n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        sg.launched();
    }
    sg.fetch(out, dout, out_bytes);
    return sg.finish();
}

int zg_selftest_lazy_fr(int op, const uint32_t *in, size_t n, uint32_t *out, int threads) {
    ZG_INIT();
    const bool block = op == FR_BLOCKSUM;
    if (op < 0 || op >= FR_NOPS || !in || !out || n == 0 || n > (1u << 12) ||
        (block ? (threads < 64 || threads > 1024 || threads % 64 != 0) : threads != 0))
        return invalid("zg_selftest_lazy_fr: invalid argument (op 0..8, 1 <= n <= 2^12, non-null records; threads a multiple of 64 up to 1024 for op 8, else 0)");
    const size_t in_bytes = (block ? n * (size_t)threads * ZG_LAZY_FR_PAIR_WORDS : n * ZG_LAZY_FR_IN_WORDS) * sizeof(u32);
    const size_t out_bytes = (block ? n * 16 : n * ZG_LAZY_FR_OUT_WORDS) * sizeof(u32);
    Staging sg(lib_stream());
    const u32 *din = sg.in(in, in_bytes);
    u32 *dout = sg.out<u32>(out_bytes);
    if (sg.ok() && ZG_STAGE(sg, hipMemsetAsync(dout, 0, out_bytes, sg.st))) {
        if (block)
            hipLaunchKernelGGL(lazy_fr_blocksum_kernel, dim3(n), dim3(threads), 0, sg.st, din, dout);
        else
            hipLaunchKernelGGL(lazy_fr_kernel, dim3(div_up(n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        sg.launched();
    }
    sg.fetch(out, dout, out_bytes);
    return sg.finish();
}

int zg_selftest_xyzz(int group, int op, const uint64_t *in, size_t n, uint64_t *out) {
    ZG_INIT();
    if (group < 0 || group > 1 || op < 0 || op >= XS_NOPS || !in || !out || n == 0 || n > (1u << 16))
        return invalid("zg_selftest_xyzz: invalid argument (group 0..1, op 0..8, 1 <= n <= 2^16, non-null records)");
    const size_t in_words = group ? XyzzRec<Fp2>::IN_WORDS : XyzzRec<Fp>::IN_WORDS, out_words = group ? XyzzRec<Fp2>::OUT_WORDS : XyzzRec<Fp>::OUT_WORDS;
    const size_t in_bytes = n * in_words * sizeof(u64), out_bytes = n * out_words * sizeof(u64);
    Staging sg(lib_stream());
    const u64 *din = sg.in(in, in_bytes);
    u64 *dout = sg.out<u64>(out_bytes);
    if (sg.ok() && ZG_STAGE(sg, hipMemsetAsync(dout, 0, out_bytes, sg.st))) {
        if (group) hipLaunchKernelGGL(xyzz_selftest_kernel<Fp2>, dim3(div_up(n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        else hipLaunchKernelGGL(xyzz_selftest_kernel<Fp>, dim3(div_up(n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        sg.launched();
    }
    sg.fetch(out, dout, out_bytes);
    return sg.finish();
}

int zg_selftest_small_msm(int group, int n_jobs, const size_t *n, const uint64_t *const *xy, const uint8_t *const *inf, const uint64_t *const *scalars,
                          uint64_t *out) {
    ZG_INIT();
    bool good = group >= 0 && group <= 1 && n_jobs >= 1 && n_jobs <= SMSM_MAX_JOBS && n && xy && scalars && out;
    size_t n_max = 0;
    for (int j = 0; good && j < n_jobs; j++) {
        good = n[j] <= (1u << 16) && (n[j] == 0 || (xy[j] && scalars[j]));
        if (n[j] > n_max) n_max = n[j];
    }
    if (!good)
        return invalid("zg_selftest_small_msm: invalid argument (group 0..1, 1..4 jobs of at most 2^16 points each, non-null arrays; inf and inf[j] may be null)");
    const size_t pt_bytes = group ? sizeof(G2Affine) : sizeof(Affine), rec_words = pt_bytes / 8 + 1;
    const size_t dev_rec_words = rec_words + 1;  // a record's coordinates are stored 16 bytes at a time: an even number of words apart
    Staging sg(lib_stream());
    SmallMsmJob job[SMSM_MAX_JOBS];
    uint64_t *d_out = sg.out<uint64_t>(SMSM_MAX_JOBS * dev_rec_words * 8);
    for (int j = 0; j < n_jobs; j++) {
        const uint64_t *d_xy = n[j] ? sg.in(xy[j], n[j] * pt_bytes) : nullptr, *d_sc = n[j] ? sg.in(scalars[j], n[j] * 32) : nullptr;
        const uint8_t *d_inf = n[j] && inf ? sg.in(inf[j], n[j]) : nullptr;
        job[j] = SmallMsmJob{d_xy, d_inf, d_sc, d_out + dev_rec_words * j, (uint32_t)n[j]};
    }
    const SmallMsmScratch sc(sg, n_max, group ? sizeof(G2XYZZ) : sizeof(XYZZ), n_jobs);
    if (sg.ok()) {
        if (group) small_msm_enqueue<Fp2>(job, n_jobs, sg.st, sc);
        else small_msm_enqueue<Fp>(job, n_jobs, sg.st, sc);
        sg.launched();
    }
    uint64_t rec[SMSM_MAX_JOBS * 18] = {};
    sg.fetch(rec, d_out, n_jobs * dev_rec_words * 8);
    ZG_TRY(sg.finish());
    for (int j = 0; j < n_jobs; j++) memcpy(out + rec_words * j, rec + dev_rec_words * j, rec_words * 8);
    return ZG_OK;
}

// host code only: every family is answered by the unit whose launches choose that shape (common.hip.h)
int zg_selftest_launch_shape(int family, size_t a, size_t b, uint32_t out[4]) {
    const size_t big = (size_t)1 << 40;
    const bool eq = family == ZG_SHAPE_EQ_TABLE || family == ZG_SHAPE_EQ_SPARTAN, flag = family <= ZG_SHAPE_SC_SUMS && family != ZG_SHAPE_EQ_SPARTAN;
    if (!out || family < ZG_SHAPE_EQ_TABLE || family > ZG_SHAPE_HK_FOLD || a > big || b > big || (eq && a > 34) ||
        (family == ZG_SHAPE_RRW ? b > 0xffffffffu : b > (flag ? 1u : 0u)))
        return invalid("zg_selftest_launch_shape: invalid argument (family 0..8, v <= 34, sizes up to 2^40, b as the family takes it)");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (family == ZG_SHAPE_FB) fb_launch_shape(a, out);
    else if (family == ZG_SHAPE_RRW) rrw_launch_shape(a, (uint32_t)b, out);
    else if (family == ZG_SHAPE_PSC) psc_launch_shape(a, out);
    else poly_launch_shape(family, a, b, out);
    return ZG_OK;
}

}  // extern "C"
