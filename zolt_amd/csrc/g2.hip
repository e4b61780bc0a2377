// g2.hip — G2 fixed-base multiplication and msmG2 for Dory's reduce-and-fold rounds (src/poly/commitment/dory.zig:1545-1635).
//
// What the prover does with G2Point in every round is embarrassingly parallel group arithmetic on SHORT vectors (2^10 points in the
// shipped configuration, a few thousand at most): n scalar multiplications per message or update, each ~380 affine group operations
// with an Fp2 inversion apiece in the reference (G2Point.scalarMul, src/field/pairing.zig:880-919). Here every entry point is one
// launch set in projective coordinates with ONE inversion per output (the per-pair scalarMul, add and axpy batches are in points.hip):
//   fixed base                  a shared window table (as fb_mul_kernel does for G1): an output is W mixed additions, no doubling
//   msmG2                       8-bit windows, a workgroup per window and a lane per bucket; the digits are counting-sorted inside the
//                               workgroup (no atomics, no global sort), buckets are combined by per-bit tree sums (no 255-long running
//                               sum) and the 32 window sums by Horner — the one serial chain left (254 doublings)
// The work is latency-bound at these sizes (a few waves per SIMD at best): docs/design/05_msm.md, "G2", has the figures.
#include <string.h>

#include "common.hip.h"
#include "g2.hip.h"
#include "small_msm.hip.h"

namespace zg {

static __device__ __forceinline__ void g2_write(uint64_t *out_xy, uint8_t *out_inf, size_t i, const G2XYZZ &acc) {
    G2Affine r;
    bool isinf = xyzz_to_affine(acc, r);
    affine_store(out_xy + 16 * i, r);
    if (out_inf) out_inf[i] = isinf ? 1 : 0;
}

// ---- fixed base: g2_vec[i] = generator.scalarMul(hash_i) (dory.zig:963-966, 1695-1712), v2[i] = g2_vec[0].scalarMul(v_vec[i]) (:1513-1519).
// One shared table T[w][d - 1] = d * 2^(c w) * B, c = 4 (64 windows x 15 rows) for up to 256 outputs, c = 8 (32 x 255 rows, 1 MB) beyond:
// an output is at most W mixed additions and one conversion to affine.
static constexpr int G2_FB_W_MAX = 64;

// step 1 (one block, lane w): 2^(c w) * B by c * w doublings — the one serial chain of the build
__global__ void __launch_bounds__(G2_FB_W_MAX) g2_fb_window_bases_kernel(const uint64_t *base_xy, int c, int W, char *bw /* W * 256 */) {
    const int w = threadIdx.x;
    if (w >= W) return;
    G2XYZZ step = G2XYZZ::from_affine(affine_load<Fp2>(base_xy));
    for (int k = 0; k < c * w; k++) step = xyzz_dbl(step);
    xyzz_store(bw + 256 * (size_t)w, step);
}

// step 2 (one lane per row): d * B_w by double-and-add over the c bits of d, then to affine (128-byte rows and a flag byte each: a
// base of small order — not a member of G2, but a point the ABI cannot rule out — may reach the identity)
__global__ void __launch_bounds__(64) g2_fb_rows_kernel(const char *bw, uint32_t n_rows, int c, uint32_t rows_per_w, uint64_t *table, uint8_t *table_inf) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t w = i / rows_per_w, d = i % rows_per_w + 1;
    const G2XYZZ b = xyzz_load<Fp2>(bw + 256 * (size_t)w);
    G2XYZZ a = G2XYZZ::identity();
    for (int bit = c - 1; bit >= 0; bit--) {
        a = xyzz_dbl(a);
        if ((d >> bit) & 1u) a = xyzz_add(a, b);
    }
    g2_write(table, table_inf, i, a);
}

__global__ void __launch_bounds__(64) g2_fb_mul_kernel(const uint64_t *table, const uint8_t *table_inf, const uint64_t *scalars, size_t n, int c, int W,
                                                       uint32_t rows_per_w, uint64_t *out_xy, uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fe_from_mont(fe_load<FrParams>(scalars + 4 * i));
    G2XYZZ acc = G2XYZZ::identity();
    const uint32_t mask = (1u << c) - 1u;
#pragma unroll 1
    for (int w = 0; w < W; w++) {
        const uint32_t d = s.l[0] & mask;  // the next c bits; the scalar is shifted down behind it (static register indices)
#pragma unroll
        for (int k = 0; k < 8; k++) s.l[k] = (s.l[k] >> c) | (k < 7 ? s.l[k + 1] << (32 - c) : 0u);
        if (d == 0) continue;
        const size_t row = (size_t)w * rows_per_w + (d - 1);
        if (table_inf[row]) continue;
        acc = xyzz_madd(acc, affine_load<Fp2>(table + 16 * row));
    }
    g2_write(out_xy, out_inf, i, acc);
}

// the fixed-base launch set over device pointers: its table is scratch of sg, which synchronises before it releases
void g2_fixed_base_enqueue(Staging &sg, const uint64_t *d_base, const uint64_t *d_sc, size_t n, uint64_t *d_out, uint8_t *d_inf) {
    const int c = n <= 256 ? 4 : 8, W = (254 + c - 1) / c;
    const uint32_t rows_per_w = (1u << c) - 1u, n_rows = (uint32_t)W * rows_per_w;
    char *d_bw = sg.out<char>((size_t)W * 256);
    uint64_t *d_tab = sg.out<uint64_t>((size_t)n_rows * 128);
    uint8_t *d_tinf = sg.out<uint8_t>(n_rows);
    if (sg.ok()) {
        hipLaunchKernelGGL(g2_fb_window_bases_kernel, dim3(1), dim3(G2_FB_W_MAX), 0, sg.st, d_base, c, W, d_bw);
        hipLaunchKernelGGL(g2_fb_rows_kernel, dim3(div_up(n_rows, 64)), dim3(64), 0, sg.st, d_bw, n_rows, c, rows_per_w, d_tab, d_tinf);
        hipLaunchKernelGGL(g2_fb_mul_kernel, dim3(div_up(n, 64)), dim3(64), 0, sg.st, d_tab, d_tinf, d_sc, n, c, W, rows_per_w, d_out, d_inf);
        sg.launched();
    }
}

// ---- msmG2 (dory.zig:693-703: n scalarMuls and n adds in the reference) as a bucket MSM for short vectors: small_msm.hip.h over Fp2.
// Nothing is tabled or assumed resident — e2_plus / e2_minus run over v2_work, which changes every round.
__global__ void g2_identity_record_kernel(uint64_t *d_out17) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    affine_store(d_out17, G2Affine::identity());
    d_out17[16] = 1;
}

// enqueues the launch set on st; the scratch must outlive it (its Staging synchronises before it releases)
static void g2_msm_enqueue(const uint64_t *d_xy, const uint8_t *d_inf, const uint64_t *d_scalars, uint32_t n, hipStream_t st, const SmallMsmScratch &sc,
                           uint64_t *d_out17) {
    const SmallMsmJob job = {d_xy, d_inf, d_scalars, d_out17, n};
    small_msm_enqueue<Fp2>(&job, 1, st, sc);
}

static constexpr size_t G2_MSM_MAX_N = (size_t)1 << 24;  // the plan is sized for n <= 2^13; longer vectors are correct, not tuned

// G2Point.identity() on the host (pairing.zig:754-760)
static void g2_identity_host(uint64_t out_xy[16]) {
    static const uint64_t ONE[4] = {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full};
    memset(out_xy, 0, 128);
    memcpy(out_xy + 8, ONE, 32);
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_g2_fixed_base_mul_batch(const uint64_t base_xy[16], uint8_t base_inf, const uint64_t *scalars, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    ZG_INIT();
    if (!base_xy || (n && (!scalars || !out_xy || !out_inf))) {
        set_error("zg_g2_fixed_base_mul_batch: invalid argument");
        return ZG_ERR_INVALID;
    }
    if (n == 0) return ZG_OK;
    if (base_inf) {  // k * identity = identity (pairing.zig:881)
        for (size_t i = 0; i < n; i++) g2_identity_host(out_xy + 16 * i);
        memset(out_inf, 1, n);
        return ZG_OK;
    }
    Staging sg(lib_stream());
    const uint64_t *d_base = sg.in(base_xy, 128), *d_sc = sg.in(scalars, n * 32);
    uint64_t *d_out = sg.out<uint64_t>(n * 128);
    uint8_t *d_inf = sg.out<uint8_t>(n);
    g2_fixed_base_enqueue(sg, d_base, d_sc, n, d_out, d_inf);
    sg.fetch(out_xy, d_out, n * 128);
    sg.fetch(out_inf, d_inf, n);
    return sg.finish();
}

int zg_msm_g2_dev(const uint64_t *d_xy, const uint8_t *d_inf, const uint64_t *d_scalars, size_t n, void *stream, uint64_t *d_out17) {
    ZG_INIT();
    if (!d_out17 || n > G2_MSM_MAX_N || (n && (!d_xy || !d_scalars))) {
        set_error("zg_msm_g2_dev: invalid argument (at most 2^24 points)");
        return ZG_ERR_INVALID;
    }
    hipStream_t st = pick_stream(stream);
    if (n == 0) {
        hipLaunchKernelGGL(g2_identity_record_kernel, dim3(1), dim3(1), 0, st, d_out17);
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    Staging sg(st);  // the scratch goes back to the pool on return: the launch set has to be complete by then
    const SmallMsmScratch sc(sg, n, sizeof(G2XYZZ));
    if (sg.ok()) {
        g2_msm_enqueue(d_xy, d_inf, d_scalars, (uint32_t)n, st, sc, d_out17);
        sg.launched();
    }
    return sg.finish();
}

int zg_msm_g2(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars, size_t n, uint64_t out_xy[16], uint8_t *out_inf) {
    ZG_INIT();
    if (!out_xy || n > G2_MSM_MAX_N || (n && (!xy || !scalars))) {
        set_error("zg_msm_g2: invalid argument (at most 2^24 points)");
        return ZG_ERR_INVALID;
    }
    if (n == 0) {  // msmG2 of nothing: G2Point.identity() (dory.zig:695)
        g2_identity_host(out_xy);
        if (out_inf) *out_inf = 1;
        return ZG_OK;
    }
    Staging sg(lib_stream());
    const uint64_t *d_xy = sg.in(xy, n * 128), *d_sc = sg.in(scalars, n * 32);
    const uint8_t *d_inf = sg.in(inf, n);
    uint64_t *d_out = sg.out<uint64_t>(17 * 8);
    const SmallMsmScratch sc(sg, n, sizeof(G2XYZZ));
    if (sg.ok()) {
        g2_msm_enqueue(d_xy, d_inf, d_sc, (uint32_t)n, sg.st, sc, d_out);
        sg.launched();
    }
    uint64_t rec[17];
    sg.fetch(rec, d_out, sizeof rec);
    ZG_TRY(sg.finish());
    memcpy(out_xy, rec, 128);
    if (out_inf) *out_inf = (uint8_t)(rec[16] & 1);
    return ZG_OK;
}

}  // extern "C"
