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

// ---- msmG2 (dory.zig:693-703: n scalarMuls and n adds in the reference) as a bucket MSM for short vectors. 8-bit unsigned windows,
// 32 of them; nothing is tabled or assumed resident — e2_plus / e2_minus run over v2_work, which changes every round.
static constexpr int G2_MSM_C = 8, G2_MSM_W = 32, G2_MSM_B = 1 << G2_MSM_C;

// digits, window-major: dig[w * n4 + i] = bits [8w, 8w + 8) of scalar i (0 for an identity base and in the padding up to n4 = 4 ceil(n/4))
__global__ void __launch_bounds__(256) g2_msm_digits_kernel(const uint64_t *scalars, const uint8_t *inf, uint32_t n, uint32_t n4, uint8_t *dig) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    Fr s = Fr::zero();
    if (i < n && !(inf && inf[i])) s = fe_from_mont(fe_load<FrParams>(scalars + 4 * (size_t)i));
#pragma unroll
    for (int w = 0; w < G2_MSM_W; w++) dig[(size_t)w * n4 + i] = (uint8_t)(s.l[w >> 2] >> (8 * (w & 3)));
}

// one workgroup per window, lane d = bucket d. The window's digits are counting-sorted by the workgroup itself — every lane walks the
// whole digit row (uniform loads, a compare per entry), counts its matches, takes its offset from a prefix sum over the 256 counts and
// walks the row again to list them — and then the lanes add their lists in lockstep: a mixed addition always runs with the whole wave.
__global__ void __launch_bounds__(G2_MSM_B) g2_msm_bucket_kernel(const uint8_t *dig, const uint64_t *xy, uint32_t n4, uint32_t *idx /* W * n4 */,
                                                                 char *buckets /* W * 256 * 256 */) {
    __shared__ uint32_t s_cnt[G2_MSM_B];
    const uint32_t w = blockIdx.x, d = threadIdx.x;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(dig + (size_t)w * n4);
    uint32_t *list = idx + (size_t)w * n4;
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < n4 / 4; j++) {
        const uint32_t v = row[j];
#pragma unroll
        for (int k = 0; k < 4; k++) cnt += ((v >> (8 * k)) & 0xffu) == d ? 1u : 0u;
    }
    if (d == 0) cnt = 0;  // digit 0 contributes nothing
    s_cnt[d] = cnt;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t k = 0; k < d; k++) off += s_cnt[k];
    if (cnt) {
        uint32_t pos = off;
        for (uint32_t j = 0; j < n4 / 4; j++) {
            const uint32_t v = row[j];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (((v >> (8 * k)) & 0xffu) == d) list[pos++] = 4 * j + k;
        }
    }
    G2XYZZ acc = G2XYZZ::identity();
    for (uint32_t k = 0; k < cnt; k++) acc = xyzz_madd(acc, affine_load<Fp2>(xy + 16 * (size_t)list[off + k]));
    xyzz_store(buckets + 256 * ((size_t)w * G2_MSM_B + d), acc);
}

// LDS image of one point per lane, 16-byte words of consecutive lanes side by side (no bank conflicts)
template <int LANES>
static __device__ __forceinline__ void fp_lds_store(uint4 *lds, int k, uint32_t t, const Fp &f) {
    lds[(2 * k) * LANES + t] = make_uint4(f.l[0], f.l[1], f.l[2], f.l[3]);
    lds[(2 * k + 1) * LANES + t] = make_uint4(f.l[4], f.l[5], f.l[6], f.l[7]);
}
template <int LANES>
static __device__ __forceinline__ Fp fp_lds_load(const uint4 *lds, int k, uint32_t t) {
    const uint4 a = lds[(2 * k) * LANES + t], b = lds[(2 * k + 1) * LANES + t];
    Fp f;
    f.l[0] = a.x; f.l[1] = a.y; f.l[2] = a.z; f.l[3] = a.w;
    f.l[4] = b.x; f.l[5] = b.y; f.l[6] = b.z; f.l[7] = b.w;
    return f;
}
template <int LANES>
static __device__ __forceinline__ void g2_lds_store(uint4 *lds, uint32_t t, const G2XYZZ &v) {
    const Fp2 *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        fp_lds_store<LANES>(lds, 2 * k, t, coord[k]->c0);
        fp_lds_store<LANES>(lds, 2 * k + 1, t, coord[k]->c1);
    }
}
template <int LANES>
static __device__ __forceinline__ G2XYZZ g2_lds_load(const uint4 *lds, uint32_t t) {
    G2XYZZ v;
    Fp2 *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        coord[k]->c0 = fp_lds_load<LANES>(lds, 2 * k, t);
        coord[k]->c1 = fp_lds_load<LANES>(lds, 2 * k + 1, t);
    }
    return v;
}

// sum_d d * bucket[d] = sum_j 2^j * S_j with S_j = the sum of the buckets whose index has bit j set: workgroup (w, j) forms S_j of
// window w by a tree over its 128 buckets — seven levels of full additions instead of a 255-long running sum
__global__ void __launch_bounds__(G2_MSM_B / 2) g2_msm_bitsum_kernel(const char *buckets, char *sums /* W * 8 * 256 */) {
    __shared__ uint4 lds[16 * (G2_MSM_B / 2)];
    const uint32_t w = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    const uint32_t d = ((t >> j) << (j + 1)) | (1u << j) | (t & ((1u << j) - 1u));  // the t-th index with bit j set
    G2XYZZ v = xyzz_load<Fp2>(buckets + 256 * ((size_t)w * G2_MSM_B + d));
    g2_lds_store<G2_MSM_B / 2>(lds, t, v);
    __syncthreads();
    for (uint32_t s = G2_MSM_B / 4; s >= 1; s >>= 1) {
        if (t < s) {
            v = xyzz_add(v, g2_lds_load<G2_MSM_B / 2>(lds, t + s));
            g2_lds_store<G2_MSM_B / 2>(lds, t, v);
        }
        __syncthreads();
    }
    if (t == 0) xyzz_store(sums + 256 * ((size_t)w * G2_MSM_C + j), v);
}

// window sums T_w = sum_j 2^j S_wj (lane w, 8 doublings and additions), then Horner over the windows in lane 0: result = sum_w 2^(8w) T_w.
// d_out17 = affine xy[16] followed by a flag word (low byte 1 = identity).
__global__ void __launch_bounds__(64) g2_msm_final_kernel(const char *sums, uint64_t *d_out17) {
    __shared__ uint4 lds[16 * G2_MSM_W];
    const uint32_t w = threadIdx.x;
    if (w < G2_MSM_W) {
        G2XYZZ t = G2XYZZ::identity();
        for (int j = G2_MSM_C - 1; j >= 0; j--) {
            t = xyzz_dbl(t);
            t = xyzz_add(t, xyzz_load<Fp2>(sums + 256 * ((size_t)w * G2_MSM_C + j)));
        }
        g2_lds_store<G2_MSM_W>(lds, w, t);
    }
    __syncthreads();
    if (w != 0) return;
    G2XYZZ acc = G2XYZZ::identity();
    for (int k = G2_MSM_W - 1; k >= 0; k--) {
        for (int j = 0; j < G2_MSM_C; j++) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, g2_lds_load<G2_MSM_W>(lds, (uint32_t)k));
    }
    G2Affine r;
    const bool isinf = xyzz_to_affine(acc, r);
    affine_store(d_out17, r);
    d_out17[16] = isinf ? 1 : 0;
}

__global__ void g2_identity_record_kernel(uint64_t *d_out17) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    affine_store(d_out17, G2Affine::identity());
    d_out17[16] = 1;
}

struct G2MsmScratch {
    uint8_t *dig;
    uint32_t *idx;
    char *buckets, *sums;
    G2MsmScratch(Staging &sg, size_t n) {
        const size_t n4 = (n + 3) & ~(size_t)3;
        dig = sg.out<uint8_t>(G2_MSM_W * n4);
        idx = sg.out<uint32_t>(G2_MSM_W * n4 * 4);
        buckets = sg.out<char>((size_t)G2_MSM_W * G2_MSM_B * 256);
        sums = sg.out<char>((size_t)G2_MSM_W * G2_MSM_C * 256);
    }
};

// enqueues the launch set on st; the scratch must outlive it (its Staging synchronises before it releases)
static void g2_msm_enqueue(const uint64_t *d_xy, const uint8_t *d_inf, const uint64_t *d_scalars, uint32_t n, hipStream_t st, const G2MsmScratch &sc,
                           uint64_t *d_out17) {
    const uint32_t n4 = (n + 3u) & ~3u;
    hipLaunchKernelGGL(g2_msm_digits_kernel, dim3(div_up(n4, 256)), dim3(256), 0, st, d_scalars, d_inf, n, n4, sc.dig);
    hipLaunchKernelGGL(g2_msm_bucket_kernel, dim3(G2_MSM_W), dim3(G2_MSM_B), 0, st, sc.dig, d_xy, n4, sc.idx, sc.buckets);
    hipLaunchKernelGGL(g2_msm_bitsum_kernel, dim3(G2_MSM_W, G2_MSM_C), dim3(G2_MSM_B / 2), 0, st, sc.buckets, sc.sums);
    hipLaunchKernelGGL(g2_msm_final_kernel, dim3(1), dim3(64), 0, st, sc.sums, d_out17);
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
    const int c = n <= 256 ? 4 : 8, W = (254 + c - 1) / c;
    const uint32_t rows_per_w = (1u << c) - 1u, n_rows = (uint32_t)W * rows_per_w;
    Staging sg(lib_stream());
    const uint64_t *d_base = sg.in(base_xy, 128), *d_sc = sg.in(scalars, n * 32);
    char *d_bw = sg.out<char>((size_t)W * 256);
    uint64_t *d_tab = sg.out<uint64_t>((size_t)n_rows * 128), *d_out = sg.out<uint64_t>(n * 128);
    uint8_t *d_tinf = sg.out<uint8_t>(n_rows), *d_inf = sg.out<uint8_t>(n);
    if (sg.ok()) {
        hipLaunchKernelGGL(g2_fb_window_bases_kernel, dim3(1), dim3(G2_FB_W_MAX), 0, sg.st, d_base, c, W, d_bw);
        hipLaunchKernelGGL(g2_fb_rows_kernel, dim3(div_up(n_rows, 64)), dim3(64), 0, sg.st, d_bw, n_rows, c, rows_per_w, d_tab, d_tinf);
        hipLaunchKernelGGL(g2_fb_mul_kernel, dim3(div_up(n, 64)), dim3(64), 0, sg.st, d_tab, d_tinf, d_sc, n, c, W, rows_per_w, d_out, d_inf);
        sg.launched();
    }
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
    const G2MsmScratch sc(sg, n);
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
    const G2MsmScratch sc(sg, n);
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
