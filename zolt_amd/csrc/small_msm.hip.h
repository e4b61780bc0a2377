// small_msm.hip.h — the bucket MSM for SHORT vectors over bases that are not tabled, for either group: msmG2 (dory.zig:693-703) and the
// MSMs of Dory's second reduce message over v1 / v2, which change every round (:1589-1592). 8-bit unsigned windows, 32 of them, a
// workgroup per window and a lane per bucket; the digits are counting-sorted inside the workgroup (no atomics, no global sort), buckets
// are combined by per-bit tree sums (no 255-long running sum) and the 32 window sums by Horner — the one serial chain left (254
// doublings). The group is the field F of xyzz.hip.h (Fp: G1, Fp2: G2); up to SMSM_MAX_JOBS independent MSMs ride in ONE launch set (a
// message's plus / minus pair): the job is a grid dimension, its arrays a table passed by value.
// Device pointers in, one record out per job: affine coordinates followed by a flag word (low byte 1 = identity). The kernels have
// internal linkage: each translation unit that includes this header launches its own copies.
#pragma once
#include "common.hip.h"
#include "g1.hip.h"
#include "g2.hip.h"

namespace zg {

static constexpr int SMSM_C = 8, SMSM_W = 32, SMSM_B = 1 << SMSM_C, SMSM_MAX_JOBS = 4;

struct SmallMsmJob {
    const uint64_t *xy;      // n affine points of the group
    const uint8_t *inf;      // n flags, or nullptr
    const uint64_t *scalars; // n Montgomery Fr elements
    uint64_t *out;           // the record: 2 * F::BYTES / 8 words of coordinates, then the flag word
    uint32_t n;
};
struct SmallMsmJobs {
    SmallMsmJob job[SMSM_MAX_JOBS];
    uint32_t n4;  // the digit rows' length: 4 * ceil(max n / 4), at least 4
};

// scratch of one launch set; per job: W digit rows, W index rows, W * 256 buckets, W * 8 bit sums
struct SmallMsmScratch {
    uint8_t *dig = nullptr;
    uint32_t *idx = nullptr;
    char *buckets = nullptr, *sums = nullptr;
    static size_t n4_of(size_t n) { return n ? (n + 3) & ~(size_t)3 : 4; }
    static size_t dig_bytes(size_t n, int jobs) { return (size_t)jobs * SMSM_W * n4_of(n); }
    static size_t idx_bytes(size_t n, int jobs) { return dig_bytes(n, jobs) * 4; }
    static size_t bucket_bytes(size_t xyzz_bytes, int jobs) { return (size_t)jobs * SMSM_W * SMSM_B * xyzz_bytes; }
    static size_t sum_bytes(size_t xyzz_bytes, int jobs) { return (size_t)jobs * SMSM_W * SMSM_C * xyzz_bytes; }
    SmallMsmScratch() = default;
    // for launch sets of up to `jobs` MSMs of up to n points of a group whose XYZZ point has xyzz_bytes (128: G1, 256: G2)
    SmallMsmScratch(Staging &sg, size_t n, size_t xyzz_bytes, int jobs = 1) {
        dig = sg.out<uint8_t>(dig_bytes(n, jobs));
        idx = sg.out<uint32_t>(idx_bytes(n, jobs));
        buckets = sg.out<char>(bucket_bytes(xyzz_bytes, jobs));
        sums = sg.out<char>(sum_bytes(xyzz_bytes, jobs));
    }
};

// digits, window-major: dig[(job * W + w) * n4 + i] = bits [8w, 8w + 8) of scalar i (0 for an identity base and in the padding up to n4)
static __global__ void __launch_bounds__(256) smsm_digits_kernel(SmallMsmJobs jobs, uint8_t *dig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n4 = jobs.n4;
    if (i >= n4) return;
    const SmallMsmJob &jb = jobs.job[blockIdx.y];
    Fr s = Fr::zero();
    if (i < jb.n && !(jb.inf && jb.inf[i])) s = fe_from_mont(fe_load<FrParams>(jb.scalars + 4 * (size_t)i));
    uint8_t *row = dig + (size_t)blockIdx.y * SMSM_W * n4;
#pragma unroll
    for (int w = 0; w < SMSM_W; w++) row[(size_t)w * n4 + i] = (uint8_t)(s.l[w >> 2] >> (8 * (w & 3)));
}

// one workgroup per (window, job), lane d = bucket d. The window's digits are counting-sorted by the workgroup itself — every lane walks
// the whole digit row (uniform loads, a compare per entry), counts its matches, takes its offset from a prefix sum over the 256 counts and
// walks the row again to list them — and then the lanes add their lists in lockstep: a mixed addition always runs with the whole wave.
template <class F>
static __global__ void __launch_bounds__(SMSM_B) smsm_bucket_kernel(SmallMsmJobs jobs, const uint8_t *dig, uint32_t *idx, char *buckets) {
    __shared__ uint32_t s_cnt[SMSM_B];
    const uint32_t w = blockIdx.x, d = threadIdx.x, n4 = jobs.n4;
    const size_t wj = (size_t)blockIdx.y * SMSM_W + w;
    const uint64_t *xy = jobs.job[blockIdx.y].xy;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(dig + wj * n4);
    uint32_t *list = idx + wj * n4;
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
    XyzzT<F> acc = XyzzT<F>::identity();
    for (uint32_t k = 0; k < cnt; k++) acc = xyzz_madd(acc, affine_load<F>(xy + (2 * F::BYTES / 8) * (size_t)list[off + k]));
    xyzz_store(buckets + 4 * F::BYTES * (wj * SMSM_B + d), acc);
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
static __device__ __forceinline__ void xyzz_lds_store(uint4 *lds, uint32_t t, const G2XYZZ &v) {
    const Fp2 *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        fp_lds_store<LANES>(lds, 2 * k, t, coord[k]->c0);
        fp_lds_store<LANES>(lds, 2 * k + 1, t, coord[k]->c1);
    }
}
template <int LANES>
static __device__ __forceinline__ void xyzz_lds_store(uint4 *lds, uint32_t t, const XYZZ &v) {
    const Fp *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) fp_lds_store<LANES>(lds, k, t, *coord[k]);
}
template <int LANES>
static __device__ __forceinline__ void xyzz_lds_load(const uint4 *lds, uint32_t t, G2XYZZ &v) {
    Fp2 *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        coord[k]->c0 = fp_lds_load<LANES>(lds, 2 * k, t);
        coord[k]->c1 = fp_lds_load<LANES>(lds, 2 * k + 1, t);
    }
}
template <int LANES>
static __device__ __forceinline__ void xyzz_lds_load(const uint4 *lds, uint32_t t, XYZZ &v) {
    Fp *coord[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) *coord[k] = fp_lds_load<LANES>(lds, k, t);
}

// sum_d d * bucket[d] = sum_j 2^j * S_j with S_j = the sum of the buckets whose index has bit j set: workgroup (w, j, job) forms S_j of
// window w by a tree over its 128 buckets — seven levels of full additions instead of a 255-long running sum
template <class F>
static __global__ void __launch_bounds__(SMSM_B / 2) smsm_bitsum_kernel(const char *buckets, char *sums) {
    __shared__ uint4 lds[(4 * F::BYTES / 16) * (SMSM_B / 2)];
    const uint32_t w = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    const size_t wj = (size_t)blockIdx.z * SMSM_W + w;
    const uint32_t d = ((t >> j) << (j + 1)) | (1u << j) | (t & ((1u << j) - 1u));  // the t-th index with bit j set
    XyzzT<F> v = xyzz_load<F>(buckets + 4 * F::BYTES * (wj * SMSM_B + d));
    xyzz_lds_store<SMSM_B / 2>(lds, t, v);
    __syncthreads();
    for (uint32_t s = SMSM_B / 4; s >= 1; s >>= 1) {
        if (t < s) {
            XyzzT<F> o;
            xyzz_lds_load<SMSM_B / 2>(lds, t + s, o);
            v = xyzz_add(v, o);
            xyzz_lds_store<SMSM_B / 2>(lds, t, v);
        }
        __syncthreads();
    }
    if (t == 0) xyzz_store(sums + 4 * F::BYTES * (wj * SMSM_C + j), v);
}

// window sums T_w = sum_j 2^j S_wj (lane w, 8 doublings and additions), then Horner over the windows in lane 0: result = sum_w 2^(8w) T_w;
// a workgroup per job
template <class F>
static __global__ void __launch_bounds__(64) smsm_final_kernel(SmallMsmJobs jobs, const char *sums) {
    __shared__ uint4 lds[(4 * F::BYTES / 16) * SMSM_W];
    const uint32_t w = threadIdx.x;
    if (w < SMSM_W) {
        const size_t wj = (size_t)blockIdx.x * SMSM_W + w;
        XyzzT<F> t = XyzzT<F>::identity();
        for (int j = SMSM_C - 1; j >= 0; j--) {
            t = xyzz_dbl(t);
            t = xyzz_add(t, xyzz_load<F>(sums + 4 * F::BYTES * (wj * SMSM_C + j)));
        }
        xyzz_lds_store<SMSM_W>(lds, w, t);
    }
    __syncthreads();
    if (w != 0) return;
    XyzzT<F> acc = XyzzT<F>::identity();
    for (int k = SMSM_W - 1; k >= 0; k--) {
        for (int j = 0; j < SMSM_C; j++) acc = xyzz_dbl(acc);
        XyzzT<F> o;
        xyzz_lds_load<SMSM_W>(lds, (uint32_t)k, o);
        acc = xyzz_add(acc, o);
    }
    AffineT<F> r;
    const bool isinf = xyzz_to_affine(acc, r);
    uint64_t *out = jobs.job[blockIdx.x].out;
    affine_store(out, r);
    out[2 * F::BYTES / 8] = isinf ? 1 : 0;
}

// enqueues the launch set of n_jobs MSMs (1..SMSM_MAX_JOBS, each of at most the n the scratch was sized for) on st; the scratch must
// outlive it
template <class F>
static void small_msm_enqueue(const SmallMsmJob *job, int n_jobs, hipStream_t st, const SmallMsmScratch &sc) {
    SmallMsmJobs jobs = {};
    uint32_t n = 0;
    for (int j = 0; j < n_jobs; j++) {
        jobs.job[j] = job[j];
        if (job[j].n > n) n = job[j].n;
    }
    jobs.n4 = (uint32_t)SmallMsmScratch::n4_of(n);
    hipLaunchKernelGGL(smsm_digits_kernel, dim3(div_up(jobs.n4, 256), n_jobs), dim3(256), 0, st, jobs, sc.dig);
    hipLaunchKernelGGL(smsm_bucket_kernel<F>, dim3(SMSM_W, n_jobs), dim3(SMSM_B), 0, st, jobs, sc.dig, sc.idx, sc.buckets);
    hipLaunchKernelGGL(smsm_bitsum_kernel<F>, dim3(SMSM_W, SMSM_C, n_jobs), dim3(SMSM_B / 2), 0, st, sc.buckets, sc.sums);
    hipLaunchKernelGGL(smsm_final_kernel<F>, dim3(n_jobs), dim3(64), 0, st, jobs, sc.sums);
}

}  // namespace zg
