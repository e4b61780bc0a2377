// msm.hip — BN254 G1 multi-scalar multiplication on gfx950.
//
// Replaces the reference's single-threaded Pippenger (/root/reference/src/msm/mod.zig:375-438:
// c = 8, 32 windows, 255 Jacobian buckets on the stack, per-window fromMontgomery) with a
// pipeline shaped for 256 CUs and 288 GB of HBM:
//
//   upload (once per SRS)   bases -> table[l][i] = 2^(c*G*l) * P_i as 64-byte rows (l < L "precompute
//                           levels", stored in the accumulate kernel's lazy 29-bit-limb format); with L = W
//                           every window of a scalar lands in ONE shared bucket set and no window-combining
//                           doublings remain at MSM time.
//   msm_digits_lds          one fromMontgomery per scalar (the reference does 32), then W signed c-bit
//                           digits -> keys (bucket group g, |digit|-1); per-block histogram in LDS
//   msm_colscan / scan_a/b / scatter_lds   counting sort of the n*W (key, point-ref) pairs: per-block
//                           offsets, two-pass coalesced scan, scatter with LDS cursors (no global atomics)
//   msm_partition / fine_count / fine_offsets / fine_place   the same sort in two LDS-staged passes (coarse bins,
//                           then slices of a bin by fine key) for >= 8192 buckets: all HBM traffic coalesced
//   msm_accumulate_chunk    the sorted list is cut into equal chunks, one per thread, whatever the bucket
//                           sizes (skew-robust); complete XYZZ mixed adds on lazy limbs; one partial per
//                           bucket run
//   msm_bucket_combine / heavy_wave / heavy_a/b   per-bucket sums of the partials: GS lanes, a wave, or
//                           block trees depending on how many partials a bucket has
//   msm_bitsum              sum_k k*B_k = sum_b 2^b * T_b,  T_b = sum of the buckets whose index has
//                           bit b set: c plain tree sums (log depth) instead of the reference's
//                           serial running sum (a lone GPU lane needs ~10 us per point add)
//   msm_rowcol / bits2d     the same T_b for c >= 11 from row and column sums of the bucket matrix (every bucket
//                           added twice instead of (c-1)/2 times)
//   msm_final               b doublings of T_b in parallel quads, tree sum, window Horner if G > 1,
//                           one inversion (safegcd) -> affine
// Every kernel but the accumulation raises its wave priority: they are short dependent chains that would otherwise
// get a third of the issue slots beside another stream's accumulate waves.
//
// Bucket sums are order-independent group sums and the final affine coordinates are
// canonical field values, so the 64-byte result is bit-identical to the reference's
// MSM(F,G).compute whatever c, L and the scheduling are (tests/test_gpu_msm.py).
#include <string.h>

#include <mutex>
#include <vector>

#include "common.hip.h"
#include "g1.hip.h"
#include "g1_29.hip.h"
#include "g1_29x4.hip.h"
#include "msm_plan.h"

// Every MSM kernel except the bucket accumulation is short and mostly a chain of dependent operations; when it shares a SIMD with
// two accumulate waves of another stream the arbiter gives it a third of the issue slots and its latency triples, which
// stretches the per-stream chain digits -> sort -> accumulate -> reduce. Raised wave priority lets these kernels issue first;
// the accumulation fills the remaining slots (its total work is unchanged).
#ifndef ZG_TAIL_PRIO
#define ZG_TAIL_PRIO 3
#endif
#define ZG_HIPRIO() __builtin_amdgcn_s_setprio(ZG_TAIL_PRIO)

struct zg_bases_s {
    size_t n = 0;
    int device = -1;  // the HIP device the table and the workspaces live on
    zg::MsmPlan plan;
    char *d_table = nullptr;     // L * n * 64 B
    uint8_t *d_inf = nullptr;    // n B or null
    uint64_t *d_scal = nullptr;  // staging for host scalars, n * 32 B
    // One MSM in flight needs one workspace ("lane"). Several lanes let independent MSMs issued on different
    // streams overlap: the latency-bound tail of one runs under the ALU-bound accumulation of the next.
    struct Lane {
        uint32_t *d_dig = nullptr, *d_sorted = nullptr, *d_hist = nullptr, *d_starts = nullptr;
        uint32_t *d_blockhist = nullptr, *d_tmp = nullptr, *d_cstarts = nullptr, *d_fine = nullptr;  // the sort's buffers (zg::SortWords)
        zg::SortWords sort_cap;           // ... their sizes (a point slice may sort under its own plan: slice_sort_plan)
        char *d_partial = nullptr;        // NK * 144 B: bucket sums (lazy 29-bit-limb XYZZ records)
        char *d_slice_buckets = nullptr;  // point slices (msm_enqueue_lane): the bucket sums of slices 1 .. S-1, built on first use
        size_t slice_buckets = 0;         // ... how many sets it holds
        uint32_t *d_slice_meta = nullptr; // ... and per slice: starts | nzrank | nzlist | nzend | MsmState
        char *d_bits = nullptr;           // G * c * PB * 144 B: per-bit partial sums
        char *d_rg = nullptr;             // G * 128 B: per-group results
        uint32_t *d_nzrank = nullptr;     // NK + 1: non-empty buckets before k
        uint32_t *d_nzlist = nullptr;     // NK: the non-empty buckets, compacted
        uint32_t *d_nzend = nullptr;      // NK + 1: where the run of the r-th non-empty bucket ends in the sorted list
        uint32_t *d_scan_tmp = nullptr;   // 2*NK + 2*tiles: tile-local scans and tile totals
        char *d_part = nullptr;           // (NT + NK) * 144 B: per-(chunk, bucket-run) partial sums
        char *d_part2 = nullptr;          // heavy-bucket stage-A partials
        uint32_t *d_heavy = nullptr;      // 2*NK: heavy bucket list, then huge bucket list
        void *d_state = nullptr;          // MsmState
        hipEvent_t done = nullptr;        // recorded after the lane's last MSM; the next user waits on it
        hipStream_t last_st = nullptr;    // ... and the stream it was recorded on
        bool used = false;
    };
    std::vector<Lane> lanes;
    size_t next_lane = 0;
    // zg_msm_g1_batch: k short scalar vectors over the same bases run as ONE launch set (k times the bucket groups);
    // its workspace is built on first use and kept while (k, n) fit
    Lane batch_lane;
    zg::MsmPlan batch_plan;
    size_t batch_n = 0;
    struct {  // the last fuse verdict (fuse_set_size): k vectors of n scalars -> sets of kc vectors (0: not fused)
        size_t n = 0, k = 0, kc = 0;
        bool wide_ok = false;
    } fuse;
    // long vectors are not fused: they rotate over the caller's stream and three forked helper streams instead
    static constexpr int NAUX = 3;  // four streams with the caller's: fewer can land two of them on one of HIP's four hardware queues
    hipStream_t aux[NAUX] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[NAUX] = {nullptr, nullptr, nullptr};
    // Wide-window handles (2^15 buckets) also keep a narrow-window table of their first SIDE_TABLE_POINTS bases: MSMs over a
    // short prefix (HyperKZG.commit of a short polynomial on a long SRS, HyperKZG.open's last levels) then sort into 2^7
    // buckets instead of 2^15, and batches of them can be fused into one launch set. Same results, by construction.
    zg_bases_s *small = nullptr;
    uint64_t *d_out = nullptr;  // 16 x u64: result record + flag
    uint64_t *h_out = nullptr;  // pinned mirror
    uint64_t *d_slice_parts = nullptr;  // zg_msm_g1 (host scalars, sliced): one Jacobian partial per slice
    // rows of a batch on a handle without a table (msm_rows_shared_tail): the bucket sums of every row side by side, the reduction's
    // bit sums / rows / columns and group results for all of them, sized for rows_cap rows; rows_done: the last set that used them
    char *d_rows_buckets = nullptr, *d_rows_bits = nullptr, *d_rows_rg = nullptr;
    size_t rows_cap = 0;
    hipEvent_t rows_done = nullptr;
    std::mutex mu;
};

namespace zg {

// ------------------------------------------------------------------ kernels

// Table build: level 0 = the bases; level l = 2^(c*G) * level (l-1), as affine.
// Levels per inversion: the chain keeps its Jacobian point across levels; every level leaves (X, Y, Z, product of the group's earlier Zs) in a
// 144-byte record of `scratch` (n * min(levels - 1, PRE_GROUP) records, index j * n + i), one safegcd inversion per group of PRE_GROUP levels
// then yields every 1 / Z_j on the way back (Montgomery's trick: two products per level) and the rows are written as affine points —
// 7 products per level instead of an inversion (~80 products' worth), and Jacobian doublings (945 multiply-adds) instead of XYZZ ones
// (1269): 2^20 bases x 15 levels 20.2 -> 13 ms. Rows are lazy representatives (< 1.1p) of the same affine coordinates as before.
constexpr int PRE_GROUP = 7;
constexpr size_t PRE_CHUNK = (size_t)1 << 21;  // bases per launch of the table kernel (bounds its records)
// A launch carries up to TWO tables: job `side` (the handle's side table: 2^14 bases, 32 narrow levels — a 2.4 ms latency chain on 64
// workgroups) takes the first side.blocks workgroups, the main table's the rest. Workgroups are dispatched in index order, so the side
// table's chain starts first and runs UNDER the main table's thousands of workgroups: no second stream (a stream created for it would
// move the caller's later streams onto other hardware queues, an idle one may share the launch stream's queue and run behind it).
struct PreJob {
    const uint64_t *xy;
    const uint8_t *inf;
    size_t n;          // bases of the handle (row stride of its table)
    int levels, dbl_per_level;
    char *table, *scratch;
    size_t first, count;  // this launch: bases [first, first + count); the records of base i sit at local index i - first (stride count)
    unsigned blocks;      // workgroups of this job in the launch
};
__global__ void __launch_bounds__(256) msm_precompute_kernel(PreJob side, PreJob main_job) {
    const bool is_side = blockIdx.x < side.blocks;
    const PreJob &jb = is_side ? side : main_job;
    const uint64_t *xy = jb.xy;
    const uint8_t *inf = jb.inf;
    const size_t n = jb.n, first = jb.first, count = jb.count;
    const int levels = jb.levels, dbl_per_level = jb.dbl_per_level;
    char *table = jb.table, *scratch = jb.scratch;
    const size_t li = (size_t)(blockIdx.x - (is_side ? 0u : side.blocks)) * blockDim.x + threadIdx.x, i = first + li;
    if (li >= count) return;
    Affine p = affine_load(xy + 8 * i);
    Jac29 a;
    a.x = f29_from_fp(p.x);
    a.y = f29_from_fp(p.y);
    f29_store_packed(table + 64 * i, a.x);
    f29_store_packed(table + 64 * i + 32, a.y);
    if (inf && inf[i]) return;  // infinity bases are never referenced (digits are suppressed)
    F29 one29;
#pragma unroll
    for (int k = 0; k < 9; k++) one29.l[k] = Fp29::ONE[k];
    a.z = one29;
    for (int l0 = 1; l0 < levels; l0 += PRE_GROUP) {
        const int g = levels - l0 < PRE_GROUP ? levels - l0 : PRE_GROUP;
        F29 pref = one29;
        for (int j = 0; j < g; j++) {
            for (int k = 0; k < dbl_per_level; k++) a = jac29_dbl(a);
            XYZZ29 rec;
            rec.x = a.x; rec.y = a.y; rec.zz = a.z; rec.zzz = pref;
            xyzz29_store(scratch + 144 * ((size_t)j * count + li), rec);
            pref = f29_mul(pref, a.z);
        }
        F29 t = f29_from_fp(fe_inv_safegcd(f29_to_fp(pref)));  // 1 / (Z_0 ... Z_(g-1))
        for (int j = g - 1; j >= 0; j--) {
            const XYZZ29 rec = xyzz29_load(scratch + 144 * ((size_t)j * count + li));  // this thread's own record
            const F29 iz = f29_mul(t, rec.zzz);  // 1 / Z_j
            t = f29_mul(t, rec.zz);              // ... and Z_j leaves the running inverse
            const F29 iz2 = f29_sqr(iz);
            char *row = table + 64 * ((size_t)(l0 + j) * n + i);
            f29_store_packed(row, f29_mul(rec.x, iz2));                     // x = X / Z^2
            f29_store_packed(row + 32, f29_mul(rec.y, f29_mul(iz2, iz)));   // y = Y / Z^3
        }
    }
}

// The same table with an inversion per level and no scratch (rounds 1-4): kept for the case that the scratch does not fit, and as the
// A/B reference (ZG_MSM_PRECOMPUTE_V1=1)
__global__ void __launch_bounds__(256) msm_precompute_v1_kernel(const uint64_t *xy, const uint8_t *inf, size_t n, int levels,
                                                                int dbl_per_level, char *table) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine p = affine_load(xy + 8 * i);
    // rows are stored in the accumulate kernel's format: x, y as packed Montgomery-2^261 values (fp29.hip.h)
    F29 px = f29_from_fp(p.x), py = f29_from_fp(p.y);
    f29_store_packed(table + 64 * i, px);
    f29_store_packed(table + 64 * i + 32, py);
    if (inf && inf[i]) return;  // infinity bases are never referenced (digits are suppressed)
    F29 one29;
#pragma unroll
    for (int k = 0; k < 9; k++) one29.l[k] = Fp29::ONE[k];
    for (int l = 1; l < levels; l++) {
        XYZZ29 a;
        a.x = px; a.y = py; a.zz = one29; a.zzz = one29;
        for (int k = 0; k < dbl_per_level; k++) a = xyzz29_dbl(a);  // never the identity: the group has odd prime order
        // back to affine in the lazy domain: 1/Z = ZZ/ZZZ, x = X/Z^2, y = Y/ZZZ (one canonical-form inversion)
        F29 izzz = f29_from_fp(fe_inv_safegcd(f29_to_fp(a.zzz)));
        F29 iz = f29_mul(izzz, a.zz);
        px = f29_mul(a.x, f29_sqr(iz));
        py = f29_mul(a.y, izzz);
        char *row = table + 64 * ((size_t)l * n + i);
        f29_store_packed(row, px);
        f29_store_packed(row + 32, py);
    }
}

// Signed-digit decomposition. The reference extracts unsigned 8-bit windows of the canonical
// integer (getWindow, msm/mod.zig:441-471) and converts from Montgomery inside every call;
// here: one conversion, digits in [-2^(c-1), 2^(c-1)], so a group needs 2^(c-1) buckets.
template <int C>
__global__ void __launch_bounds__(256) msm_digits_kernel(const uint64_t *scalars, const uint8_t *inf, uint32_t n, uint32_t n_pts, int G,
                                                         uint32_t *dig, uint32_t *hist) {
    constexpr int W = (255 + C - 1) / C;
    constexpr uint32_t NB = 1u << (C - 1);
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fr s = fr_from_mont29(fe_load<FrParams>(scalars + 4 * (size_t)i));
    uint32_t batch = i / n_pts, pt = i - batch * n_pts;  // scalar vector `batch`, base `pt` (n == n_pts: one MSM)
    bool skip = inf && inf[pt];  // msm/mod.zig:407: infinity bases contribute nothing
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const int bit = w * C, limb = bit / 32, sh = bit % 32;
        uint32_t v = s.l[limb] >> sh;
        if (sh + C > 32 && limb + 1 < 8) v |= s.l[limb + 1] << (32 - sh);
        v = (v & ((1u << C) - 1u)) + carry;
        uint32_t neg = v > NB ? 1u : 0u;
        uint32_t d = neg ? (1u << C) - v : v;
        carry = neg;
        uint32_t e = 0xFFFFFFFFu;
        if (d != 0 && !skip) {
            uint32_t key = (batch * (uint32_t)G + (uint32_t)(w % G)) * NB + (d - 1);
            e = key | (neg << 31);
            atomicAdd(&hist[key], 1u);
        }
        dig[(size_t)w * n + i] = e;
    }
}

// exclusive scan of the bucket histogram (NK <= 2^21 entries), one block
// Exclusive scan of the bucket histogram in two coalesced passes (a one-block scan with strided slices was
// L2-latency-bound: 83 us for 32768 buckets). Pass A: each 1024-bucket tile is scanned in LDS (bucket sizes and
// non-empty flags) and its totals are published. Pass B: every tile adds the totals of the tiles before it and
// writes starts / nzrank / the compacted list of non-empty buckets.
__global__ void __launch_bounds__(1024) msm_scan_a_kernel(const uint32_t *__restrict__ hist, uint32_t NK, uint32_t *__restrict__ loc,
                                                          uint32_t *__restrict__ locz, uint32_t *__restrict__ tile_tot) {
    ZG_HIPRIO();
    __shared__ uint32_t sh[1024], shz[1024];
    uint32_t tid = threadIdx.x, k = blockIdx.x * 1024 + tid;
    uint32_t h = k < NK ? hist[k] : 0u, z = h ? 1u : 0u;
    sh[tid] = h;
    shz[tid] = z;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        uint32_t v = tid >= o ? sh[tid - o] : 0, vz = tid >= o ? shz[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        shz[tid] += vz;
        __syncthreads();
    }
    if (k < NK) {
        loc[k] = sh[tid] - h;    // exclusive within the tile
        locz[k] = shz[tid] - z;
    }
    if (tid == 1023) {
        tile_tot[2 * blockIdx.x] = sh[1023];
        tile_tot[2 * blockIdx.x + 1] = shz[1023];
    }
}

__global__ void __launch_bounds__(1024) msm_scan_b_kernel(const uint32_t *__restrict__ hist, uint32_t NK, const uint32_t *__restrict__ loc,
                                                          const uint32_t *__restrict__ locz, const uint32_t *__restrict__ tile_tot,
                                                          uint32_t *__restrict__ starts, uint32_t *__restrict__ nzrank,
                                                          uint32_t *__restrict__ nzlist, uint32_t *__restrict__ nzend, uint32_t *__restrict__ state,
                                                          uint32_t nstate) {
    ZG_HIPRIO();
    __shared__ uint32_t pre[2];
    // the launch set's MsmState (heavy / huge bucket counters of the reduction and the arrival counters of the huge buckets) is
    // cleared here: one launch less than a memset
    if (state && blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < nstate; w += 1024) state[w] = 0;
    uint32_t tid = threadIdx.x, k = blockIdx.x * 1024 + tid;
    if (tid < 64) {  // one wave sums the totals of the preceding tiles (at most 2048 tiles)
        uint32_t a = 0, az = 0;
        for (uint32_t t = tid; t < blockIdx.x; t += 64) {
            a += tile_tot[2 * t];
            az += tile_tot[2 * t + 1];
        }
        for (int d = 32; d > 0; d >>= 1) {
            a += __shfl_down(a, d, 64);
            az += __shfl_down(az, d, 64);
        }
        if (tid == 0) {
            pre[0] = a;
            pre[1] = az;
        }
    }
    __syncthreads();
    if (k < NK) {
        uint32_t s = pre[0] + loc[k], r = pre[1] + locz[k];
        starts[k] = s;
        nzrank[k] = r;  // number of non-empty buckets before k
        uint32_t h = hist[k];
        if (h) {
            nzlist[r] = k;     // compacted list of the non-empty buckets
            nzend[r] = s + h;  // and the ends of their runs: the accumulate loop walks them by rank, without going through nzlist and starts
        }
        if (k == NK - 1) {
            starts[NK] = s + h;
            nzrank[NK] = r + (h ? 1u : 0u);
        }
    }
}

// counting-sort scatter; order inside a bucket is irrelevant (group sums commute).
// fill[] is the histogram array re-zeroed by the caller.
__global__ void __launch_bounds__(256) msm_scatter_kernel(const uint32_t *dig, uint32_t n, uint32_t n_pts, int G, size_t table_n,
                                                          uint32_t off, const uint32_t *starts, uint32_t *fill, uint32_t *sorted) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t w = blockIdx.y;
    if (i >= n) return;
    uint32_t e = dig[(size_t)w * n + i];
    if (e == 0xFFFFFFFFu) return;
    uint32_t key = e & 0x7FFFFFFFu;
    uint32_t pos = starts[key] + atomicAdd(&fill[key], 1u);
    uint32_t ref = (uint32_t)((size_t)(w / G) * table_n + off + i % n_pts);
    sorted[pos] = (e & 0x80000000u) | ref;
}

// Rows of a zero-padded matrix of scalar vectors by their LIVE lengths (HyperKZG.open's long levels: 2^19, 2^18, ... entries in rows of
// 2^19): the digit and sort kernels walk the compact index space [0, off[k]) — row j holds [off[j], off[j + 1]), its scalars sit at
// j * n_pts + (i - off[j]) — instead of k * n_pts scalars of which four in five are padding. k = 0: uniform rows of n_pts scalars.
struct RowOffs {
    uint32_t k;
    uint32_t off[33];
};
ZG_DEV void row_split(const RowOffs &r, uint32_t n_pts, uint32_t i, uint32_t &batch, uint32_t &pt) {
    if (r.k == 0) {
        batch = i / n_pts;
        pt = i - batch * n_pts;
        return;
    }
    uint32_t b = 0;
    while (b + 1 < r.k && i >= r.off[b + 1]) b++;
    batch = b;
    pt = i - r.off[b];
}

// ---- LDS-staged counting sort (used when the whole bucket histogram fits in LDS: NK*4 <= 128 KiB).
// One 1024-thread block per CU owns a contiguous slice of the scalars; its histogram and, later, its
// scatter cursors live in LDS (ds_add_rtn_u32), so the sort issues no global atomics at all. The global
// path above costs one device-scope atomic per digit, twice (histogram + scatter).
template <int C>
__global__ void __launch_bounds__(1024) msm_digits_lds_kernel(const uint64_t *scalars, const uint8_t *inf, uint32_t n, uint32_t n_pts,
                                                              int G, uint32_t per_block, uint32_t NK, int shift, uint32_t *dig,
                                                              uint32_t *blockhist, RowOffs rows) {
    ZG_HIPRIO();
    extern __shared__ uint32_t lds_hist[];
    constexpr int W = (255 + C - 1) / C;
    constexpr uint32_t NB = 1u << (C - 1);
    for (uint32_t k = threadIdx.x; k < NK; k += blockDim.x) lds_hist[k] = 0;
    __syncthreads();
    uint32_t i0 = blockIdx.x * per_block, i1 = i0 + per_block < n ? i0 + per_block : n;
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        uint32_t batch, pt;
        row_split(rows, n_pts, i, batch, pt);
        Fr s = fr_from_mont29(fe_load<FrParams>(scalars + 4 * (rows.k ? (size_t)batch * n_pts + pt : (size_t)i)));
        bool skip = inf && inf[pt];
        uint32_t carry = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int bit = w * C, limb = bit / 32, sh = bit % 32;
            uint32_t v = s.l[limb] >> sh;
            if (sh + C > 32 && limb + 1 < 8) v |= s.l[limb + 1] << (32 - sh);
            v = (v & ((1u << C) - 1u)) + carry;
            uint32_t neg = v > NB ? 1u : 0u;
            uint32_t d = neg ? (1u << C) - v : v;
            carry = neg;
            uint32_t e = 0xFFFFFFFFu;
            if (d != 0 && !skip) {
                uint32_t key = (batch * (uint32_t)G + (uint32_t)(w % G)) * NB + (d - 1);
                e = key | (neg << 31);
                atomicAdd(&lds_hist[key >> shift], 1u);  // shift > 0: coarse bins of the two-pass sort (NK = their number)
            }
            dig[(size_t)w * n + i] = e;
        }
    }
    __syncthreads();
    uint32_t *row = blockhist + (size_t)blockIdx.x * NK;
    for (uint32_t k = threadIdx.x; k < NK; k += blockDim.x) row[k] = lds_hist[k];
}

// per key: exclusive prefix over the blocks (in place) and the key's total
__global__ void __launch_bounds__(256) msm_colscan_kernel(uint32_t *blockhist, uint32_t nblk, uint32_t NK, uint32_t *total) {
    ZG_HIPRIO();
    uint32_t key = blockIdx.x * 256 + threadIdx.x;
    if (key >= NK) return;
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 16) {  // 16 independent loads in flight, then the in-place prefix
        uint32_t v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = (b0 + u < nblk) ? blockhist[(size_t)(b0 + u) * NK + key] : 0u;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (b0 + u < nblk) blockhist[(size_t)(b0 + u) * NK + key] = run;
            run += v[u];
        }
    }
    total[key] = run;
}

__global__ void __launch_bounds__(1024) msm_scatter_lds_kernel(const uint32_t *dig, uint32_t n, uint32_t n_pts, int W, int G,
                                                               size_t table_n, uint32_t off, uint32_t per_block, uint32_t NK,
                                                               const uint32_t *starts, const uint32_t *blockhist, uint32_t *sorted, RowOffs rows) {
    ZG_HIPRIO();
    extern __shared__ uint32_t lds_cur[];
    const uint32_t *row = blockhist + (size_t)blockIdx.x * NK;
    for (uint32_t k = threadIdx.x; k < NK; k += blockDim.x) lds_cur[k] = starts[k] + row[k];
    __syncthreads();
    uint32_t i0 = blockIdx.x * per_block, i1 = i0 + per_block < n ? i0 + per_block : n;
    if (i1 - i0 < blockDim.x) {
        // fewer scalars than threads (a short MSM): the (window, scalar) pairs are spread over the threads — with the window as the outer
        // loop a 16-point MSM of 51 windows walked 51 dependent load -> LDS atomic -> store rounds with 16 lanes busy (17 us of a 130 us call)
        const uint32_t cnt = i1 - i0, total = cnt * (uint32_t)W;
        for (uint32_t t = threadIdx.x; t < total; t += blockDim.x) {
            const uint32_t w = t / cnt, i = i0 + (t - w * cnt);
            uint32_t e = dig[(size_t)w * n + i];
            if (e == 0xFFFFFFFFu) continue;
            uint32_t pos = atomicAdd(&lds_cur[e & 0x7FFFFFFFu], 1u);
            uint32_t batch, pt;
            row_split(rows, n_pts, i, batch, pt);
            sorted[pos] = (e & 0x80000000u) | (uint32_t)((size_t)(w / (uint32_t)G) * table_n + off + pt);
        }
        return;
    }
    // four windows per trip, their digit loads issued together: a trip used to be one dependent load -> LDS atomic -> store round per
    // window (~0.9 us each: 33 us of a 1024-point MSM's 37 windows)
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        uint32_t batch, pt;
        row_split(rows, n_pts, i, batch, pt);
        for (int w0 = 0; w0 < W; w0 += 4) {
            uint32_t e[4];
#pragma unroll
            for (int u = 0; u < 4; u++) e[u] = w0 + u < W ? dig[(size_t)(w0 + u) * n + i] : 0xFFFFFFFFu;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (e[u] == 0xFFFFFFFFu) continue;
                uint32_t pos = atomicAdd(&lds_cur[e[u] & 0x7FFFFFFFu], 1u);
                sorted[pos] = (e[u] & 0x80000000u) | (uint32_t)((size_t)((uint32_t)(w0 + u) / (uint32_t)G) * table_n + off + pt);
            }
        }
    }
}

// ---- two-pass counting sort for many buckets (NK >= 8192). The single-pass scatter above writes runs of only
// n*W / (blocks * NK) entries per (block, bucket) — 2 entries = 8 bytes at 2^20 points — and rocprofv3 shows the price:
// WRITE_SIZE 514 MB for 64 MB of sorted references (every 64-byte line leaves L2 eight times, partially filled).
// Pass 1 (msm_scatter_lds_kernel with shift = fb) partitions by the HIGH key bits only: <= 8192 coarse bins, so a block
// writes runs of hundreds of bytes. Pass 2 (below) gives each coarse bin to one block: its entries are contiguous
// (~256 KiB, L2-resident), it counts the 2^fb fine keys in LDS, publishes the per-bucket histogram the accumulate
// scheduler needs, and places the entries — scattered 4-byte stores again, but confined to a region that is complete
// before it leaves L2.
// cstarts[b] = entries before coarse bin b (positions in the sorted list); tstarts[b] = the same with every bin rounded up to
// a multiple of 4 entries (positions in the intermediate buffer, so that pass 2 can use 16-byte loads); istarts[b] = work items
// before bin b, an item being a slice of at most FINE_SLICE entries of one bin (a skewed witness column can put half of all
// entries into one bin: it is then spread over many blocks instead of one).
__global__ void __launch_bounds__(1024) msm_coarse_base_kernel(const uint32_t *totals, uint32_t NCB, uint32_t *cstarts, uint32_t *tstarts,
                                                               uint32_t *istarts) {
    ZG_HIPRIO();
    __shared__ uint32_t sh[1024], sh4[1024], shi[1024];
    uint32_t tid = threadIdx.x, per = (NCB + 1023) / 1024, a = tid * per, b = a + per < NCB ? a + per : NCB;
    uint32_t s = 0, s4 = 0, si = 0;
    for (uint32_t k = a; k < b; k++) {
        s += totals[k];
        s4 += (totals[k] + 3u) & ~3u;
        si += (totals[k] + FINE_SLICE - 1) / FINE_SLICE;
    }
    sh[tid] = s;
    sh4[tid] = s4;
    shi[tid] = si;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        uint32_t v = tid >= o ? sh[tid - o] : 0, v4 = tid >= o ? sh4[tid - o] : 0, vi = tid >= o ? shi[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        sh4[tid] += v4;
        shi[tid] += vi;
        __syncthreads();
    }
    uint32_t run = sh[tid] - s, run4 = sh4[tid] - s4, runi = shi[tid] - si;  // exclusive
    for (uint32_t k = a; k < b; k++) {
        cstarts[k] = run;
        tstarts[k] = run4;
        istarts[k] = runi;
        run += totals[k];
        run4 += (totals[k] + 3u) & ~3u;
        runi += (totals[k] + FINE_SLICE - 1) / FINE_SLICE;
    }
    if (tid == 1023) {
        cstarts[NCB] = sh[1023];
        tstarts[NCB] = sh4[1023];
        istarts[NCB] = shi[1023];
    }
}

// pass 1: partition the digit entries by coarse bin (key >> fb). An intermediate entry keeps the fine key bits above the rb bits
// of the table-row reference: sign | fine << rb | ref. A block owns <= STAGE_ENTRIES entries (its scalars x W windows), sorts
// them by coarse bin INSIDE LDS (count, scan, place — LDS handles divergent addresses at full rate, the global store path
// handles about one divergent lane per two cycles per CU), and then copies every bin's run to its place in `tmp` with
// consecutive lanes on consecutive addresses: all HBM traffic of the pass is coalesced.
static constexpr uint32_t STAGE_ENTRIES = 32768;  // 128 KiB of LDS
// PLAIN: one bucket group and one scalar vector (the full-precompute single MSM) — level = window, point = scalar index; the
// general form divides by G and reduces modulo n_pts per entry (a select would evaluate both: 50 instructions per entry)
template <bool PLAIN>
__global__ void __launch_bounds__(1024) msm_partition_kernel(const uint32_t *dig, uint32_t n, uint32_t n_pts, int W, int G, size_t table_n,
                                                             uint32_t off, uint32_t per_block, uint32_t NCB, int fb, int rb,
                                                             const uint32_t *tstarts, const uint32_t *blockoff, uint32_t *tmp, int local_shift,
                                                             RowOffs rows) {
    ZG_HIPRIO();
    extern __shared__ uint32_t lds[];
    uint32_t *buf = lds, *cnt = lds + STAGE_ENTRIES, *lbase = cnt + NCB, *sums = lbase + NCB + 1;  // sums: 1024 scan partials
    const uint32_t tid = threadIdx.x, T = 1024, fmask = (1u << fb) - 1u;
    uint32_t i0 = blockIdx.x * per_block, cntl = i0 < n ? (n - i0 < per_block ? n - i0 : per_block) : 0;
    for (uint32_t k = tid; k < NCB; k += T) cnt[k] = 0;
    __syncthreads();
    // the block's entries stay in registers between the counting and the placing pass (<= 32 per thread). Register r holds
    // window w = r / JW, scalar (r % JW) * T + tid of the block, JW = ceil(cntl / T) in {1, 2} (two_pass_span keeps JW * W <= 32):
    // w and the row base are wave-uniform, so no per-entry division is needed to find them.
    const uint32_t jw2 = cntl > T ? 1u : 0u;
    uint32_t e[STAGE_ENTRIES / 1024];
#pragma unroll
    for (int r = 0; r < (int)(STAGE_ENTRIES / 1024); r++) {
        uint32_t w = (uint32_t)r >> jw2, j = ((uint32_t)r & jw2) * T + tid;
        e[r] = 0xFFFFFFFFu;
        if (w < (uint32_t)W && j < cntl) {
            uint32_t d = dig[(size_t)w * n + i0 + j];
            e[r] = d;  // key | sign, or 0xFFFFFFFF for a dropped digit
            if (d != 0xFFFFFFFFu) atomicAdd(&cnt[(d & 0x7FFFFFFFu) >> fb], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of cnt[0..NCB) -> lbase (each thread owns a contiguous run of bins)
    {
        uint32_t per = (NCB + T - 1) / T, a = tid * per, b = a + per < NCB ? a + per : NCB, sacc = 0;
        for (uint32_t k = a; k < b && k < NCB; k++) sacc += cnt[k];
        sums[tid] = sacc;
        __syncthreads();
        for (uint32_t o = 1; o < T; o <<= 1) {
            uint32_t v = tid >= o ? sums[tid - o] : 0;
            __syncthreads();
            sums[tid] += v;
            __syncthreads();
        }
        uint32_t run = sums[tid] - sacc;
        for (uint32_t k = a; k < b && k < NCB; k++) {
            lbase[k] = run;
            run += cnt[k];
            cnt[k] = 0;  // becomes the placing cursor
        }
        if (tid == T - 1) lbase[NCB] = sums[T - 1];
    }
    __syncthreads();
    // destinations of this block's bins (at most 3 per thread: NCB <= 3000), loaded now so that their latency hides under the placing pass
    const uint32_t *row = blockoff + (size_t)blockIdx.x * NCB;
    uint32_t dst_pre[3];
#pragma unroll
    for (int u = 0; u < 3; u++) {
        uint32_t k = (uint32_t)u * T + tid;
        dst_pre[u] = k < NCB ? tstarts[k] + row[k] : 0u;
    }
    // a thread's entries belong to at most two scalars (rows 0 and 1 of every window): their point indices are found once
    // (several scalar vectors lie back to back over the same bases: index modulo n_pts)
    uint32_t pt_row0 = i0 + tid, pt_row1 = i0 + T + tid, row_unused;
    if (!PLAIN) {
        row_split(rows, n_pts, i0 + tid, row_unused, pt_row0);
        row_split(rows, n_pts, i0 + T + tid, row_unused, pt_row1);
    }
#pragma unroll
    for (int r = 0; r < (int)(STAGE_ENTRIES / 1024); r++) {
        if (e[r] != 0xFFFFFFFFu) {
            uint32_t w = (uint32_t)r >> jw2;
            uint32_t key = e[r] & 0x7FFFFFFFu, bin = key >> fb, lvl = (PLAIN || G == 1) ? w : w / (uint32_t)G;
            uint32_t pt = ((uint32_t)r & jw2) ? pt_row1 : pt_row0;
            // a point slice keeps slice-local references level << local_shift | point in the INTERMEDIATE entries (fewer bits than a table
            // row index: more fine bits, fewer coarse bins); msm_fine_place_kernel writes table rows into the final list
            const uint32_t ref = local_shift ? (lvl << local_shift) | pt : (uint32_t)((size_t)lvl * table_n + off + pt);
            uint32_t packed = (e[r] & 0x80000000u) | ((key & fmask) << rb) | ref;
            buf[lbase[bin] + atomicAdd(&cnt[bin], 1u)] = packed;
        }
    }
    __syncthreads();
    // every bin's destination goes to LDS first (the placing cursors are done with): read inside the copy loop, the two global
    // loads per bin were a dependent ~2 us each, i.e. most of this kernel's time (NCB / 16 iterations per wave)
#pragma unroll
    for (int u = 0; u < 3; u++) {
        uint32_t k = (uint32_t)u * T + tid;
        if (k < NCB) cnt[k] = dst_pre[u];
    }
    __syncthreads();
    // copy-out: a group of sg lanes (64, 32 or 16, by the average run length) walks one bin's run; wave v takes the bins
    // v * (64 / sg) + group, stepping by 16 waves' worth
    const uint32_t avg = STAGE_ENTRIES / NCB, sg = avg >= 48 ? 64u : (avg >= 24 ? 32u : 16u), per = 64u / sg;
    const uint32_t lane = tid & 63, sub = lane / sg, sl = lane % sg;
    for (uint32_t bin = (tid >> 6) * per + sub; bin < NCB; bin += (T >> 6) * per) {
        uint32_t a = lbase[bin], b = lbase[bin + 1];
        uint32_t dst = cnt[bin];
        for (uint32_t j = a + sl; j < b; j += sg) tmp[dst + (j - a)] = buf[j];
    }
}

// pass 2, three launches over the work items (slices of coarse bins; the grid is an upper bound, surplus blocks exit):
//   count : fine-key histogram of the slice (LDS) -> slicecnt[item][f]
//   offsets (one block per bin): per fine key, exclusive prefix over the bin's slices (in place) and the bucket's size ->
//           hist[key]; exclusive prefix over the fine keys -> fbase[bin][f]
//   place : cursor[f] = cstarts[bin] + fbase[bin][f] + slicecnt[item][f]; scattered 4-byte stores confined to the bin's region
// Entries are read with 16-byte loads (bins are 16-byte aligned in tmp and FINE_SLICE is a multiple of 4).
ZG_DEV bool fine_item(uint32_t item, const uint32_t *istarts, uint32_t NCB, uint32_t &bin, uint32_t &q0) {
    if (item >= istarts[NCB]) return false;
    uint32_t lo = 0, hi = NCB;  // istarts[lo] <= item < istarts[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (istarts[mid] <= item) lo = mid; else hi = mid;
    }
    // bins without entries have no items: skip back over equal istarts values is not needed (istarts[lo] <= item < istarts[lo+1])
    bin = lo;
    q0 = (item - istarts[lo]) * FINE_SLICE;
    return true;
}

__global__ void __launch_bounds__(1024) msm_fine_count_kernel(const uint32_t *tmp, const uint32_t *cstarts, const uint32_t *tstarts,
                                                              const uint32_t *istarts, uint32_t NCB, int fb, int rb, uint32_t *slicecnt) {
    ZG_HIPRIO();
    __shared__ uint32_t cnt[128];
    __shared__ uint32_t sh_bin, sh_q0, sh_ok;
    uint32_t tid = threadIdx.x, nf = 1u << fb, fmask = nf - 1u;
    if (tid == 0) {
        uint32_t bb = 0, qq = 0;
        sh_ok = fine_item(blockIdx.x, istarts, NCB, bb, qq) ? 1u : 0u;
        sh_bin = bb;
        sh_q0 = qq;
    }
    if (tid < nf) cnt[tid] = 0;
    __syncthreads();
    if (!sh_ok) return;
    uint32_t bin = sh_bin, q0 = sh_q0;
    uint32_t total = cstarts[bin + 1] - cstarts[bin];
    uint32_t count = total - q0 < FINE_SLICE ? total - q0 : FINE_SLICE;
    const uint4 *src = reinterpret_cast<const uint4 *>(tmp + tstarts[bin] + q0);
    const uint32_t T = blockDim.x, quads = (count + 3) / 4;
    for (uint32_t qb = 0; qb < quads; qb += 2 * T) {
        uint4 v[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            uint32_t q = qb + u * T + tid;
            v[u] = q < quads ? src[q] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            uint32_t q = qb + u * T + tid, e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (4 * q + j < count) atomicAdd(&cnt[(e[j] >> rb) & fmask], 1u);
        }
    }
    __syncthreads();
    if (tid < nf) slicecnt[(size_t)blockIdx.x * nf + tid] = cnt[tid];
}

// place: the slice (<= FINE_SLICE = STAGE_ENTRIES entries, held in registers) is sorted by fine key inside LDS, then every
// fine key's run is copied to  cstarts[bin] + fbase[bin][f] + (prefix over the earlier slices)  with coalesced stores.
__global__ void __launch_bounds__(1024) msm_fine_place_kernel(const uint32_t *tmp, const uint32_t *cstarts, const uint32_t *tstarts,
                                                              const uint32_t *istarts, uint32_t NCB, int fb, int rb, const uint32_t *slicecnt,
                                                              const uint32_t *fbase, uint32_t *sorted, int local_shift, uint32_t table_n,
                                                              uint32_t off) {
    ZG_HIPRIO();
    extern __shared__ uint32_t lds[];
    uint32_t *buf = lds, *cnt = lds + STAGE_ENTRIES, *lbase = cnt + 128;  // lbase: 129 entries
    __shared__ uint32_t sh_bin, sh_q0, sh_ok;
    uint32_t tid = threadIdx.x, nf = 1u << fb, fmask = nf - 1u, rmask = (1u << rb) - 1u;
    if (tid == 0) {
        uint32_t bb = 0, qq = 0;
        sh_ok = fine_item(blockIdx.x, istarts, NCB, bb, qq) ? 1u : 0u;
        sh_bin = bb;
        sh_q0 = qq;
    }
    if (tid < nf) cnt[tid] = 0;
    __syncthreads();
    if (!sh_ok) return;
    uint32_t bin = sh_bin, q0 = sh_q0;
    uint32_t total = cstarts[bin + 1] - cstarts[bin];
    uint32_t count = total - q0 < FINE_SLICE ? total - q0 : FINE_SLICE;
    const uint4 *src = reinterpret_cast<const uint4 *>(tmp + tstarts[bin] + q0);
    const uint32_t T = 1024, quads = (count + 3) / 4;
    // where every fine key's run goes: loaded now (latency under the counting pass), kept in LDS for the copy loop, which used
    // to wait for two dependent global loads per key
    uint32_t dst_pre = tid < nf ? cstarts[bin] + fbase[(size_t)bin * nf + tid] + slicecnt[(size_t)blockIdx.x * nf + tid] : 0u;
    uint4 v[FINE_SLICE / 4 / 1024];
#pragma unroll
    for (int u = 0; u < (int)(FINE_SLICE / 4 / 1024); u++) {
        uint32_t q = (uint32_t)u * T + tid;
        v[u] = q < quads ? src[q] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < (int)(FINE_SLICE / 4 / 1024); u++) {
        uint32_t q = (uint32_t)u * T + tid, e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * q + j < count) atomicAdd(&cnt[(e[j] >> rb) & fmask], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t f = 0; f < nf; f++) {
            lbase[f] = run;
            run += cnt[f];
            cnt[f] = 0;
        }
        lbase[nf] = run;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (int)(FINE_SLICE / 4 / 1024); u++) {
        uint32_t q = (uint32_t)u * T + tid, e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * q + j < count) {
                uint32_t f = (e[j] >> rb) & fmask;
                uint32_t ref = e[j] & rmask;
                // a point slice sorted on slice-local references (level << shift | point): the final list holds table rows again,
                // so the accumulate kernel is the same for every launch (decoding there cost it 3 %)
                if (local_shift) ref = (ref >> local_shift) * table_n + off + (ref & ((1u << local_shift) - 1u));
                buf[lbase[f] + atomicAdd(&cnt[f], 1u)] = (e[j] & 0x80000000u) | ref;
            }
    }
    __syncthreads();
    if (tid < nf) cnt[tid] = dst_pre;  // the cursors are done with
    __syncthreads();
    for (uint32_t f = tid >> 6; f < nf; f += T >> 6) {
        uint32_t a = lbase[f], b = lbase[f + 1];
        uint32_t dst = cnt[f];
        for (uint32_t j = a + (tid & 63); j < b; j += 64) sorted[dst + (j - a)] = buf[j];
    }
}

__global__ void __launch_bounds__(128) msm_fine_offsets_kernel(const uint32_t *istarts, int fb, uint32_t NK, uint32_t *slicecnt, uint32_t *fbase,
                                                               uint32_t *hist) {
    ZG_HIPRIO();
    __shared__ uint32_t sh[128];
    uint32_t bin = blockIdx.x, f = threadIdx.x, nf = 1u << fb;
    uint32_t i0 = istarts[bin], i1 = istarts[bin + 1], run = 0;
    if (f < nf)
        for (uint32_t it = i0; it < i1; it++) {
            uint32_t v = slicecnt[(size_t)it * nf + f];
            slicecnt[(size_t)it * nf + f] = run;
            run += v;
        }
    sh[f] = f < nf ? run : 0;
    __syncthreads();
    for (uint32_t o = 1; o < 128; o <<= 1) {
        uint32_t v = f >= o ? sh[f - o] : 0;
        __syncthreads();
        sh[f] += v;
        __syncthreads();
    }
    if (f < nf) {
        fbase[(size_t)bin * nf + f] = sh[f] - run;
        uint32_t key = (bin << fb) | f;
        if (key < NK) hist[key] = run;
    }
}

// per coarse bin: exclusive prefix over the blocks' counts, in place, and the bin's total. The layout is chist[blk][bin]: a
// 1024-thread workgroup takes 16 CONSECUTIVE bins (16 lanes along the bin index: every access is a 64-byte row segment) and
// splits the blocks into 64 contiguous slices; the slices' sums meet in LDS. (One workgroup per bin walking a column with an
// 8 KiB stride cost 100 us at 2^22 points — 4 M uncoalesced 4-byte accesses; 64 bins per workgroup left only 32 workgroups.)
__global__ void __launch_bounds__(1024) msm_colscan_bins_kernel(uint32_t *chist, uint32_t nblk, uint32_t NCB, uint32_t *total) {
    ZG_HIPRIO();
    __shared__ uint32_t sh[64][16];
    const uint32_t lane = threadIdx.x & 15, slice = threadIdx.x >> 4, bin = blockIdx.x * 16 + lane;
    const uint32_t per = (nblk + 63) / 64, a = slice * per < nblk ? slice * per : nblk, b = a + per < nblk ? a + per : nblk;
    uint32_t s = 0;
    if (bin < NCB)
        for (uint32_t k = a; k < b; k++) s += chist[(size_t)k * NCB + bin];
    sh[slice][lane] = s;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t q = 0; q < slice; q++) run += sh[q][lane];
    if (bin < NCB) {
        for (uint32_t k = a; k < b; k++) {
            uint32_t v = chist[(size_t)k * NCB + bin];
            chist[(size_t)k * NCB + bin] = run;
            run += v;
        }
        if (slice == 63) total[bin] = run;
    }
}

ZG_DEV XYZZ xyzz_shfl_down(const XYZZ &v, int delta) {
    XYZZ r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r.x.l[i] = __shfl_down(v.x.l[i], delta, 64);
        r.y.l[i] = __shfl_down(v.y.l[i], delta, 64);
        r.zz.l[i] = __shfl_down(v.zz.l[i], delta, 64);
        r.zzz.l[i] = __shfl_down(v.zzz.l[i], delta, 64);
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// Skew-robust scheduling of the bucket accumulation — the reference's inner loop buckets[idx] = buckets[idx].addAffine(base)
// (msm/mod.zig:406-418). A fixed number of lanes per bucket is perfectly balanced for uniform scalars and pathological for real
// witness columns (a 0/1 column puts half of all points into ONE bucket: 0.4-0.9 s on skewed vectors). Here the sorted reference
// list is cut into NT equal chunks instead, one per thread, whatever the bucket sizes; a thread emits one partial sum per bucket run it
// crosses, at slot  chunk + (number of non-empty buckets before the run's bucket)  — unique and, for one
// bucket, contiguous. Buckets with few partials are finished by one thread each; "heavy" buckets
// (more than 8 partials) go through two block-level tree stages.
struct MsmState {
    uint32_t nheavy;  // buckets with more than 8*GS and at most HUGE_PARTIALS partials (queued by msm_bucket_combine)
    uint32_t nhuge;   // buckets with more than HUGE_PARTIALS partials (queued by msm_bucket_combine)
    uint32_t pad[2];
    // followed by one arrival counter per huge bucket (index = position in the huge list): see msm_heavy_kernel
};
static constexpr uint32_t HUGE_PARTIALS = 2048;
static constexpr uint32_t HEAVY_BLOCK_ITEMS = 2048;
// words of a launch set's state: the header and one arrival counter per possible huge bucket (each owns > 2048 partial slots)
static uint32_t state_words(uint32_t NT, uint32_t NK) { return 4 + (NT + NK) / HUGE_PARTIALS + 1; }

ZG_DEV uint32_t chunk_len(uint32_t total, uint32_t NT) {
    uint32_t C = (total + NT - 1) / NT;
    return C ? C : 1;
}

// QUAD = true: one chunk per quad of lanes, every mixed add by xyzz29_madd4 — for launch sets too short to fill the GPU, where
// the kernel is a latency chain of a few adds per chunk rather than a throughput problem (4 * NT lanes are launched).
#define ZG_ROW_MASK 0x7FFFFFFFu  // a sorted entry: sign << 31 | table row
#ifdef ZG_EXP_ACC_WAVES  // experiment: force the register budget of N waves per SIMD (tools/build_variant.sh)
#define ZG_ACC_ATTR __attribute__((amdgpu_waves_per_eu(ZG_EXP_ACC_WAVES, ZG_EXP_ACC_WAVES)))
#else
// two waves per SIMD whatever the register count (156 since the exceptional cases left the addition's path): three were measured
// slower for this kernel (docs/design/04_kernels.md), and the launch geometry is sized for two
#define ZG_ACC_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
// A table row as it is gathered: x then y, 256-bit words each (packed lazy form), four 16-byte loads
struct Row29 {
    uint4 w[4];
};
ZG_DEV Row29 row29_load(const char *p) {
    Row29 r;
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 4; i++) r.w[i] = q[i];
    return r;
}
ZG_DEV void row29_unpack(const Row29 &r, F29 &px, F29 &py) {
    const u32 x[8] = {r.w[0].x, r.w[0].y, r.w[0].z, r.w[0].w, r.w[1].x, r.w[1].y, r.w[1].z, r.w[1].w};
    const u32 y[8] = {r.w[2].x, r.w[2].y, r.w[2].z, r.w[2].w, r.w[3].x, r.w[3].y, r.w[3].z, r.w[3].w};
    px = f29_unpack(x);
    py = f29_unpack(y);
    // the limbs exist from here on: left to itself the compiler sinks the unpacking below the next row's loads, which then need a
    // second set of row registers and a copy
#pragma unroll
    for (int i = 0; i < 9; i++) {
        asm volatile("" : "+v"(px.l[i]));
        asm volatile("" : "+v"(py.l[i]));
    }
}

// nzend[r] = end of the r-th non-empty bucket's run in the sorted list (msm_scan_b_kernel), so the next run's end is one load at an
// address known a run ahead and is requested a run ahead (reading nzlist[r] and then starts[.. + 1] inside the loop was two dependent
// loads behind a full wait that also drained the row prefetch).
template <bool QUAD>
__global__ void __launch_bounds__(256) ZG_ACC_ATTR msm_accumulate_chunk_kernel(const uint32_t *sorted, const uint32_t *starts, const uint32_t *nzrank,
                                                                   const uint32_t *nzend, const char *table, uint32_t NK, uint32_t NT,
                                                                   char *part) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, q = 0;
    if (QUAD) {
        q = i & 3;
        i >>= 2;
    }
    uint32_t total = starts[NK];
    uint32_t C = chunk_len(total, NT);
    uint64_t a64 = (uint64_t)i * C;
    if (i >= NT || a64 >= total) return;
    uint32_t a = (uint32_t)a64, b = a + C < total ? a + C : total;
    // bucket of entry a: starts[k] <= a < starts[k+1]
    uint32_t lo = 0, hi = NK;  // invariant: starts[lo] <= a < starts[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= a) lo = mid; else hi = mid;
    }
    uint32_t r = nzrank[lo], kend = starts[lo + 1];  // r-th non-empty bucket (it is bucket lo), and where its run ends
    uint32_t knext = nzend[r + 1];  // the end of the run after it (the slot past the last run is allocated and never used)
    XYZZ29 acc;
    bool acc_inf = true;
    // Two loads feed an addition: the reference sorted[p] and the table row it names. Both run ahead of the arithmetic — the row
    // of entry p+1 is in flight during addition p, and the reference of entry p+2 is loaded then too, so
    // the row gather of the next iteration never waits for its index (measured: accumulate 1.18 -> 1.13-1.14 ms at 2^20 points,
    // 784 -> 791-794 MSM/s; the sorted list is read at a stride of one chunk per lane, i.e. every lane pulls its own cache line).
    // TWO rows in flight (214 registers instead of 200) were measured slower: 759 MSM/s.
    // The row has ONE set of 16 registers: an iteration unpacks it into the limbs of (px, py) and only then requests the next row
    // into the same registers, so nothing is copied at the loop's end (a second buffer cost 16 moves per addition).
    uint32_t e = sorted[a];
    Row29 row = row29_load(table + 64 * (size_t)(e & ZG_ROW_MASK));  // packed lazy-form row
    uint32_t rneg = e >> 31;
    uint32_t e1 = a + 1 < b ? sorted[a + 1] : 0u;
    for (uint32_t p = a; p < b; p++) {
        F29 px, py;
        row29_unpack(row, px, py);
        const uint32_t neg = 0u - rneg;  // 0 or ~0: subtract the point
        if (p + 1 < b) {  // prefetch the next row under the current add
            uint32_t e2 = e1;
            if (p + 2 < b) e1 = sorted[p + 2];
            row = row29_load(table + 64 * (size_t)(e2 & ZG_ROW_MASK));
            rneg = e2 >> 31;
        }
        // The order of the three cases matters to the register allocator. A divergent if / else runs one side after the other, so a
        // value the later side reads is live across everything the earlier side writes. The run's end reads the accumulator and
        // comes first; the addition reads and replaces it; the run's start and the exceptional cases read nothing of it and come
        // last. The new sums can then take the registers of the old ones, and the loop's end copies no accumulator limb (36 moves
        // per addition before).
        if (__builtin_expect(p == kend, 0)) {  // the run of bucket k ended inside this chunk: emit its partial, move on
            if (q == 0) xyzz29_store(part + 144 * (size_t)(i + r), acc_inf ? xyzz29_identity() : acc);
            acc_inf = true;
            r++;  // next non-empty bucket (p < total, so it exists); empty buckets are never walked
            // kend = knext, as a move the compiler cannot push behind the load below: the load then lands in knext's own register and
            // nothing on this path waits for it (left to itself the compiler loads into a scratch register and copies, behind a full wait)
            asm volatile("v_mov_b32 %0, %1" : "=v"(kend) : "v"(knext));
            knext = nzend[r + 1];
        }
        uint32_t exc = 0;  // the addition met acc == +-P (xyzz29_madd_nz): finished below, from the point alone
        if (QUAD) {
            if (neg) py = f29_neg2(py);
            xyzz29_madd4(acc, acc_inf, px, py, q);
        } else if (__builtin_expect(acc_inf, 0)) {
            // a run starts (the chunk's first entry, the entry after a run's end, or after a sum that came out as infinity): the
            // sign applied to y and the ONE limbs stay inside this branch (it follows the addition, so nothing of it is hoisted)
            xyzz29_start(acc, px, neg ? f29_neg2(py) : py);
            acc_inf = false;
        } else {
            exc = xyzz29_madd_nz(acc, px, py, neg);  // the sign is folded into R = +-S2 - Y1, not a negation of y under a branch
        }
        if (__builtin_expect(exc != 0, 0)) xyzz29_madd_except(acc, acc_inf, px, py, neg, exc);
    }
    if (q == 0) xyzz29_store(part + 144 * (size_t)(i + r), acc_inf ? xyzz29_identity() : acc);
}

// GS adjacent QUADS of lanes per bucket (4*GS | 64, GS chosen from the expected partials per bucket) sum its partials: strided
// serial adds, then a segmented shuffle tree, every addition by a quad (g1_29x4.hip.h); buckets with more than 8*GS partials
// are queued as heavy
__global__ void __launch_bounds__(64) msm_bucket_combine_kernel(const char *part, const uint32_t *starts, const uint32_t *nzrank, uint32_t NK,
                                                                uint32_t NT, int GS, char *buckets, uint32_t *heavy_list, MsmState *st) {
    ZG_HIPRIO();
    uint32_t t = (blockIdx.x * 64 + threadIdx.x) >> 2, q = threadIdx.x & 3;
    uint32_t k = t / (uint32_t)GS, g = t % (uint32_t)GS;
    XYZZ29 acc = xyzz29_identity();
    bool light = false;
    if (k < NK) {
        uint32_t C = chunk_len(starts[NK], NT);
        uint32_t s0 = starts[k], s1 = starts[k + 1];
        if (s1 == s0) {
            light = true;  // empty bucket: identity
        } else {
            uint32_t q0 = s0 / C, q1 = (s1 - 1) / C, cnt = q1 - q0 + 1, base = q0 + nzrank[k];
            if (cnt > 8u * (uint32_t)GS) {  // heavy: a wave each; huge (a 0/1 witness column's bucket): block trees — msm_heavy_kernel
                if (g == 0 && q == 0) {
                    if (cnt > HUGE_PARTIALS) heavy_list[NK + atomicAdd(&st->nhuge, 1u)] = k;
                    else heavy_list[atomicAdd(&st->nheavy, 1u)] = k;
                }
            } else {
                light = true;
                if (g < cnt) acc = xyzz29_load(part + 144 * (size_t)(base + g));  // the first partial is taken as it is
                // the next partial is loaded under the current addition (the chain used to pay a memory latency per partial)
                uint32_t j = g + (uint32_t)GS;
                XYZZ29 nxt = j < cnt ? xyzz29_load(part + 144 * (size_t)(base + j)) : xyzz29_identity();
                while (j < cnt) {
                    XYZZ29 cur = nxt;
                    j += (uint32_t)GS;
                    if (j < cnt) nxt = xyzz29_load(part + 144 * (size_t)(base + j));
                    acc = xyzz29_add4(acc, cur, q);
                }
            }
        }
    }
    for (int d = 1; d < GS; d <<= 1) {
        XYZZ29 o = xyzz29_shfl_down(acc, 4 * d);  // the same lane of the quad d quads further
        if ((g & (uint32_t)(2 * d - 1)) == 0) acc = xyzz29_add4(acc, o, q);
    }
    if (light && g == 0 && q == 0) xyzz29_store(buckets + 144 * (size_t)k, acc);
}

// The LANE form of the same pass (MsmPlan::tail): ONE lane per bucket sums its partials with single-lane additions — a quarter of the
// lanes a quad form occupies for about twice the instructions per lane, and 64 buckets instead of 16 share the rounds of a wave.
// The loop runs while any lane of the wave has a partial left, the addition under the lane's own predicate; buckets with more than
// 8 partials are queued as heavy exactly as the quad form does with GS = 1.
__global__ void __launch_bounds__(64) msm_bucket_combine_lane_kernel(const char *part, const uint32_t *starts, const uint32_t *nzrank, uint32_t NK,
                                                                     uint32_t NT, char *buckets, uint32_t *heavy_list, MsmState *st) {
    ZG_HIPRIO();
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    uint32_t cnt = 0, base = 0;  // the partials this lane sums: part[base .. base + cnt)
    bool light = false;
    if (k < NK) {
        const uint32_t C = chunk_len(starts[NK], NT);
        const uint32_t s0 = starts[k], s1 = starts[k + 1];
        if (s1 == s0) {
            light = true;  // empty bucket: identity
        } else {
            const uint32_t q0 = s0 / C, q1 = (s1 - 1) / C, c = q1 - q0 + 1;
            if (c > 8u) {  // heavy / huge: msm_heavy_kernel
                if (c > HUGE_PARTIALS) heavy_list[NK + atomicAdd(&st->nhuge, 1u)] = k;
                else heavy_list[atomicAdd(&st->nheavy, 1u)] = k;
            } else {
                light = true;
                cnt = c;
                base = q0 + nzrank[k];
            }
        }
    }
    XYZZ29 acc = cnt ? xyzz29_load(part + 144 * (size_t)base) : xyzz29_identity();  // the first partial is taken as it is
    XYZZ29 nxt = cnt > 1 ? xyzz29_load(part + 144 * (size_t)(base + 1)) : xyzz29_identity();
    uint32_t j = 1;
    while (__any(j < cnt)) {
        const XYZZ29 cur = nxt;
        const bool on = j < cnt;
        j++;
        if (j < cnt) nxt = xyzz29_load(part + 144 * (size_t)(base + j));  // the next partial is loaded under the current addition
        if (on) acc = xyzz29_add(acc, cur);
    }
    if (light) xyzz29_store(buckets + 144 * (size_t)k, acc);
}

// block-wide sum of lazy XYZZ points through LDS (256 threads x 144 B); result returned to every thread. After the first level
// (128 additions, one lane each) every addition of a level is done by a quad of lanes (g1_29x4.hip.h): the chain is one
// single-lane addition plus seven quad additions instead of eight single-lane ones.
__device__ __forceinline__ XYZZ29 block_sum_xyzz29(const XYZZ29 &acc, uint4 *sh) {
    uint32_t tid = threadIdx.x;
    xyzz29_store(&sh[tid * 9], acc);
    __syncthreads();
    if (tid < 128) {
        XYZZ29 x = xyzz29_load(&sh[tid * 9]), y = xyzz29_load(&sh[(tid + 128) * 9]);
        xyzz29_store(&sh[tid * 9], xyzz29_add(x, y));
    }
    __syncthreads();
    uint32_t g = tid >> 2, q = tid & 3;
    for (uint32_t o = 64; o > 0; o >>= 1) {
        if (g < o) {  // slot g is read and written by quad g only, slot g + o read by quad g only: no hazard inside a level
            XYZZ29 x = xyzz29_load(&sh[g * 9]), y = xyzz29_load(&sh[(g + o) * 9]);
            XYZZ29 r = xyzz29_add4(x, y, q);
            if (q == 0) xyzz29_store(&sh[g * 9], r);
        }
        __syncthreads();
    }
    return xyzz29_load(&sh[0]);
}

// The same sum over ONE wave (64 partial sums, 9 KiB of LDS): one single-lane addition, then five levels of quad additions. For launches
// with many rows (several bucket sets: a batch, a handle without a table) — see msm_rowcol_wave_kernel.
__device__ __forceinline__ XYZZ29 wave_sum_xyzz29(const XYZZ29 &acc, uint4 *sh) {
    const uint32_t tid = threadIdx.x;  // 64 threads
    xyzz29_store(&sh[tid * 9], acc);
    __syncthreads();
    if (tid < 32) {
        XYZZ29 x = xyzz29_load(&sh[tid * 9]), y = xyzz29_load(&sh[(tid + 32) * 9]);
        xyzz29_store(&sh[tid * 9], xyzz29_add(x, y));
    }
    __syncthreads();
    const uint32_t g = tid >> 2, q = tid & 3;
    for (uint32_t o = 16; o > 0; o >>= 1) {
        if (g < o) {
            XYZZ29 x = xyzz29_load(&sh[g * 9]), y = xyzz29_load(&sh[(g + o) * 9]);
            XYZZ29 r = xyzz29_add4(x, y, q);
            if (q == 0) xyzz29_store(&sh[g * 9], r);
        }
        __syncthreads();
    }
    return xyzz29_load(&sh[0]);
}

// Heavy buckets in ONE launch (uniform scalars have none: the kernel then returns at once — it used to be three launches of ~5 us
// each). Part 1, one wave per heavy bucket (more than 8*GS, at most HUGE_PARTIALS partials; typical source: the top window of a
// c-bit decomposition covers only a few bits, so its digits pile into a small set of buckets): strided serial sums (<= 32 per lane)
// and a shuffle tree. Part 2, huge buckets (a 0/1 column: one bucket holds everything): block b owns the partial slots
// [2048 b, 2048 (b+1)) and tree-sums every run of a huge bucket inside into part2[b + nzrank[k]] (stage A); the block that
// arrives LAST at the bucket's counter (device-scope acq_rel, as the sumcheck rounds end) sums the bucket's stage-A partials
// (stage B). The counters are cleared by msm_scan_b_kernel.
__global__ void __launch_bounds__(256) msm_heavy_kernel(const char *part, const uint32_t *starts, const uint32_t *nzrank, const uint32_t *nzlist,
                                                        uint32_t NK, uint32_t NT, const uint32_t *heavy_list, MsmState *st, char *part2,
                                                        char *buckets) {
    ZG_HIPRIO();
    __shared__ uint4 sh[256 * 9];
    __shared__ uint32_t sh_last;
    const uint32_t nheavy = st->nheavy, nhuge = st->nhuge;
    if (nheavy == 0 && nhuge == 0) return;
    const uint32_t C = chunk_len(starts[NK], NT), tid = threadIdx.x;
    {
        const uint32_t lane = tid & 63;
        for (uint32_t h = blockIdx.x * 4 + (tid >> 6); h < nheavy; h += gridDim.x * 4) {
            uint32_t k = heavy_list[h];
            uint32_t s0 = starts[k], s1 = starts[k + 1];
            uint32_t q0 = s0 / C, q1 = (s1 - 1) / C, cnt = q1 - q0 + 1, base = q0 + nzrank[k];
            XYZZ29 acc = xyzz29_identity();
            for (uint32_t j = lane; j < cnt; j += 64) acc = xyzz29_add(acc, xyzz29_load(part + 144 * (size_t)(base + j)));
            for (int d = 1; d < 64; d <<= 1) {
                XYZZ29 o = xyzz29_shfl_down(acc, d);
                if ((lane & (uint32_t)(2 * d - 1)) == 0) acc = xyzz29_add(acc, o);
            }
            if (lane == 0) xyzz29_store(buckets + 144 * (size_t)k, acc);
        }
    }
    if (nhuge == 0) return;
    const uint32_t *huge_list = heavy_list + NK;
    uint32_t *arrive = reinterpret_cast<uint32_t *>(st) + 4;
    uint32_t NZ = nzrank[NK];  // non-empty buckets; the r-th one, k = nzlist[r], owns slots [starts[k]/C + r, ...)
    uint32_t lo_slot = blockIdx.x * HEAVY_BLOCK_ITEMS, hi_slot = lo_slot + HEAVY_BLOCK_ITEMS;
    if (lo_slot >= NT + NK) return;
    uint32_t lo = 0, hi = NZ;  // last r whose first slot is <= lo_slot (first slots increase strictly with r)
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (starts[nzlist[mid]] / C + mid <= lo_slot) lo = mid; else hi = mid;
    }
    for (uint32_t r = lo; r < NZ; r++) {
        uint32_t k = nzlist[r];
        uint32_t s0 = starts[k], s1 = starts[k + 1];
        uint32_t q0 = s0 / C, q1 = (s1 - 1) / C, cnt = q1 - q0 + 1, base = q0 + r;
        if (base >= hi_slot) break;
        if (cnt <= HUGE_PARTIALS || base + cnt <= lo_slot) continue;
        uint32_t r0 = base > lo_slot ? base : lo_slot, r1 = base + cnt < hi_slot ? base + cnt : hi_slot;
        XYZZ29 acc = xyzz29_identity();
        for (uint32_t j = r0 + tid; j < r1; j += 256) acc = xyzz29_add(acc, xyzz29_load(part + 144 * (size_t)j));
        XYZZ29 res = block_sum_xyzz29(acc, sh);
        const uint32_t b0 = base / HEAVY_BLOCK_ITEMS, b1 = (base + cnt - 1) / HEAVY_BLOCK_ITEMS;
        if (tid == 0) {
            xyzz29_store(part2 + 144 * (size_t)(blockIdx.x + r), res);  // plain store: the arrival's release publishes it
            uint32_t h = 0;
            while (h < nhuge && huge_list[h] != k) h++;
            uint32_t arrived = __hip_atomic_fetch_add(&arrive[h], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the acquire's invalidate has completed before the barrier releases the other waves' loads
            sh_last = arrived == b1 - b0 ? 1u : 0u;
        }
        __syncthreads();
        if (sh_last) {  // stage B: this block saw every other block of the bucket arrive
            XYZZ29 a2 = xyzz29_identity();
            for (uint32_t bb = b0 + tid; bb <= b1; bb += 256) a2 = xyzz29_add(a2, xyzz29_load(part2 + 144 * (size_t)(bb + r)));
            __syncthreads();  // sh is reused
            XYZZ29 tot = block_sum_xyzz29(a2, sh);
            if (tid == 0) xyzz29_store(buckets + 144 * (size_t)k, tot);
        }
        __syncthreads();
    }
}

// Bucket reduction, step 1. The reference computes sum_k k*B_k with a serial running sum
// (msm/mod.zig:423-432). Here  sum_k k*B_k = sum_b 2^b * T_b  with  T_b = sum_{k: bit b of k set} B_k;
// block (x, b, g) tree-sums a slice of T_b of group g. Bucket index idx holds digit magnitude k = idx+1.
__global__ void __launch_bounds__(256) msm_bitsum_kernel(const char *buckets, uint32_t NB, int c, char *out) {
    ZG_HIPRIO();
    __shared__ uint4 sh[256 * 9];
    uint32_t b = blockIdx.y, g = blockIdx.z, PB = gridDim.x;
    uint32_t total = (b == (uint32_t)(c - 1)) ? 1u : NB / 2;
    XYZZ29 acc = xyzz29_identity();
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < total; j += PB * 256) {
        uint32_t k = (b == (uint32_t)(c - 1)) ? NB : ((((j >> b) << 1) | 1u) << b) | (j & ((1u << b) - 1u));
        acc = xyzz29_add(acc, xyzz29_load(buckets + 144 * ((size_t)g * NB + (k - 1))));
    }
    XYZZ29 r = block_sum_xyzz29(acc, sh);
    if (threadIdx.x == 0) xyzz29_store(out + 144 * (((size_t)g * c + b) * PB + blockIdx.x), r);
}

// Bucket reduction, step 1, two-dimensional form for wide windows (c >= 11). The bit sums above touch every bucket (c-1)/2 times
// on average: 2^(c-2) * (c-1) additions per group — for c = 16 a quarter of a million, 16 M VALU wave-instructions, a fixed cost
// that does not shrink with the number of points. Write a digit magnitude k < NB = 2^(c-1) as k = h * 2^lb + l: then
//     sum_k k * B_k = 2^lb * sum_h h * R_h + sum_l l * C_l,    R_h = sum_l B_(h,l),  C_l = sum_h B_(h,l),
// i.e. every bucket is added twice (one row sum, one column sum: 2^c additions), and the weighted sums run over 2^hb rows and
// 2^lb columns only. msm_rowcol_kernel: block x < 2^hb sums row x, block 2^hb + l sums column l (<= 256 elements each, one
// block tree). msm_bits2d_kernel then forms the same T_b the one-dimensional kernel produces — for b < lb from the columns whose
// index has bit b, for lb <= b < c-1 from the rows whose index has bit b - lb, T_(c-1) = B_NB — so msm_final_kernel is unchanged.
__global__ void __launch_bounds__(256) msm_rowcol_kernel(const char *buckets, uint32_t NB, int lb, int hb, char *rc) {
    ZG_HIPRIO();
    __shared__ uint4 sh[256 * 9];
    const uint32_t x = blockIdx.x, g = blockIdx.y, nrow = 1u << hb, ncol = 1u << lb, t = threadIdx.x;
    XYZZ29 acc = xyzz29_identity();
    // (rows / columns of more than 256 elements — windows of 18 bits and more — take several elements per thread)
    const uint32_t len = x < nrow ? ncol : nrow;
    for (uint32_t e = t; e < len; e += 256) {
        const uint32_t k = x < nrow ? ((x << lb) | e) : ((e << lb) | (x - nrow));  // digit magnitude of the element; 0 = none
        if (k != 0) {
            XYZZ29 v = xyzz29_load(buckets + 144 * ((size_t)g * NB + (k - 1)));
            acc = e < 256 ? v : xyzz29_add(acc, v);
        }
    }
    XYZZ29 r = block_sum_xyzz29(acc, sh);
    if (t == 0) xyzz29_store(rc + 144 * ((size_t)g * (nrow + ncol) + x), r);
}
// The same sums by ONE wave per row / column: a lane adds up to four of the 256 elements itself, then the wave's tree. A 256-thread
// workgroup per row keeps three quarters of its lanes idle from the second tree level on and needs 36 KiB of LDS: with several bucket
// sets in one launch (K rows of a batch, the G window groups of a handle without a table: 2560 ... 8704 workgroups) the launch ran in
// waves of workgroups — 230 us for the five long levels of HyperKZG.open, 240 us for ONE table-less MSM. One wave per row is a few
// additions longer alone (57 -> ~70 us) and several times shorter there, so it is taken from three bucket sets on.
__global__ void __launch_bounds__(64) msm_rowcol_wave_kernel(const char *buckets, uint32_t NB, int lb, int hb, char *rc) {
    ZG_HIPRIO();
    __shared__ uint4 sh[64 * 9];
    const uint32_t x = blockIdx.x, g = blockIdx.y, nrow = 1u << hb, ncol = 1u << lb, t = threadIdx.x;
    XYZZ29 acc = xyzz29_identity();
    const uint32_t len = x < nrow ? ncol : nrow;
    bool first = true;
    for (uint32_t e = t; e < len; e += 64) {
        const uint32_t k = x < nrow ? ((x << lb) | e) : ((e << lb) | (x - nrow));  // digit magnitude of the element; 0 = none
        if (k != 0) {
            XYZZ29 v = xyzz29_load(buckets + 144 * ((size_t)g * NB + (k - 1)));
            acc = first ? v : xyzz29_add(acc, v);
            first = false;
        }
    }
    XYZZ29 r = wave_sum_xyzz29(acc, sh);
    if (t == 0) xyzz29_store(rc + 144 * ((size_t)g * (nrow + ncol) + x), r);
}
static void launch_rowcol(hipStream_t st, const char *buckets, uint32_t NB, int lb, int hb, int sets, char *rc) {
    const int wave_from = env_int("ZG_MSM_ROWCOL_WAVE_FROM", 3);  // bucket sets from which one wave sums a row (0: never)
    if (wave_from > 0 && sets >= wave_from)
        hipLaunchKernelGGL(msm_rowcol_wave_kernel, dim3((1u << hb) + (1u << lb), sets), dim3(64), 0, st, buckets, NB, lb, hb, rc);
    else
        hipLaunchKernelGGL(msm_rowcol_kernel, dim3((1u << hb) + (1u << lb), sets), dim3(256), 0, st, buckets, NB, lb, hb, rc);
}

// The LANE form of the row / column sums (MsmPlan::tail; one bucket set, rows and columns of 64 or 256 buckets): a workgroup sums four
// rows or four columns in radix-4 stages — every lane of the first stage adds four consecutive elements itself, so no lane of the
// stages that hold most of the additions is idle; the last two stages (16 and 4 sums) are done by quads of lanes. msm_lane_map.h is
// the index map. Four lines of 256 buckets cost four waves and then one wave of three lane additions and two waves of three quad
// additions, against four block trees of 256 threads (2^20 points: 13.5 M -> 7.6 M wave instructions per MSM); the chain is six lane
// and six quad additions against one and seven (55 -> 75 us alone). The sums land in the rc slots msm_rowcol_kernel writes.
__global__ void __launch_bounds__(256) msm_rowcol_lane_kernel(const char *buckets, uint32_t NB, int lb, int hb, char *rc) {
    namespace lm = lane_map;
    ZG_HIPRIO();
    __shared__ uint4 sh[lm::SLOTS * 9];
    const uint32_t t = threadIdx.x, line0 = blockIdx.x * lm::LINES, g = blockIdx.y, q = t & 3;
    const int m = lm::line_bits(lb, hb, line0), S = lm::stages(m);
    const char *bg = buckets + 144 * (size_t)g * NB;
    if (t < lm::units(m, 1)) {
        const uint32_t line = line0 + lm::first_line(m, t), e0 = lm::first_element(m, t);
        auto element = [&](uint32_t i) {
            const uint32_t k = lm::element(lb, hb, line, e0 + i);  // 0: the first element of row 0 and of column 0 has no bucket
            return k != 0 ? xyzz29_load(bg + 144 * (size_t)(k - 1)) : xyzz29_identity();
        };
        XYZZ29 acc = element(0), nxt = element(1);
#pragma unroll 1
        for (uint32_t i = 2; i <= 4; i++) {
            const XYZZ29 cur = nxt;
            if (i < 4) nxt = element(i);  // loaded under the current addition
            acc = xyzz29_add(acc, cur);
        }
        xyzz29_store(&sh[lm::out_slot(1, t) * 9], acc);
    }
    __syncthreads();
    for (int s = 2; s <= S; s++) {
        const bool quad = lm::quad_stage(m, s);
        const uint32_t u = quad ? t >> 2 : t;
        if (u < lm::units(m, s)) {
            XYZZ29 acc = xyzz29_load(&sh[lm::in_slot(s, u, 0) * 9]);
#pragma unroll 1
            for (uint32_t i = 1; i < 4; i++) {
                const XYZZ29 v = xyzz29_load(&sh[lm::in_slot(s, u, i) * 9]);
                acc = quad ? xyzz29_add4(acc, v, q) : xyzz29_add(acc, v);
            }
            if (s == S) {  // unit u is line u of the workgroup
                if (q == 0) xyzz29_store(rc + 144 * ((size_t)g * ((1u << hb) + (1u << lb)) + line0 + u), acc);
            } else if (!quad || q == 0) {
                xyzz29_store(&sh[lm::out_slot(s, u) * 9], acc);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) msm_bits2d_kernel(const char *buckets, const char *rc, uint32_t NB, int c, int lb, int hb, char *out) {
    ZG_HIPRIO();
    __shared__ uint4 sh[256 * 9];
    const uint32_t b = blockIdx.x, g = blockIdx.y, nrow = 1u << hb, ncol = 1u << lb, t = threadIdx.x;
    const char *rcg = rc + 144 * (size_t)g * (nrow + ncol);
    XYZZ29 acc = xyzz29_identity();
    if (b == (uint32_t)(c - 1)) {
        if (t == 0) acc = xyzz29_load(buckets + 144 * ((size_t)g * NB + (NB - 1)));
    } else if (b < (uint32_t)lb) {
        for (uint32_t e = t; e < ncol; e += 256)
            if ((e >> b) & 1u) acc = xyzz29_add(acc, xyzz29_load(rcg + 144 * (size_t)(nrow + e)));
    } else {
        for (uint32_t e = t; e < nrow; e += 256)
            if ((e >> (b - (uint32_t)lb)) & 1u) acc = xyzz29_add(acc, xyzz29_load(rcg + 144 * (size_t)e));
    }
    XYZZ29 r = block_sum_xyzz29(acc, sh);
    if (t == 0) xyzz29_store(out + 144 * ((size_t)g * c + b), r);
}

ZG_DEV void write_result(const XYZZ &acc, int mode, uint64_t *out_rec, uint8_t *out_inf) {
    Affine r;
    bool inf = xyzz_to_affine(acc, r);
    if (mode == 0) {  // affine xy[8] + inf flag (AffinePoint, msm/mod.zig:15-30)
        affine_store(out_rec, r);
        *out_inf = inf ? 1 : 0;
    } else {  // ParallelMSM's threadWorker record fromAffine(result) = (x,y,1) / (1,1,0) (msm/mod.zig:663-664)
        Fp one = Fp::one();
        if (inf) {
            fe_store(out_rec, one); fe_store(out_rec + 4, one); fe_store(out_rec + 8, Fp::zero());
        } else {
            fe_store(out_rec, r.x); fe_store(out_rec + 4, r.y); fe_store(out_rec + 8, one);
        }
    }
}

// mode 2: a per-GPU partial that is only ever fed to the combine step. Any Jacobian representative of the shard's
// sum works there, so the inversion (the longest single piece of a small MSM's tail) is skipped:
// (X*ZZ, Y*ZZZ, ZZ) has the same affine image as the XYZZ point; identity = (1,1,0).
ZG_DEV void write_partial_unnormalised(const XYZZ &acc, uint64_t *out_rec) {
    Fp X, Y, Z;
    xyzz_to_jacobian(acc, X, Y, Z);
    fe_store(out_rec, X); fe_store(out_rec + 4, Y); fe_store(out_rec + 8, Z);
}

// Bucket reduction, step 2 (block g, 512 threads = 128 quads): the c x PB partial sums of group g go to LDS; a tree over the
// partials of each bit, then quad b doubles T_b b times, then a tree over the bits  ->  R_g = sum_k k*B_k of group g.
// Every point operation is done by a quad of lanes (g1_29x4.hip.h). With a single group (full precompute) thread 0 goes
// straight on to toAffine (msm/mod.zig:178-189).
__global__ void __launch_bounds__(512) msm_final_kernel(const char *bits, int c, int PB, int G, char *rg, int mode, uint64_t *out_rec,
                                                        uint8_t *out_inf, uint32_t rec_stride, uint32_t inf_stride) {
    ZG_HIPRIO();
    __shared__ uint4 pts[256 * 9];  // slot b * S + j, S = PB rounded up to a power of two: 256 / S bit rows (c <= 16 for S = 16, c <= 32 below)
    uint32_t tid = threadIdx.x, g = blockIdx.x, quad = tid >> 2, q = tid & 3;
    uint32_t S = 1;
    while (S < (uint32_t)PB) S <<= 1;
    if (tid < 256) {
        uint32_t b = tid / S, j = tid % S;
        XYZZ29 v = xyzz29_identity();
        if (b < (uint32_t)c && j < (uint32_t)PB) v = xyzz29_load(bits + 144 * (((size_t)g * c + b) * PB + j));
        xyzz29_store(&pts[tid * 9], v);
    }
    __syncthreads();
    for (uint32_t d = 1; d < S; d <<= 1) {   // per bit: partial j += partial j + d, for j a multiple of 2d
        uint32_t per_bit = S / (2 * d);      // additions per bit at this level; (256 / S) * per_bit <= 128 quads
        if (quad < (256 / S) * per_bit) {
            uint32_t b = quad / per_bit, j = (quad % per_bit) * 2 * d;
            XYZZ29 x = xyzz29_load(&pts[(b * S + j) * 9]), y = xyzz29_load(&pts[(b * S + j + d) * 9]);
            XYZZ29 r = xyzz29_add4(x, y, q);
            if (q == 0) xyzz29_store(&pts[(b * S + j) * 9], r);
        }
        __syncthreads();
    }
    if (quad < (uint32_t)c) {  // 2^b * T_b
        XYZZ29 v = xyzz29_load(&pts[(quad * S) * 9]);
        for (uint32_t i = 0; i < quad; i++) v = xyzz29_dbl4(v, q);
        if (q == 0) xyzz29_store(&pts[(quad * S) * 9], v);
    }
    __syncthreads();
    uint32_t top = 1;  // bit rows c .. top-1 hold the identity (top <= 256 / S)
    while (top < (uint32_t)c) top <<= 1;
    for (uint32_t o = top >> 1; o > 0; o >>= 1) {
        if (quad < o) {
            XYZZ29 x = xyzz29_load(&pts[(quad * S) * 9]), y = xyzz29_load(&pts[((quad + o) * S) * 9]);
            XYZZ29 r = xyzz29_add4(x, y, q);
            if (q == 0) xyzz29_store(&pts[(quad * S) * 9], r);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    XYZZ r = xyzz29_to_std_val(xyzz29_load(&pts[0]));  // canonical Montgomery-2^256 from here on
    if (G == 1) {  // block g is scalar vector g of a batched launch (g == 0 for a single MSM)
        out_rec += (size_t)rec_stride * g;
        out_inf += (size_t)inf_stride * g;
        if (mode == 2) write_partial_unnormalised(r, out_rec);
        else write_result(r, mode, out_rec, out_inf);
    } else {
        xyzz_store(rg + 128 * (size_t)g, r);
    }
}

// window combine for G > 1 (msm/mod.zig:393-398,434): Horner from the top group with c doublings per step
__global__ void msm_groups_kernel(const char *rg, int G, int c, int mode, uint64_t *out_rec, uint8_t *out_inf, uint32_t rec_stride,
                                  uint32_t inf_stride) {
    ZG_HIPRIO();
    rg += 128 * (size_t)G * blockIdx.x;  // one single-thread block per scalar vector
    out_rec += (size_t)rec_stride * blockIdx.x;
    out_inf += (size_t)inf_stride * blockIdx.x;
    // one quad of lanes per scalar vector (g1_29x4.hip.h): the (G-1)*c doublings are a serial chain
    uint32_t q = threadIdx.x & 3;
    XYZZ29 acc29 = xyzz29_from_std_val(xyzz_load(rg + 128 * (size_t)(G - 1)));
    for (int g = G - 2; g >= 0; g--) {
        for (int k = 0; k < c; k++) acc29 = xyzz29_dbl4(acc29, q);
        acc29 = xyzz29_add4(acc29, xyzz29_from_std_val(xyzz_load(rg + 128 * (size_t)g)), q);
    }
    if (threadIdx.x != 0) return;
    XYZZ acc = xyzz29_to_std_val(acc29);
    if (mode == 2) write_partial_unnormalised(acc, out_rec);
    else write_result(acc, mode, out_rec, out_inf);
}

__global__ void msm_identity_kernel(int mode, uint64_t *out_rec, uint8_t *out_inf) {
    if (mode == 0) {
        for (int i = 0; i < 8; i++) out_rec[i] = 0;
        *out_inf = 1;
    } else {
        Fp one = Fp::one();
        fe_store(out_rec, one); fe_store(out_rec + 4, one); fe_store(out_rec + 8, Fp::zero());
    }
}

// ParallelMSM combine (msm/mod.zig:647-652): serial add of k Jacobian partials + toAffine. Block j combines scalar vector j of
// a sharded batch: rank i's record for it sits at partials + i * rank_stride + 12 * j (u64 units); its result record goes to
// out_xy + j * rec_stride / out_inf + j * inf_stride.
__global__ void __launch_bounds__(64) msm_combine_kernel(const uint64_t *partials, uint32_t k, uint32_t rank_stride, uint64_t *out_xy,
                                                         uint8_t *out_inf, uint32_t rec_stride, uint32_t inf_stride, int mode = 0) {
    // one wave = 16 quads of lanes: quad i folds partials i, i+16, ... (Jacobian -> lazy XYZZ), then a shuffle tree over the
    // quads, every addition by a quad (g1_29x4.hip.h); the group sum does not depend on the association order, and the
    // affine result is canonical
    partials += 12 * (size_t)blockIdx.x;
    out_xy += (size_t)rec_stride * blockIdx.x;
    out_inf += (size_t)inf_stride * blockIdx.x;
    uint32_t lane = threadIdx.x, quad = lane >> 2, q = lane & 3;
    XYZZ29 acc = xyzz29_identity();
    for (uint32_t i = quad; i < k; i += 16) {
        const uint64_t *rec = partials + (size_t)rank_stride * i;
        Fp X = fe_load<FpParams>(rec), Y = fe_load<FpParams>(rec + 4), Z = fe_load<FpParams>(rec + 8);
        if (!Z.is_zero()) {
            XYZZ29 p;
            F29 z = f29_from_fp(Z);
            p.x = f29_from_fp(X); p.y = f29_from_fp(Y);
            p.zz = f29_sqr(z);
            p.zzz = f29_mul(p.zz, z);
            acc = xyzz29_add4(acc, p, q);
        }
    }
    for (int d = 1; d < 16; d <<= 1) {
        XYZZ29 o = xyzz29_shfl_down(acc, 4 * d);
        if ((quad & (uint32_t)(2 * d - 1)) == 0 && (uint32_t)d < k) acc = xyzz29_add4(acc, o, q);
    }
    if (lane != 0) return;
    XYZZ tot = xyzz29_to_std_val(acc);
    if (mode == 2) write_partial_unnormalised(tot, out_xy);  // the record modes of msm_final_kernel (a sliced MSM ends here instead)
    else write_result(tot, mode, out_xy, out_inf);
}

// ---- fixed-base batch scalar multiplication: HyperKZG.setup's loop powers[i] = scalarMul(g1, tau^i).toAffine()
// (src/poly/commitment/mod.zig:194-199; generateMockSRS, srs.zig:326-355) — every product has the SAME base. The reference's
// scalarMul is double-and-add (254 doublings + ~127 additions per output, msm/mod.zig:503-540); with one shared table
// T[w][d-1] = d * 2^(8w) * G (32 windows x 255 multiples, 510 KiB, L2-resident) an output is at most 32 mixed additions
// and one toAffine, no doubling at all.
// Window width by batch size: 8 bits (32 windows, 510 KiB of table, 8160 rows to build) up to 2^15 outputs, 10 bits (26 windows, 1.7 MB)
// up to 2^18, 11 bits (24 windows, 3.1 MB — still inside one XCD's L2) beyond: an output then costs 24 additions instead of 32.
// HyperKZG.setup of 2^20 powers, key without a table: 5.25 ms at 8 bits, 4.87 / 4.69 / 4.74 / 4.83 at 10 / 11 / 12 / 13.
// ZG_FB_WINDOW_BITS overrides.
struct FbPlan {
    int c, W;
    uint32_t rows;  // 2^c - 1 multiples per window
};
static constexpr int FB_W_MAX = 64;  // c >= 4

// step 1 (one block, quad w of lanes per window): B_w = 2^(8w) * G by 8w doublings, every doubling by a quad (g1_29x4.hip.h) —
// the only serial chain of the build (248 doublings for the top window)
__global__ void __launch_bounds__(4 * FB_W_MAX) fb_window_bases_kernel(const uint64_t *base_xy, int FB_C, char *bw /* W * 144 */) {
    uint32_t w = threadIdx.x >> 2, q = threadIdx.x & 3;
    Affine g = affine_load(base_xy);
    F29 one29;
#pragma unroll
    for (int k = 0; k < 9; k++) one29.l[k] = Fp29::ONE[k];
    XYZZ29 step;
    step.x = f29_from_fp(g.x); step.y = f29_from_fp(g.y); step.zz = one29; step.zzz = one29;
    for (uint32_t k = 0; k < (uint32_t)FB_C * w; k++) step = xyzz29_dbl4(step, q);  // odd prime order: never the identity
    if (q == 0) xyzz29_store(bw + 144 * (size_t)w, step);
}

// step 2 (one thread per table row): d * B_w by double-and-add over the 8 bits of d, then to affine — the packed 64-byte row
// format of the accumulate kernel (x, y as lazy Montgomery-2^261 values)
__global__ void __launch_bounds__(256) fb_table_rows_kernel(const char *bw, uint32_t n_rows, int FB_C, uint32_t FB_ROWS, char *table) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    uint32_t w = i / FB_ROWS, d = i % FB_ROWS + 1;
    XYZZ29 b = xyzz29_load(bw + 144 * (size_t)w), a = xyzz29_identity();
    for (int bit = FB_C - 1; bit >= 0; bit--) {
        a = xyzz29_dbl(a);
        if ((d >> bit) & 1u) a = xyzz29_add(a, b);
    }
    F29 izzz = f29_from_fp(fe_inv_safegcd(f29_to_fp(a.zzz)));
    F29 iz = f29_mul(izzz, a.zz);  // 1/Z = ZZ / ZZZ
    f29_store_packed(table + 64 * (size_t)i, f29_mul(a.x, f29_sqr(iz)));
    f29_store_packed(table + 64 * (size_t)i + 32, f29_mul(a.y, izzz));
}

__global__ void __launch_bounds__(256) fb_mul_kernel(const char *table, const uint64_t *scalars, size_t n, int FB_C, int FB_W, uint32_t FB_ROWS,
                                                     uint64_t *out_xy, uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fr_from_mont29(fe_load<FrParams>(scalars + 4 * i));  // canonical integer, 8 x 32-bit words
    XYZZ29 acc;
    bool acc_inf = true;
    const uint32_t mask = (1u << FB_C) - 1u;
#pragma unroll 1
    for (int w = 0; w < FB_W; w++) {
        const uint32_t d = s.l[0] & mask;  // the next FB_C bits; the scalar is shifted down behind it (static register indices)
#pragma unroll
        for (int k = 0; k < 8; k++) s.l[k] = (s.l[k] >> FB_C) | (k < 7 ? s.l[k + 1] << (32 - FB_C) : 0u);
        if (d == 0) continue;
        Affine row = affine_load(table + 64 * ((size_t)w * FB_ROWS + (d - 1)));
        xyzz29_madd(acc, acc_inf, f29_unpack(row.x.l), f29_unpack(row.y.l));
    }
    Affine r;
    bool isinf = acc_inf;
    if (!isinf) isinf = xyzz_to_affine(xyzz29_to_std_val(acc), r);
    if (isinf) {
        r.x = Fp::zero();
        r.y = Fp::zero();
    }
    affine_store(out_xy + 8 * i, r);
    out_inf[i] = isinf ? 1 : 0;
}

// tau^i for i < n as canonical Montgomery elements, for HyperKZG.setup on the device (zg_hyperkzg_setup): three 256-entry tables of
// powers — tau^a, (tau^256)^b, (tau^65536)^c, one thread each walks its chain of 255 products — then every i = a + 256 b + 65536 c is two
// products. Exact products: the bytes are those of the reference's running product tau_power = tau_power * tau
// (src/poly/commitment/mod.zig:190-199).
__global__ void __launch_bounds__(64) tau_tables_kernel(FeArg tau, uint64_t *tabs /* 4 x 256 x 4 */) {
    if (threadIdx.x >= 4) return;
    Fr t;  // copied here, not through fe_from_arg: that form compiles this kernel to 99 SGPRs instead of 102
#pragma unroll
    for (int i = 0; i < 8; i++) t.l[i] = tau.l[i];
    for (uint32_t k = 0; k < threadIdx.x; k++)  // t = tau^(256^table)
        for (int j = 0; j < 8; j++) t = fr_mul29v(t, t);
    Fr acc = Fr::one();
    uint64_t *out = tabs + (size_t)threadIdx.x * 256 * 4;
    for (int j = 0; j < 256; j++) {
        fe_store(out + 4 * j, acc);
        acc = fr_mul29v(acc, t);
    }
}
__global__ void __launch_bounds__(256) tau_powers_kernel(const uint64_t *tabs, size_t n, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fr v = fe_load<FrParams>(tabs + 4 * (i & 255));
    if (i >> 8) v = fr_mul29v(v, fe_load<FrParams>(tabs + 4 * (256 + ((i >> 8) & 255))));
    if (i >> 16) v = fr_mul29v(v, fe_load<FrParams>(tabs + 4 * (512 + ((i >> 16) & 255))));
    if (i >> 24) v = fr_mul29v(v, fe_load<FrParams>(tabs + 4 * (768 + (i >> 24))));  // the reference's largest key is 2^24 + 256 powers (src/host/mod.zig:384-387)
    fe_store(out + 4 * i, v);
}

// ------------------------------------------------------------------ host side

static void lane_free(zg_bases_s::Lane &ln) {
    void *lp[] = {ln.d_dig, ln.d_sorted, ln.d_hist, ln.d_starts, ln.d_blockhist, ln.d_tmp, ln.d_cstarts, ln.d_fine, ln.d_partial, ln.d_slice_buckets, ln.d_slice_meta, ln.d_bits, ln.d_rg,
                  ln.d_nzrank, ln.d_nzlist, ln.d_nzend, ln.d_scan_tmp, ln.d_part, ln.d_part2, ln.d_heavy, ln.d_state};
    for (void *p : lp) pool_free(p);
    if (ln.done) (void)hipEventDestroy(ln.done);
    ln = zg_bases_s::Lane();
}

static hipError_t lane_malloc(void **p, size_t bytes) {  // from the device pool, like the handle's table (free_bases)
    *p = pool_alloc(bytes ? bytes : 16);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
// workspace of one MSM launch set: n_total scalars (all scalar vectors of a batched launch together) under plan p
static hipError_t lane_alloc(zg_bases_s::Lane &ln, const MsmPlan &p, size_t n_total) {
    hipError_t e = hipSuccess;
    auto A = [&](auto &ptr, size_t bytes) {
        if (e == hipSuccess) e = lane_malloc((void **)&ptr, bytes);
    };
    A(ln.d_dig, (size_t)p.W * n_total * 4);
    A(ln.d_sorted, (size_t)p.W * n_total * 4);
    A(ln.d_hist, (size_t)p.NK * 4);
    A(ln.d_starts, ((size_t)p.NK + 1) * 4);
    const SortWords w = workspace_sort_words(p, n_total);  // the set's own sort and the sort of a point slice
    if (w.blockhist) A(ln.d_blockhist, w.blockhist * 4);
    if (w.tmp) A(ln.d_tmp, w.tmp * 4);
    if (w.cstarts) A(ln.d_cstarts, w.cstarts * 4);
    if (w.fine) A(ln.d_fine, w.fine * 4);
    ln.sort_cap = w;
    A(ln.d_partial, (size_t)p.NK * 144);
    A(ln.d_bits, (size_t)p.G * p.K * bitsum_per_group(p) * 144);
    A(ln.d_rg, (size_t)p.G * p.K * 128);
    A(ln.d_nzrank, ((size_t)p.NK + 1) * 4);
    A(ln.d_nzlist, (size_t)p.NK * 4);
    A(ln.d_nzend, ((size_t)p.NK + 1) * 4);
    A(ln.d_scan_tmp, (2 * (size_t)p.NK + 2 * (p.NK / 1024 + 1)) * 4);
    const size_t slots = (size_t)p.NT + p.NK;
    A(ln.d_part, slots * 144);
    A(ln.d_part2, (slots / HEAVY_BLOCK_ITEMS + 1 + p.NK) * 144);
    A(ln.d_heavy, (size_t)p.NK * 8);
    A(ln.d_state, state_words(p.NT, p.NK) * 4);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.done, hipEventDisableTiming);
    return e;
}

// A handle's table and workspaces come from the device pool (runtime.hip) like every transient allocation: a prover that rebuilds its key
// per proof (or a test that uploads bases per case) reuses the blocks instead of paying hipMalloc / hipFree of gigabytes — 26 ms against
// 113 ms for HyperKZG.setup at 2^20 powers when another process holds a context on the same GPU (bench.py's child runs, round 5). The blocks
// go back only after the device is idle (hipFree used to imply that).
static hipError_t handle_malloc(void **p, size_t bytes) {
    *p = pool_alloc(bytes ? bytes : 16);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static void free_bases(zg_bases_s *b) {
    if (!b) return;
    (void)hipDeviceSynchronize();
    free_bases(b->small);
    void *ptrs[] = {b->d_table, b->d_inf, b->d_scal, b->d_out, b->d_slice_parts, b->d_rows_buckets, b->d_rows_bits, b->d_rows_rg};
    for (void *p : ptrs) pool_free(p);
    if (b->rows_done) (void)hipEventDestroy(b->rows_done);
    for (auto &ln : b->lanes) lane_free(ln);
    lane_free(b->batch_lane);
    for (int i = 0; i < zg_bases_s::NAUX; i++) {
        if (b->aux[i]) (void)hipStreamDestroy(b->aux[i]);
        if (b->ev_join[i]) (void)hipEventDestroy(b->ev_join[i]);
    }
    if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
    if (b->h_out) (void)hipHostFree(b->h_out);
    delete b;
}

#define ZG_ALLOC(ptr, bytes)                                                         \
    do {                                                                             \
        hipError_t _e = handle_malloc((void **)&(ptr), (bytes));                      \
        if (_e != hipSuccess) {                                                      \
            set_error(std::string("hipMalloc(" #ptr "): ") + hipGetErrorString(_e)); \
            free_bases(b);                                                           \
            return _e == hipErrorOutOfMemory ? ZG_ERR_NOMEM : ZG_ERR_HIP;            \
        }                                                                            \
    } while (0)

static constexpr size_t SIDE_TABLE_POINTS = 16384;

// defer_table: everything but the table (plan, allocations, workspaces) — the caller builds it (a handle's side table is built by the
// launch that builds its main table: PreJob).
static int bases_create(const uint64_t *d_xy, const uint8_t *d_inf_in, size_t n, const zg_msm_config *cfg, hipStream_t st,
                        zg_bases_t *out, bool defer_table = false) {
    if (n >= (1ull << 27)) return invalid("msm: at most 2^27 bases per handle");
    zg_bases_s *b = new zg_bases_s();
    b->n = n;
    b->device = current_device();
    int rc = plan_msm(n, cfg, 1, n, b->plan);
    if (rc != ZG_OK) {
        free_bases(b);
        return rc;
    }
    const MsmPlan &p = b->plan;
    if ((uint64_t)p.L * n >= (1ull << 31)) {
        set_error("msm: precompute table too large for 31-bit point references");
        free_bases(b);
        return ZG_ERR_INVALID;
    }
    ZG_ALLOC(b->d_table, (size_t)p.L * n * 64);
    if (d_inf_in) ZG_ALLOC(b->d_inf, n);
    int nlanes = env_int("ZG_MSM_LANES", 6);  // 2^17-point MSMs: 0.36 ms per MSM with 3 in flight, 0.25 with 6 (tools/bench_tail.py)
    if (nlanes < 1) nlanes = 1;
    if (nlanes > 8) nlanes = 8;
    // a one-shot handle (MSM.compute on a temporary slice) serves one MSM: one workspace — a workspace is ~18 allocations, and the
    // upload + free of such a handle is most of what its caller pays (tools/crossover.py: one_shot_msm)
    if (cfg && cfg->expected_uses > 0 && cfg->expected_uses < 16 && !getenv("ZG_MSM_LANES")) nlanes = 1;
    b->lanes.resize(nlanes);
    for (auto &ln : b->lanes) {
        hipError_t le = lane_alloc(ln, p, n);
        if (le != hipSuccess) {
            set_error(std::string("msm workspace: ") + hipGetErrorString(le));
            free_bases(b);
            return le == hipErrorOutOfMemory ? ZG_ERR_NOMEM : ZG_ERR_HIP;
        }
    }
    ZG_ALLOC(b->d_out, 16 * 8);
    if (hipHostMalloc((void **)&b->h_out, 16 * 8) != hipSuccess) {
        set_error("hipHostMalloc failed");
        free_bases(b);
        return ZG_ERR_NOMEM;
    }
    // The side table (narrow windows over the first SIDE_TABLE_POINTS bases, for short MSMs) is a handle of its own; its table is built by
    // the first launch of THIS handle's table kernel (PreJob): created here without a table.
    const bool want_small = !defer_table && (size_t)p.NB * p.G > 4096 && n > SIDE_TABLE_POINTS && env_int("ZG_MSM_SIDE_TABLE", 1);
    if (want_small) {
        zg_msm_config small_cfg{8, 0, 0};
        int src = bases_create(d_xy, d_inf_in, SIDE_TABLE_POINTS, &small_cfg, st, &b->small, true);
        if (src != ZG_OK) {
            b->small = nullptr;
            free_bases(b);
            return src;
        }
    }
    if (defer_table) {  // (the inf flags are copied by the caller's launch sequence, on the same stream)
        *out = b;
        return ZG_OK;
    }
    // the table kernel's per-level records (see msm_precompute_kernel); without them (allocation refused, ZG_MSM_PRECOMPUTE_V1) the
    // round-4 kernel builds the same table with an inversion per level. Released after the synchronisation below.
    const size_t pre_levels = p.L > 1 ? (size_t)(p.L - 1 < PRE_GROUP ? p.L - 1 : PRE_GROUP) : 0;
    // ... for at most PRE_CHUNK bases at a time (2^21: 2.1 GB of records whatever the handle's size — a 2^24-base handle would ask for 17 GB
    // beside its 16 GiB table, and a fresh allocation of that size costs more than the kernel it serves)
    const size_t pre_chunk = n < PRE_CHUNK ? (n ? n : 1) : PRE_CHUNK;
    const bool v1 = env_int("ZG_MSM_PRECOMPUTE_V1", 0) != 0;
    Staging sg(st);
    char *pre_rec = n && pre_levels && !v1 ? sg.try_out<char>(pre_levels * pre_chunk * 144) : nullptr;
    const zg_bases_s *sm = b->small;
    char *side_rec = sm && !v1 ? sg.try_out<char>((size_t)PRE_GROUP * sm->n * 144) : nullptr;
    if (n) {
        if (d_inf_in) ZG_STAGE(sg, hipMemcpyAsync(b->d_inf, d_inf_in, n, hipMemcpyDeviceToDevice, st));
        if (sg.ok() && sm && d_inf_in) ZG_STAGE(sg, hipMemcpyAsync(sm->d_inf, d_inf_in, sm->n, hipMemcpyDeviceToDevice, st));
        if (sg.ok()) {
            PreJob side{};  // no workgroups unless the side table rides along
            bool side_pending = sm != nullptr;
            if (side_pending && side_rec)
                side = PreJob{d_xy, sm->d_inf, sm->n, sm->plan.L, sm->plan.c * sm->plan.G, sm->d_table, side_rec, 0, sm->n, (unsigned)div_up(sm->n, 256)};
            if (pre_rec || p.L == 1) {
                // (a handle without a table, L == 1, needs no records: its job only converts the bases; the side table still rides along)
                for (size_t first = 0; first < n; first += pre_chunk) {  // the launches reuse the records one after the other (stream order)
                    const size_t count = n - first < pre_chunk ? n - first : pre_chunk;
                    const PreJob mj{d_xy, b->d_inf, n, p.L, p.c * p.G, b->d_table, pre_rec, first, count, (unsigned)div_up(count, 256)};
                    hipLaunchKernelGGL(msm_precompute_kernel, dim3(side.blocks + mj.blocks), dim3(256), 0, st, side, mj);
                    if (side.blocks) side_pending = false;
                    side = PreJob{};
                }
            } else {
                hipLaunchKernelGGL(msm_precompute_v1_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_xy, b->d_inf, n, p.L, p.c * p.G, b->d_table);
            }
            if (side_pending)  // no records for it (allocation refused / ZG_MSM_PRECOMPUTE_V1): the round-4 kernel, on its own
                hipLaunchKernelGGL(msm_precompute_v1_kernel, dim3(div_up(sm->n, 256)), dim3(256), 0, st, d_xy, sm->d_inf, sm->n, sm->plan.L,
                                   sm->plan.c * sm->plan.G, sm->d_table);
            sg.launched();
        }
    }
    if (sg.finish() != ZG_OK) {  // (it waits on failure too: nothing of this handle may still be in flight when it is freed)
        free_bases(b);
        return sg.rc;
    }
    *out = b;
    return ZG_OK;
}

template <int C>
static void launch_digits(hipStream_t st, const uint64_t *sc, const uint8_t *inf, uint32_t n, uint32_t n_pts, int G, uint32_t *dig,
                          uint32_t *hist) {
    hipLaunchKernelGGL(msm_digits_kernel<C>, dim3(div_up(n, 256)), dim3(256), 0, st, sc, inf, n, n_pts, G, dig, hist);
}

// threads per block of the two LDS sort kernels (one block per CU either way: each needs all bucket counters in LDS)
static unsigned sort_threads() {
    static const unsigned t = [] {
        int v = env_int("ZG_MSM_SORT_THREADS", 512);  // 8 waves: fit beside two accumulate workgroups of another stream (measured +3.7 % MSM/s)
        return (unsigned)(v >= 1024 ? 1024 : (v >= 512 ? 512 : 256));
    }();
    return t;
}

template <int C>
static int launch_digits_lds(hipStream_t st, const uint64_t *sc, const uint8_t *inf, uint32_t n, uint32_t n_pts, int G, uint32_t per_block,
                             uint32_t NK, uint32_t nblk, uint32_t *dig, uint32_t *blockhist, int shift, unsigned threads, const RowOffs &rows) {
    static PerDeviceOnce once;  // per instantiation and device; MSM entry points are re-entrant (std.Thread workers call MSM.compute)
    ZG_HIP(once.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(msm_digits_lds_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    }));
    hipLaunchKernelGGL(msm_digits_lds_kernel<C>, dim3(nblk), dim3(threads), NK * 4, st, sc, inf, n, n_pts, G, per_block, NK, shift, dig, blockhist, rows);
    return ZG_OK;
}

static int launch_digits_lds_c(int c, hipStream_t st, const uint64_t *sc, const uint8_t *inf, uint32_t n, uint32_t n_pts, int G,
                               uint32_t per_block, uint32_t NK, uint32_t nblk, uint32_t *dig, uint32_t *blockhist, int shift = 0,
                               unsigned threads = 0, const RowOffs *rows_in = nullptr) {
    static const RowOffs uniform{};
    const RowOffs &rows = rows_in ? *rows_in : uniform;
    if (!threads) threads = sort_threads();
    switch (c) {
#define ZG_CASE(C) case C: return launch_digits_lds<C>(st, sc, inf, n, n_pts, G, per_block, NK, nblk, dig, blockhist, shift, threads, rows);
        ZG_CASE(2) ZG_CASE(3) ZG_CASE(4) ZG_CASE(5) ZG_CASE(6) ZG_CASE(7) ZG_CASE(8) ZG_CASE(9) ZG_CASE(10)
        ZG_CASE(11) ZG_CASE(12) ZG_CASE(13) ZG_CASE(14) ZG_CASE(15) ZG_CASE(16) ZG_CASE(17) ZG_CASE(18) ZG_CASE(19)
#undef ZG_CASE
        default: return invalid("msm: unsupported window size");
    }
}

static int launch_digits_c(int c, hipStream_t st, const uint64_t *sc, const uint8_t *inf, uint32_t n, uint32_t n_pts, int G, uint32_t *dig,
                           uint32_t *hist) {
    switch (c) {
#define ZG_CASE(C) case C: launch_digits<C>(st, sc, inf, n, n_pts, G, dig, hist); break;
        ZG_CASE(2) ZG_CASE(3) ZG_CASE(4) ZG_CASE(5) ZG_CASE(6) ZG_CASE(7) ZG_CASE(8) ZG_CASE(9) ZG_CASE(10)
        ZG_CASE(11) ZG_CASE(12) ZG_CASE(13) ZG_CASE(14) ZG_CASE(15) ZG_CASE(16) ZG_CASE(17) ZG_CASE(18) ZG_CASE(19)
#undef ZG_CASE
        default: return invalid("msm: unsupported window size");
    }
    return ZG_OK;
}

static int two_pass_attrs() {
    static PerDeviceOnce once;
    ZG_HIP(once.run([] {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(msm_partition_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void *>(msm_partition_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void *>(msm_fine_place_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
        return err;
    }));
    return ZG_OK;
}

static int ensure_aux_streams(zg_bases_s *b) {
    if (b->aux[0]) return ZG_OK;
    hipError_t e = hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming);
    for (int i = 0; i < zg_bases_s::NAUX && e == hipSuccess; i++) {
        e = hipStreamCreateWithFlags(&b->aux[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->ev_join[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        set_error(std::string("msm helper streams: ") + hipGetErrorString(e));
        return ZG_ERR_HIP;
    }
    return ZG_OK;
}

// ---- point slices. The accumulate kernel gathers one random 64-byte table row per addition; the rows of one launch set span
// L * n * 64 bytes, and random rows over more than ~1-2 GiB run at half the rate of rows inside 1 GiB on this part (translation
// reach: tools/microbench_tlb — 56 G rows/s inside 1 GiB, 25 G over 4 GiB, however the 4 GiB are allocated). At 2^22 points
// (4 GiB table) that cost the kernel +10 % per addition, at 2^24 (16 GiB) +45 %. A long MSM is therefore cut into slices of
// consecutive points whose L table segments together stay within ZG_MSM_TABLE_SPAN_MB (default 1024): slice j is sorted and
// accumulated by itself (same workspace, same stream, one after the other) into its own set of bucket sums, one launch adds
// the sets up bucket by bucket, and the reduction runs ONCE — the fixed tail is not multiplied (slices as separate MSMs with
// a Jacobian combine were measured first: 4 x 0.45 ms of sorts and tails ate the whole gain). The sums are the same group
// elements, so the result bytes are those of the unsliced launch set.
static size_t table_span_points(const zg_bases_s *b) { return table_span_points(b->plan.L); }
struct SliceView {  // what the sort of a point slice hands to its accumulation
    uint32_t *sorted, *starts, *nzrank, *nzlist, *nzend;
    void *state;
};

// bucket set 0 += sets 1 .. S-1 (set j at sets + (j-1) * NK * 144), one quad of lanes per bucket
__global__ void __launch_bounds__(256) msm_bucket_fold_kernel(char *buckets, const char *sets, uint32_t NK, uint32_t S) {
    ZG_HIPRIO();
    uint32_t k = (blockIdx.x * 256 + threadIdx.x) >> 2, q = threadIdx.x & 3;
    if (k >= NK) return;
    XYZZ29 acc = xyzz29_load(buckets + 144 * (size_t)k);
    XYZZ29 nxt = xyzz29_load(sets + 144 * (size_t)k);
    for (uint32_t j = 1; j < S; j++) {
        XYZZ29 cur = nxt;
        if (j + 1 < S) nxt = xyzz29_load(sets + 144 * ((size_t)j * NK + k));
        acc = xyzz29_add4(acc, cur, q);
    }
    if (q == 0) xyzz29_store(buckets + 144 * (size_t)k, acc);
}

// bucket counts (ln.d_hist) -> what a sort hands to its accumulation: bucket starts, non-empty ranks / list / run ends, reduction state
static void launch_scan(const MsmPlan &p, const zg_bases_s::Lane &ln, hipStream_t st, const SliceView &sv) {
    const uint32_t tiles = div_up(p.NK, 1024);
    hipLaunchKernelGGL(msm_scan_a_kernel, dim3(tiles), dim3(1024), 0, st, ln.d_hist, p.NK, ln.d_scan_tmp, ln.d_scan_tmp + p.NK,
                       ln.d_scan_tmp + 2 * (size_t)p.NK);
    hipLaunchKernelGGL(msm_scan_b_kernel, dim3(tiles), dim3(1024), 0, st, ln.d_hist, p.NK, ln.d_scan_tmp, ln.d_scan_tmp + p.NK,
                       ln.d_scan_tmp + 2 * (size_t)p.NK, sv.starts, sv.nzrank, sv.nzlist, sv.nzend, reinterpret_cast<uint32_t *>(sv.state),
                       state_words(p.NT, p.NK));
}

// Stage 1 of a launch set: digits and sort of bases[off, off + n_pts) x p.K scalar vectors at d_scalars -> sv (sorted references, bucket
// starts, ...). q: the plan this range sorts under (LaunchCut::sort: fine bits / coarse bins), local_shift: its references
// (LaunchCut::local_shift). rows: the live lengths of the p.K rows, or nullptr for the padded matrix (msm_enqueue_lane).
static int sort_range(const zg_bases_s *b, const MsmPlan &p, const MsmPlan &q, int local_shift, const zg_bases_s::Lane &ln, const RowOffs *rows,
                      size_t off, size_t n_pts, const uint64_t *d_scalars, hipStream_t st, const SliceView &sv) {
    static const RowOffs uniform_rows{};
    const RowOffs &rowv = rows ? *rows : uniform_rows;
    const size_t n = rows ? rows->off[rows->k] : n_pts * (size_t)p.K;  // scalars in this launch set
    const uint8_t *infp = b->d_inf ? b->d_inf + off : nullptr;
    const uint32_t nblk = sort_blocks(q, n);
    if (q.sort == MsmSort::TWO_PASS) {
        // two-pass sort: blocks of 256 threads over TWO_PASS_SPAN scalars each (coarse counters are a few KiB of LDS)
        if ((size_t)nblk * q.NCB > ln.sort_cap.blockhist) return invalid("msm: two-pass workspace too small for this launch");
        uint32_t per_block = (uint32_t)((n + nblk - 1) / nblk);
        prof_begin(ZG_PROF_MSM_DIGITS, st);
        ZG_TRY(launch_digits_lds_c(p.c, st, d_scalars, infp, (uint32_t)n, (uint32_t)n_pts, p.G, per_block, q.NCB, nblk, ln.d_dig,
                                   ln.d_blockhist, q.fb, 256, rows));
        prof_end(ZG_PROF_MSM_DIGITS, st);
        prof_begin(ZG_PROF_MSM_SORT, st);
        uint32_t *d_tot = ln.d_cstarts + q.NCB + 1, *d_tst = ln.d_cstarts + 2 * (size_t)q.NCB + 2, *d_ist = ln.d_cstarts + 3 * (size_t)q.NCB + 3;
        hipLaunchKernelGGL(msm_colscan_bins_kernel, dim3(div_up(q.NCB, 16)), dim3(1024), 0, st, ln.d_blockhist, nblk, q.NCB, d_tot);
        hipLaunchKernelGGL(msm_coarse_base_kernel, dim3(1), dim3(1024), 0, st, d_tot, q.NCB, ln.d_cstarts, d_tst, d_ist);
        ZG_TRY(two_pass_attrs());
        if (!rows && p.G == 1 && n == n_pts)  // PLAIN uses i as the point index: never with live row lengths (their total may equal n_pts)
            hipLaunchKernelGGL(msm_partition_kernel<true>, dim3(nblk), dim3(1024), (STAGE_ENTRIES + 2 * (size_t)q.NCB + 1 + 1024) * 4, st, ln.d_dig,
                               (uint32_t)n, (uint32_t)n_pts, p.W, p.G, b->n, (uint32_t)off, per_block, q.NCB, q.fb, q.rb, d_tst, ln.d_blockhist,
                               ln.d_tmp, local_shift, rowv);
        else
            hipLaunchKernelGGL(msm_partition_kernel<false>, dim3(nblk), dim3(1024), (STAGE_ENTRIES + 2 * (size_t)q.NCB + 1 + 1024) * 4, st, ln.d_dig,
                               (uint32_t)n, (uint32_t)n_pts, p.W, p.G, b->n, (uint32_t)off, per_block, q.NCB, q.fb, q.rb, d_tst, ln.d_blockhist,
                               ln.d_tmp, local_shift, rowv);
        {
            uint32_t items = (uint32_t)fine_max_items(q, n);
            uint32_t *d_fbase = ln.d_fine + (size_t)items * ((size_t)1 << q.fb);
            hipLaunchKernelGGL(msm_fine_count_kernel, dim3(items), dim3(1024), 0, st, ln.d_tmp, ln.d_cstarts, d_tst, d_ist, q.NCB, q.fb, q.rb,
                               ln.d_fine);
            hipLaunchKernelGGL(msm_fine_offsets_kernel, dim3(q.NCB), dim3(128), 0, st, d_ist, q.fb, p.NK, ln.d_fine, d_fbase, ln.d_hist);
            hipLaunchKernelGGL(msm_fine_place_kernel, dim3(items), dim3(1024), (STAGE_ENTRIES + 128 + 132) * 4, st, ln.d_tmp, ln.d_cstarts, d_tst,
                               d_ist, q.NCB, q.fb, q.rb, ln.d_fine, d_fbase, sv.sorted, local_shift, (uint32_t)b->n, (uint32_t)off);
        }
        launch_scan(p, ln, st, sv);
    } else if (q.sort == MsmSort::LDS) {
        uint32_t per_block = (uint32_t)((n + nblk - 1) / nblk);
        prof_begin(ZG_PROF_MSM_DIGITS, st);
        ZG_TRY(launch_digits_lds_c(p.c, st, d_scalars, infp, (uint32_t)n, (uint32_t)n_pts, p.G, per_block, p.NK, nblk, ln.d_dig,
                                   ln.d_blockhist, 0, 0, rows));
        prof_end(ZG_PROF_MSM_DIGITS, st);
        prof_begin(ZG_PROF_MSM_SORT, st);
        hipLaunchKernelGGL(msm_colscan_kernel, dim3(div_up(p.NK, 256)), dim3(256), 0, st, ln.d_blockhist, nblk, p.NK, ln.d_hist);
        launch_scan(p, ln, st, sv);
        static PerDeviceOnce scatter_once;
        ZG_HIP(scatter_once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(msm_scatter_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        }));
        hipLaunchKernelGGL(msm_scatter_lds_kernel, dim3(nblk), dim3(sort_threads()), p.NK * 4, st, ln.d_dig, (uint32_t)n, (uint32_t)n_pts, p.W, p.G,
                           b->n, (uint32_t)off, per_block, p.NK, sv.starts, ln.d_blockhist, sv.sorted, rowv);
    } else {
        prof_begin(ZG_PROF_MSM_DIGITS, st);
        ZG_HIP(hipMemsetAsync(ln.d_hist, 0, (size_t)p.NK * 4, st));
        ZG_TRY(launch_digits_c(p.c, st, d_scalars, infp, (uint32_t)n, (uint32_t)n_pts, p.G, ln.d_dig, ln.d_hist));
        prof_end(ZG_PROF_MSM_DIGITS, st);
        prof_begin(ZG_PROF_MSM_SORT, st);
        launch_scan(p, ln, st, sv);
        ZG_HIP(hipMemsetAsync(ln.d_hist, 0, (size_t)p.NK * 4, st));
        hipLaunchKernelGGL(msm_scatter_kernel, dim3(div_up(n, 256), p.W), dim3(256), 0, st, ln.d_dig, (uint32_t)n, (uint32_t)n_pts, p.G,
                           b->n, (uint32_t)off, sv.starts, ln.d_hist, sv.sorted);
    }
    prof_end(ZG_PROF_MSM_SORT, st);
    return ZG_OK;
}

// Stage 2: accumulation, bucket combine and heavy stage of a sorted range of n_pts x p.K scalars -> the bucket sums at bucket_out
static int accumulate_range(zg_bases_s *b, const MsmPlan &p, const zg_bases_s::Lane &ln, size_t n_pts, hipStream_t st, const SliceView &sv,
                            char *bucket_out) {
    prof_begin(ZG_PROF_MSM_ACCUMULATE, st);
    bool alone = env_int("ZG_MSM_ALONE_FULL", 1) != 0;
    // (round 6) an MSM still in flight ON THIS STREAM is not company: its kernels finish before this launch starts (stream order), so
    // there is nothing the spare registers could run under. Only work on OTHER streams makes the 7/8 launch pay; a caller that
    // pipelines on one stream gets the full grid (serial bench at 2^20: accumulate 1.30 -> 1.18 ms per launch).
    for (auto &o : b->lanes)
        if (alone && &o != &ln && o.used && o.last_st != st && hipEventQuery(o.done) == hipErrorNotReady) alone = false;
    (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure
    // a table-less launch set (one bucket set per window: its reduction is a few hundred short workgroups, not a latency chain under
    // someone else's accumulation) takes every slot either way: 612 MSM/s against 587 / 596 / 603 at 15/16, 7/8, 13/16 of them
    if (p.G > 1) alone = true;
    const uint32_t NT = launch_chunks(p, n_pts * (size_t)p.K, alone);
    // threads per accumulate workgroup (64 / 128 / 256). Smaller workgroups spread evenly over the CUs and lose what the 7/8 launch
    // gains (profiles/r4h_accumulate_slots_sweep.txt: 64 threads 771 / 745 / 696 MSM/s at 512 / 480 / 448 workgroups' worth of
    // chunks against 761 / 780 / 791 with 256; 512-thread workgroups 776 / 754 / 777)
    static const unsigned acc_block = [] {
        int v = env_int("ZG_MSM_ACC_BLOCK", 256);
        return (unsigned)(v == 64 || v == 128 ? v : 256);
    }();
    if (NT <= (uint32_t)env_int("ZG_MSM_QUAD_ACC_MAX_CHUNKS", 32768))
        hipLaunchKernelGGL(msm_accumulate_chunk_kernel<true>, dim3(div_up((size_t)NT * 4, 256)), dim3(256), 0, st, sv.sorted, sv.starts,
                           sv.nzrank, sv.nzend, b->d_table, p.NK, NT, ln.d_part);
    else
        hipLaunchKernelGGL(msm_accumulate_chunk_kernel<false>, dim3(div_up(NT, acc_block)), dim3(acc_block), 0, st, sv.sorted, sv.starts,
                           sv.nzrank, sv.nzend, b->d_table, p.NK, NT, ln.d_part);
    prof_end(ZG_PROF_MSM_ACCUMULATE, st);  // the dominant kernel alone; combine/heavy stages count as reduction
    prof_begin(ZG_PROF_MSM_REDUCE, st);
    if (p.tail == MsmTail::LANE)
        hipLaunchKernelGGL(msm_bucket_combine_lane_kernel, dim3(div_up(p.NK, 64)), dim3(64), 0, st, ln.d_part, sv.starts, sv.nzrank, p.NK, NT,
                           bucket_out, ln.d_heavy, reinterpret_cast<MsmState *>(sv.state));
    else
        hipLaunchKernelGGL(msm_bucket_combine_kernel, dim3(div_up((size_t)p.NK * p.GS * 4, 64)), dim3(64), 0, st, ln.d_part, sv.starts,
                           sv.nzrank, p.NK, NT, p.GS, bucket_out, ln.d_heavy, reinterpret_cast<MsmState *>(sv.state));
    uint32_t nblk_a = (NT + p.NK) / HEAVY_BLOCK_ITEMS + 1;  // stage-A blocks of the huge buckets; at least 256 blocks = 1024 waves for the heavy ones
    hipLaunchKernelGGL(msm_heavy_kernel, dim3(nblk_a < 256 ? 256 : nblk_a), dim3(256), 0, st, ln.d_part, sv.starts, sv.nzrank, sv.nzlist,
                       p.NK, NT, ln.d_heavy, reinterpret_cast<MsmState *>(sv.state), ln.d_part2, bucket_out);
    return ZG_OK;
}

// Stage 3: the bucket sums of GK bucket groups (p.G per scalar vector, back to back at `buckets`) -> result records. Row / column sums
// and the two-dimensional bit sums, or the one-dimensional bit sums; msm_final_kernel per group; the window combine when G > 1. bits
// holds GK * bitsum_per_group(p) sums, rg one result per group; vector i's record lands at d_rec + i*rec_stride / d_inf_out + i*inf_stride.
static void reduce_buckets(const MsmPlan &p, int GK, const char *buckets, char *bits, char *rg, hipStream_t st, int mode, uint64_t *d_rec,
                           uint8_t *d_inf_out, uint32_t rec_stride, uint32_t inf_stride) {
    if (p.lb) {
        char *d_rc = bits + 144 * (size_t)GK * p.c;  // rows and columns behind the c bit sums of every group
        if (p.tail == MsmTail::LANE)  // one bucket set (plan_tail)
            hipLaunchKernelGGL(msm_rowcol_lane_kernel, dim3(lane_map::workgroups(p.lb, p.hb), 1), dim3(256), 0, st, buckets, p.NB, p.lb, p.hb, d_rc);
        else
            launch_rowcol(st, buckets, p.NB, p.lb, p.hb, GK, d_rc);
        hipLaunchKernelGGL(msm_bits2d_kernel, dim3(p.c, GK), dim3(256), 0, st, buckets, d_rc, p.NB, p.c, p.lb, p.hb, bits);
    } else {
        hipLaunchKernelGGL(msm_bitsum_kernel, dim3(p.PB, p.c, GK), dim3(256), 0, st, buckets, p.NB, p.c, bits);
    }
    hipLaunchKernelGGL(msm_final_kernel, dim3(GK), dim3(512), 0, st, bits, p.c, p.lb ? 1 : p.PB, p.G, rg, mode, d_rec, d_inf_out, rec_stride,
                       inf_stride);
    if (p.G > 1)
        hipLaunchKernelGGL(msm_groups_kernel, dim3(GK / p.G), dim3(4), 0, st, rg, p.G, p.c, mode, d_rec, d_inf_out, rec_stride, inf_stride);
}

// One launch set on workspace `ln` under plan `p`: p.K scalar vectors of n_pts scalars each, stored back to back at
// d_scalars, all over bases[off, off+n_pts); vector i's record lands at d_rec + i*rec_stride / d_inf_out + i*inf_stride.
// rows: the live lengths of the p.K zero-padded rows, which the sort then walks instead of the padded matrix (see RowOffs), or nullptr.
// bucket_sink: where the set leaves its bucket sums INSTEAD of reducing them (the caller reduces them: msm_rows_shared_tail), or nullptr.
// The callers decide when either applies; both need a set that is not sliced.
static int msm_enqueue_lane(zg_bases_s *b, const MsmPlan &p, zg_bases_s::Lane &ln, size_t off, size_t n_pts,
                            const uint64_t *d_scalars, hipStream_t st, int mode, uint64_t *d_rec, uint8_t *d_inf_out,
                            uint32_t rec_stride, uint32_t inf_stride, const RowOffs *rows, char *bucket_sink) {
    if (ln.used) ZG_HIP(hipStreamWaitEvent(st, ln.done, 0));  // the lane's previous MSM may be on another stream
    ln.used = true;
    ln.last_st = st;
    // point slices (see table_span_points): S > 1 only for one scalar vector over a table wider than the span
    const LaunchCut cut = launch_cut(p, n_pts, ln.sort_cap);
    const size_t S = cut.S, per = cut.per;
    // no caller gets here (K >= 2 is never sliced: slice_counts; rows_shared_tail_ok): ignoring a sink would leave the caller reducing stale sums
    if ((rows || bucket_sink) && S != 1) return invalid("msm: live row lengths and a bucket sink need an unsliced launch set");
    // per slice: bucket starts, non-empty ranks, non-empty list, run ends, reduction state (what a sort hands to its accumulation), 16-byte aligned
    const size_t meta_stride = (4 * ((size_t)p.NK + 1) + state_words(p.NT, p.NK) + 3) & ~(size_t)3;
    if (S > 1 && ln.slice_buckets < S - 1) {
        if (ln.d_slice_buckets || ln.d_slice_meta) ZG_HIP(hipDeviceSynchronize());  // once per lane and slice count: the old buffers may be in use
        pool_free(ln.d_slice_buckets);
        ln.d_slice_buckets = nullptr;
        ln.slice_buckets = 0;
        ZG_HIP(lane_malloc((void **)&ln.d_slice_buckets, (S - 1) * (size_t)p.NK * 144));
        pool_free(ln.d_slice_meta);
        ln.d_slice_meta = nullptr;
        ZG_HIP(lane_malloc((void **)&ln.d_slice_meta, S * meta_stride * 4));
        ln.slice_buckets = S - 1;
    }
    // slice by slice, each sorted right before its accumulation (sorting every slice first measured 7 % slower at 2^22)
    for (size_t j = 0; j < S; j++) {
        const size_t a = j * per, cnt = n_pts - a < per ? n_pts - a : per;
        SliceView sv{ln.d_sorted, ln.d_starts, ln.d_nzrank, ln.d_nzlist, ln.d_nzend, ln.d_state};
        if (S > 1) {
            uint32_t *m = ln.d_slice_meta + j * meta_stride;
            sv = SliceView{ln.d_sorted + j * (size_t)p.W * per, m, m + ((size_t)p.NK + 1), m + 2 * ((size_t)p.NK + 1), m + 3 * ((size_t)p.NK + 1),
                           m + 4 * ((size_t)p.NK + 1)};
        }
        if (j) prof_end(ZG_PROF_MSM_REDUCE, st);  // the bucket sums of a slice count as reduction
        ZG_TRY(sort_range(b, p, cut.sort, cut.local_shift, ln, rows, off + a, cnt, d_scalars + 4 * a, st, sv));
        ZG_TRY(accumulate_range(b, p, ln, cnt, st, sv, j ? ln.d_slice_buckets + (j - 1) * (size_t)p.NK * 144 : bucket_sink ? bucket_sink : ln.d_partial));
    }
    if (S > 1)
        hipLaunchKernelGGL(msm_bucket_fold_kernel, dim3(div_up((size_t)p.NK * 4, 256)), dim3(256), 0, st, ln.d_partial, ln.d_slice_buckets, p.NK,
                           (uint32_t)S);
    if (!bucket_sink)  // with a sink the set ends at its bucket sums
        reduce_buckets(p, p.G * p.K, ln.d_partial, ln.d_bits, ln.d_rg, st, mode, d_rec, d_inf_out, rec_stride, inf_stride);
    prof_end(ZG_PROF_MSM_REDUCE, st);
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipEventRecord(ln.done, st));
    return ZG_OK;
}

// Enqueue one MSM over bases[off, off+n) on `st`; result record lands in d_rec / d_inf_out — or, with a bucket_sink, its bucket sums land
// there and no record is written (msm_enqueue_lane; the caller has made sure that the launch is not sliced). A single vector has no rows
// of different lengths.
static int msm_enqueue(zg_bases_s *b, size_t off, size_t n, const uint64_t *d_scalars, hipStream_t st, int mode, uint64_t *d_rec,
                       uint8_t *d_inf_out, char *bucket_sink = nullptr /* the default reduces to a record */) {
    if (off + n > b->n) return invalid("msm: range exceeds uploaded bases");
    if (n == 0) {  // msm/mod.zig:361-363
        hipLaunchKernelGGL(msm_identity_kernel, dim3(1), dim3(1), 0, st, mode, d_rec, d_inf_out);
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    if (b->small && off + n <= b->small->n) return msm_enqueue(b->small, off, n, d_scalars, st, mode, d_rec, d_inf_out, bucket_sink);  // short prefix
    zg_bases_s::Lane &ln = b->lanes[b->next_lane];
    b->next_lane = (b->next_lane + 1) % b->lanes.size();
    return msm_enqueue_lane(b, b->plan, ln, off, n, d_scalars, st, mode, d_rec, d_inf_out, 0, 0, nullptr, bucket_sink);
}

// ---- toAffine on the host for the entry points that hand the result to the host anyway. On the device the inversion is a
// single-lane safegcd of ~41 us at the very end of a latency chain (a third of msm_final_kernel); the host does it in a few
// microseconds. The device hands over the un-normalised Jacobian record of mode 2, (X*ZZ, Y*ZZZ, ZZ): x = X'/Z^2, y = Y'/Z^3 —
// canonical Montgomery residues, so the bytes are those of the device's own toAffine (msm/mod.zig:178-189).
namespace hostfp {
typedef unsigned __int128 u128;
static const uint64_t P[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static uint64_t n0inv() {  // -P^-1 mod 2^64
    uint64_t inv = 1;
    for (int i = 0; i < 6; i++) inv *= 2 - P[0] * inv;
    return 0 - inv;
}
static void mul(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {  // Montgomery product, CIOS, result < P
    static const uint64_t N0 = n0inv();
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a[j] * b[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * N0;
        c = ((u128)m * P[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * P[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    uint64_t d[4];
    u128 br = 0;
    for (int j = 0; j < 4; j++) {
        u128 v = (u128)t[j] - P[j] - (uint64_t)br;
        d[j] = (uint64_t)v;
        br = (v >> 64) & 1;
    }
    const bool ge = t[4] != 0 || br == 0;
    for (int j = 0; j < 4; j++) r[j] = ge ? d[j] : t[j];
}
static void inv(uint64_t r[4], const uint64_t a[4]) {  // a^(P-2), Montgomery domain in and out; a != 0
    uint64_t e[4] = {P[0] - 2, P[1], P[2], P[3]}, acc[4], base[4];
    bool started = false;
    for (int j = 0; j < 4; j++) base[j] = a[j];
    for (int bit = 253; bit >= 0; bit--) {
        if (started) mul(acc, acc, acc);
        if ((e[bit >> 6] >> (bit & 63)) & 1) {
            if (started) mul(acc, acc, base);
            else {
                for (int j = 0; j < 4; j++) acc[j] = base[j];
                started = true;
            }
        }
    }
    for (int j = 0; j < 4; j++) r[j] = acc[j];
}
// (X, Y, Z) Jacobian record -> affine xy[8] + infinity flag
static void jacobian_to_affine(const uint64_t rec[12], uint64_t out_xy[8], uint8_t *out_inf) {
    const uint64_t *X = rec, *Y = rec + 4, *Z = rec + 8;
    if ((Z[0] | Z[1] | Z[2] | Z[3]) == 0) {
        for (int i = 0; i < 8; i++) out_xy[i] = 0;
        if (out_inf) *out_inf = 1;
        return;
    }
    uint64_t iz[4], iz2[4], iz3[4];
    inv(iz, Z);
    mul(iz2, iz, iz);
    mul(iz3, iz2, iz);
    mul(out_xy, X, iz2);
    mul(out_xy + 4, Y, iz3);
    if (out_inf) *out_inf = 0;
}
}  // namespace hostfp

static int msm_to_host(zg_bases_s *b, size_t off, size_t n, const uint64_t *d_scalars, hipStream_t st, uint64_t out_xy[8],
                       uint8_t *out_inf) {
    if (!env_int("ZG_MSM_HOST_AFFINE", 1)) {  // A/B: toAffine inside msm_final_kernel
        ZG_TRY(msm_enqueue(b, off, n, d_scalars, st, 0, b->d_out, reinterpret_cast<uint8_t *>(b->d_out + 8)));
        ZG_HIP(hipMemcpyAsync(b->h_out, b->d_out, 9 * 8, hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < 8; i++) out_xy[i] = b->h_out[i];
        if (out_inf) *out_inf = (uint8_t)(b->h_out[8] & 0xff);
        return ZG_OK;
    }
    ZG_TRY(msm_enqueue(b, off, n, d_scalars, st, 2, b->d_out, nullptr));
    ZG_HIP(hipMemcpyAsync(b->h_out, b->d_out, 12 * 8, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    hostfp::jacobian_to_affine(b->h_out, out_xy, out_inf);
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_g1_bases_upload_dev(const uint64_t *d_xy, const uint8_t *d_inf, size_t n, const zg_msm_config *cfg, void *stream,
                           zg_bases_t *out) {
    ZG_INIT();
    if (!out || (n && !d_xy)) return invalid("zg_g1_bases_upload_dev: invalid argument");
    return bases_create(d_xy, d_inf, n, cfg, pick_stream(stream), out);
}

int zg_g1_bases_upload(const uint64_t *xy, const uint8_t *inf, size_t n, const zg_msm_config *cfg, zg_bases_t *out) {
    ZG_INIT();
    if (!out || (n && !xy)) return invalid("zg_g1_bases_upload: invalid argument");
    Staging sg(lib_stream());  // the staging copies go back to the pool only after the table build that reads them has finished
    const uint64_t *dxy = n ? sg.in(xy, n * 64) : nullptr;
    const uint8_t *dinf = n ? sg.in(inf, n) : nullptr;
    if (sg.ok()) sg.adopt(bases_create(dxy, dinf, n, cfg, sg.st, out));
    return sg.finish();
}

int zg_g1_bases_free(zg_bases_t b) {
    if (!b) return ZG_OK;
    ZG_INIT();
    DeviceGuard dg(b->device);
    (void)hipDeviceSynchronize();
    free_bases(b);
    return ZG_OK;
}

size_t zg_g1_bases_len(zg_bases_t b) { return b ? b->n : 0; }

int zg_g1_bases_plan(zg_bases_t b, int *window_bits, int *windows, int *precompute_levels) {
    if (!b) return invalid("zg_g1_bases_plan: invalid argument");
    if (window_bits) *window_bits = b->plan.c;
    if (windows) *windows = b->plan.W;
    if (precompute_levels) *precompute_levels = b->plan.L;
    return ZG_OK;
}

size_t zg_g1_bases_table_bytes(zg_bases_t b) { return b ? (size_t)(b->plan.L > 1 ? b->plan.L : 1) * b->n * 64 : 0; }

int zg_msm_g1_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars, void *stream, uint64_t out_xy[8], uint8_t *out_inf) {
    ZG_INIT();
    if (!b || !out_xy || (n && !d_scalars)) return invalid("zg_msm_g1_dev: invalid argument");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_to_host(b, off, n, d_scalars, pick_stream(stream), out_xy, out_inf);
}

// The host-scalar entry point — what an unmodified MSM.compute / HyperKZG.commit call site reaches — pays a 32*n-byte H2D copy
// (0.7 ms at 2^20 over PCIe Gen5) before anything can run. Long vectors are therefore cut into slices: slice i's copy runs
// while slice i-1's launch set computes (three streams, the handle's workspaces rotate), every slice ends in an un-normalised
// Jacobian partial, and one combine launch adds them up (the group sum does not depend on how the points were grouped, so
// the bytes are those of the unsliced MSM).
static constexpr size_t HOST_SLICE_MIN_POINTS = (size_t)1 << 18;
static size_t host_slice_min() { return (size_t)env_int("ZG_MSM_HOST_SLICE_MIN", (int)HOST_SLICE_MIN_POINTS); }  // tests lower it
static constexpr int HOST_SLICES_MAX = 8;

static int msm_host_sliced(zg_bases_s *b, size_t off, size_t n, const uint64_t *scalars, int slices, uint64_t out_xy[8], uint8_t *out_inf) {
    hipStream_t st = lib_stream();
    ZG_TRY(ensure_aux_streams(b));
    if (!b->d_slice_parts) ZG_HIP(lane_malloc((void **)&b->d_slice_parts, HOST_SLICES_MAX * 12 * 8));
    hipStream_t ss[zg_bases_s::NAUX + 1] = {st, b->aux[0], b->aux[1], b->aux[2]};
    ZG_HIP(hipEventRecord(b->ev_fork, st));
    for (int i = 0; i < zg_bases_s::NAUX; i++) ZG_HIP(hipStreamWaitEvent(b->aux[i], b->ev_fork, 0));
    const size_t per = (n + (size_t)slices - 1) / (size_t)slices;
    int rc = ZG_OK;
    hipError_t e = hipSuccess;
    for (int i = 0; i < slices && rc == ZG_OK && e == hipSuccess; i++) {
        size_t a = (size_t)i * per, cnt = a >= n ? 0 : (n - a < per ? n - a : per);
        hipStream_t si = ss[i % (zg_bases_s::NAUX + 1)];
        if (cnt) e = hipMemcpyAsync(b->d_scal + 4 * a, scalars + 4 * a, cnt * 32, hipMemcpyHostToDevice, si);
        // (an empty trailing slice — more slices than scalars, a test setting — still writes its identity record; its range is [off, off))
        if (e == hipSuccess) rc = msm_enqueue(b, cnt ? off + a : off, cnt, b->d_scal + 4 * (cnt ? a : 0), si, 2, b->d_slice_parts + 12 * (size_t)i, nullptr);
    }
    for (int i = 0; i < zg_bases_s::NAUX; i++) {  // join even after an error so the helpers never run ahead of the caller's next work
        hipError_t e1 = hipEventRecord(b->ev_join[i], b->aux[i]);
        if (e1 == hipSuccess) e1 = hipStreamWaitEvent(st, b->ev_join[i], 0);
        if (e == hipSuccess) e = e1;
    }
    if (rc == ZG_OK && e == hipSuccess) {
        hipLaunchKernelGGL(msm_combine_kernel, dim3(1), dim3(64), 0, st, b->d_slice_parts, (uint32_t)slices, 12u, b->d_out,
                           reinterpret_cast<uint8_t *>(b->d_out + 12), 0u, 0u, 2);  // Jacobian record: toAffine on the host (msm_to_host)
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(b->h_out, b->d_out, 12 * 8, hipMemcpyDeviceToHost, st);
    }
    hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (rc != ZG_OK) return rc;
    if (e != hipSuccess) {
        set_error(std::string("zg_msm_g1 (sliced): ") + hipGetErrorString(e));
        return ZG_ERR_HIP;
    }
    hostfp::jacobian_to_affine(b->h_out, out_xy, out_inf);
    return ZG_OK;
}

int zg_msm_g1(zg_bases_t b, size_t off, size_t n, const uint64_t *scalars, uint64_t out_xy[8], uint8_t *out_inf) {
    ZG_INIT();
    if (!b || !out_xy || (n && !scalars)) return invalid("zg_msm_g1: invalid argument");
    if (off + n > b->n) return invalid("msm: range exceeds uploaded bases");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    hipStream_t st = lib_stream();
    if (n && !b->d_scal) ZG_HIP(lane_malloc((void **)&b->d_scal, b->n * 32));
    int slices = env_int("ZG_MSM_HOST_SLICES", 3);  // 2^20 scalars: 2.32 ms unsliced, 2.20 / 2.15 / 2.20 / 2.30 / 2.45 with 2 / 3 / 4 / 6 / 8 slices
    if (slices > HOST_SLICES_MAX) slices = HOST_SLICES_MAX;
    if (slices >= 2 && n >= host_slice_min() && b->lanes.size() >= 2) return msm_host_sliced(b, off, n, scalars, slices, out_xy, out_inf);
    if (n) ZG_HIP(hipMemcpyAsync(b->d_scal, scalars, n * 32, hipMemcpyHostToDevice, st));
    return msm_to_host(b, off, n, b->d_scal, st, out_xy, out_inf);
}

// Scalars that are F.fromU64 of machine words — every polynomial `zolt prove` commits to (commitBytecode / commitMemory / commitRegisters,
// src/zkvm/mod.zig:1518-1617: program bytes, memory values, rd_value per cycle): 8 bytes per scalar cross PCIe instead of 32, the
// Montgomery conversion runs on the device (the reference spends a field multiplication per evaluation on the CPU for it), and since such
// a scalar has no digits above bit 64 the accumulation walks 4 of the 15 windows. Same bytes out as zg_msm_g1 on the converted vector.
int zg_msm_g1_u64(zg_bases_t b, size_t off, size_t n, const uint64_t *values, uint64_t out_xy[8], uint8_t *out_inf) {
    ZG_INIT();
    if (!b || !out_xy || (n && !values)) return invalid("zg_msm_g1_u64: invalid argument");
    if (off + n > b->n) return invalid("msm: range exceeds uploaded bases");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    hipStream_t st = lib_stream();
    if (n && !b->d_scal) ZG_HIP(lane_malloc((void **)&b->d_scal, b->n * 32));
    Staging sg(st);
    if (n) {
        const uint64_t *d_vals = sg.in(values, n * 8);
        if (sg.ok()) sg.adopt(ingest_u64_to_fr(d_vals, n, b->d_scal, st));
    }
    if (sg.ok()) sg.adopt(msm_to_host(b, off, n, b->d_scal, st, out_xy, out_inf));  // synchronises st before it returns
    return sg.finish_drained();
}

int zg_msm_g1_dev_async(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars, void *stream, uint64_t *d_out_xy,
                        uint8_t *d_out_inf) {
    ZG_INIT();
    if (!b || !d_out_xy || !d_out_inf || (n && !d_scalars)) return invalid("zg_msm_g1_dev_async: invalid argument");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_enqueue(b, off, n, d_scalars, pick_stream(stream), 0, d_out_xy, d_out_inf);
}

int zg_msm_g1_partial_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars, void *stream, uint64_t *d_out_jac) {
    ZG_INIT();
    if (!b || !d_out_jac || (n && !d_scalars)) return invalid("zg_msm_g1_partial_dev: invalid argument");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_enqueue(b, off, n, d_scalars, pick_stream(stream), 1, d_out_jac, nullptr);
}

int zg_msm_g1_partial_fast_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars, void *stream, uint64_t *d_out_jac) {
    ZG_INIT();
    if (!b || !d_out_jac || (n && !d_scalars)) return invalid("zg_msm_g1_partial_fast_dev: invalid argument");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_enqueue(b, off, n, d_scalars, pick_stream(stream), 2, d_out_jac, nullptr);
}

// Fused batches (fuse_set_size): the verdict for k vectors of n scalars, kept with the batch workspace so that a repeated batch of the same
// shape plans nothing. A verdict that fuses leaves the plan of a full set in `set` when it had to plan one (set.K == 0 otherwise).
static size_t batch_fuse(zg_bases_s *b, size_t n, size_t k, bool wide_ok, MsmPlan &set) {
    set.K = 0;
    if (!env_int("ZG_MSM_BATCH_FUSE", 1)) return 0;
    auto &f = b->fuse;
    if (f.n != n || f.k != k || f.wide_ok != wide_ok) {
        f.kc = fuse_set_size(b->plan, b->n, n, k, wide_ok, set);
        f.n = n;
        f.k = k;
        f.wide_ok = wide_ok;
    }
    return f.kc;
}

// Rows of a batch on a handle WITHOUT a table (G > 1: one bucket set per window) cannot share a sort (K * G * NB buckets leave the coarse
// counters' LDS), and as launch sets of their own each ends in its own reduction: row / column sums (0.24 ms), bit sums, msm_final and the
// window combine msm_groups_kernel — (G - 1) * c dependent doublings on one quad of lanes, 0.85 ms — all latency chains. HyperKZG.open's five
// long levels paid that five times, one after the other (9.1 ms per opening of 2^20 evaluations, 4.3 ms of it in msm_groups_kernel). Here
// every row is sorted and accumulated as a set of its own, its bucket sums land side by side in ONE array, and the reduction kernels run
// once over K * G groups (their grids already take a batch): the chains of all rows run beside each other.
static constexpr size_t ROWS_SHARED_TAIL_MAX = 16;
static bool rows_shared_tail_ok(const zg_bases_s *b, size_t n) {
    const MsmPlan &p = b->plan;
    if (p.G <= 1 || !p.lb || !env_int("ZG_MSM_ROWS_SHARED_TAIL", 1)) return false;
    size_t S, per;
    slice_counts(p, n, S, per);
    return S == 1;
}
static int msm_rows_shared_tail(zg_bases_s *b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out9) {
    const MsmPlan &p = b->plan;
    const size_t row_bytes = (size_t)p.NK * 144;  // p.K == 1: NK = G * NB
    const size_t per_group = bitsum_per_group(p);
    if (!b->rows_done) ZG_HIP(hipEventCreateWithFlags(&b->rows_done, hipEventDisableTiming));
    if (b->rows_cap < k) {
        if (b->rows_cap) ZG_HIP(hipEventSynchronize(b->rows_done));
        for (char **q : {&b->d_rows_buckets, &b->d_rows_bits, &b->d_rows_rg}) {
            pool_free(*q);
            *q = nullptr;
        }
        b->rows_cap = 0;
        ZG_HIP(lane_malloc((void **)&b->d_rows_buckets, k * row_bytes));
        ZG_HIP(lane_malloc((void **)&b->d_rows_bits, (size_t)p.G * k * per_group * 144));
        ZG_HIP(lane_malloc((void **)&b->d_rows_rg, (size_t)p.G * k * 128));
        b->rows_cap = k;
    } else {
        ZG_HIP(hipStreamWaitEvent(st, b->rows_done, 0));  // the previous batch may have run on another stream
    }
    int rc = ZG_OK;
    // row i ends at its bucket sums, in its part of the shared array (a bucket sink needs an unsliced launch: rows_shared_tail_ok)
    for (size_t i = 0; i < k && rc == ZG_OK; i++)
        rc = msm_enqueue(b, 0, n, d_scalars + 4 * n * i, st, 0, d_out9 + 9 * i, reinterpret_cast<uint8_t *>(d_out9 + 9 * i + 8),
                         b->d_rows_buckets + i * row_bytes);
    if (rc != ZG_OK) return rc;
    prof_begin(ZG_PROF_MSM_REDUCE, st);
    reduce_buckets(p, p.G * (int)k, b->d_rows_buckets, b->d_rows_bits, b->d_rows_rg, st, 0, d_out9, reinterpret_cast<uint8_t *>(d_out9 + 8), 9u, 72u);
    prof_end(ZG_PROF_MSM_REDUCE, st);
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipEventRecord(b->rows_done, st));
    return ZG_OK;
}

// enqueue k scalar vectors (device, back to back) over bases[0, n) on st. mode 0: record i = d_out9[9*i .. 9*i+8] (xy[8], flag
// word); mode 1 / 2: record i = 12 limbs at d_out9 + 12*i (Jacobian partial, normalised / any representative — see write_result).
// rows: the live lengths of the k zero-padded vectors (msm_batch_dev_wide), or nullptr. They reach exactly one kind of launch set, the
// fused set below that takes all k vectors at once; every other path walks the padded matrix.
static int msm_batch_enqueue(zg_bases_s *b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out9,
                             bool wide_ok = false, int mode = 0, const RowOffs *rows = nullptr /* the default walks the padded matrix */) {
    const uint32_t RS = mode == 0 ? 9u : 12u;  // record stride in u64
    auto inf_of = [&](size_t i) { return mode == 0 ? reinterpret_cast<uint8_t *>(d_out9 + RS * i + 8) : (uint8_t *)nullptr; };
    if (n > b->n) return invalid("msm: range exceeds uploaded bases");
    if (b->small && n <= b->small->n) return msm_batch_enqueue(b->small, n, d_scalars, k, st, d_out9, false, mode, rows);  // narrow-window side table
    MsmPlan set;
    const size_t kc = batch_fuse(b, n, k, wide_ok, set);
    if (kc == 0 && wide_ok && k >= 2 && k <= ROWS_SHARED_TAIL_MAX && mode == 0 && rows_shared_tail_ok(b, n)) return msm_rows_shared_tail(b, n, d_scalars, k, st, d_out9);
    if (kc == 0) {
        // one launch set per vector, rotating through the handle's workspaces AND through three streams (the caller's
        // plus two forked helpers), so the latency-bound tail of one MSM runs under the accumulation of the next
        bool fork = k >= 2 && n > 0 && b->lanes.size() >= 2;
        if (fork) ZG_TRY(ensure_aux_streams(b));
        if (fork) {
            ZG_HIP(hipEventRecord(b->ev_fork, st));
            for (int i = 0; i < zg_bases_s::NAUX; i++) ZG_HIP(hipStreamWaitEvent(b->aux[i], b->ev_fork, 0));
        }
        int rc = ZG_OK;
        for (size_t i = 0; i < k && rc == ZG_OK; i++) {
            hipStream_t si = !fork || i % (zg_bases_s::NAUX + 1) == 0 ? st : b->aux[i % (zg_bases_s::NAUX + 1) - 1];
            rc = msm_enqueue(b, 0, n, d_scalars + 4 * n * i, si, mode, d_out9 + RS * i, inf_of(i));
        }
        if (fork) {  // join even after an error so the helpers never run ahead of the caller's next work
            for (int i = 0; i < zg_bases_s::NAUX; i++) {
                ZG_HIP(hipEventRecord(b->ev_join[i], b->aux[i]));
                ZG_HIP(hipStreamWaitEvent(st, b->ev_join[i], 0));
            }
        }
        return rc;
    }
    const zg_msm_config cfg{b->plan.c, b->plan.L, 0};
    if (b->batch_n != n || (size_t)b->batch_plan.K < kc) {  // (re)build the fused workspace for kc vectors of n scalars
        if (b->batch_lane.done) {
            (void)hipEventSynchronize(b->batch_lane.done);
            lane_free(b->batch_lane);
        }
        b->batch_n = 0;
        if (set.K == 0) ZG_TRY(plan_msm(n, &cfg, kc, b->n, set));  // (the verdict was cached: plan the set now)
        b->batch_plan = set;
        hipError_t e = lane_alloc(b->batch_lane, b->batch_plan, n * kc);
        if (e != hipSuccess) {
            lane_free(b->batch_lane);
            set_error(std::string("msm batch workspace: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? ZG_ERR_NOMEM : ZG_ERR_HIP;
        }
        b->batch_n = n;
    }
    for (size_t i0 = 0; i0 < k; i0 += kc) {
        size_t kk = k - i0 < kc ? k - i0 : kc;
        MsmPlan pl = b->batch_plan;
        if (kk != (size_t)pl.K) ZG_TRY(plan_msm(n, &cfg, kk, b->n, pl, &b->batch_plan));  // a shorter last set: same workspace, same sort
        // live row lengths: only for THE set of all rows->k vectors (not one of several sets, not a shorter last set) that sorts by LDS
        // histograms (LDS, TWO_PASS; the global-atomic sort walks the padded matrix). K >= 2, so the set is never sliced (slice_counts).
        const RowOffs *live = rows && rows->k == (uint32_t)pl.K && pl.sort != MsmSort::ATOMIC ? rows : nullptr;
        ZG_TRY(msm_enqueue_lane(b, pl, b->batch_lane, 0, n, d_scalars + 4 * n * i0, st, mode, d_out9 + RS * i0, inf_of(i0), RS,
                                mode == 0 ? 72 : 0, live, nullptr));
    }
    return ZG_OK;
}

}  // extern "C"

namespace zg {
// zg_msm_g1_batch_dev for zero-padded rows of different live lengths (HyperKZG.open's long levels): also fuses on wide-window
// handles. Not exported: a general batch of full-length vectors on such a handle is better served by the stream rotation.
int msm_batch_dev_wide(zg_bases_t b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out9, const size_t *row_len) {
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    RowOffs rows{};
    if (row_len && k >= 2 && k <= 32) {  // row j is zero beyond row_len[j] <= n: the sort walks the live entries only
        rows.k = (uint32_t)k;
        for (size_t j = 0; j < k; j++) rows.off[j + 1] = rows.off[j] + (uint32_t)(row_len[j] < n ? row_len[j] : n);
    }
    return msm_batch_enqueue(b, n, d_scalars, k, st, d_out9, true, 0, rows.k ? &rows : nullptr);
}

// sharded.hip: this device's k partial sums of a sharded batch (BatchMSM over one shard of the bases), as un-normalised
// Jacobian records back to back (12 limbs each) — the batch form of zg_msm_g1_partial_fast_dev
int msm_batch_partials_dev(zg_bases_t b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out12) {
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_batch_enqueue(b, n, d_scalars, k, st, d_out12, false, 2);
}

// sharded.hip: combine `ranks` gathered partial records per scalar vector (rank r's k records back to back at
// d_partials + r * rank_stride) into k affine result records of 9 words (xy[8], flag)
int msm_combine_batch_enqueue(const uint64_t *d_partials, size_t ranks, size_t rank_stride, size_t k, hipStream_t st, uint64_t *d_out9) {
    if (k == 0) return ZG_OK;
    hipLaunchKernelGGL(msm_combine_kernel, dim3((unsigned)k), dim3(64), 0, st, d_partials, (uint32_t)ranks, (uint32_t)rank_stride, d_out9,
                       reinterpret_cast<uint8_t *>(d_out9 + 8), 9u, 72u);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int bases_device(zg_bases_t b) { return b ? b->device : -1; }
}  // namespace zg

extern "C" {

int zg_msm_g1_batch_dev(zg_bases_t b, size_t n, const uint64_t *d_scalars, size_t k, void *stream, uint64_t *d_out9) {
    ZG_INIT();
    if (!b || (k && (!d_out9 || (n && !d_scalars)))) return invalid("zg_msm_g1_batch_dev: invalid argument");
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    return msm_batch_enqueue(b, n, d_scalars, k, pick_stream(stream), d_out9);
}

int zg_msm_g1_batch(zg_bases_t b, size_t n, const uint64_t *const *batches, size_t k, uint64_t *out_xy, uint8_t *out_inf) {
    ZG_INIT();
    if (!b || (k && (!batches || !out_xy))) return invalid("zg_msm_g1_batch: invalid argument");
    if (n > b->n) return invalid("msm: range exceeds uploaded bases");
    if (k == 0) return ZG_OK;
    DeviceGuard dg(b->device);
    std::lock_guard<std::mutex> lk(b->mu);
    hipStream_t st = lib_stream();
    Staging sg(st);
    // the k vectors are staged back to back on the device; all results stay there until one final copy
    uint64_t *d_sc = sg.out<uint64_t>((n ? n : 1) * 32 * k), *d_res = sg.out<uint64_t>(9 * 8 * k);
    if (sg.ok()) ZG_STAGE(sg, hipMemsetAsync(d_res, 0, 9 * 8 * k, st));
    const bool routed_small = b->small && n <= b->small->n;
    MsmPlan set;
    if (sg.ok() && !routed_small && k >= 2 && n >= host_slice_min() && batch_fuse(b, n, k, false, set) == 0 && b->lanes.size() >= 2) {
        // long vectors (HyperKZG.batchCommit of full-size polynomials): vector i's copy and launch set go on stream i mod 3, so the
        // 32n-byte copy of the next vector runs under the MSM of the previous one instead of all k copies preceding all k MSMs
        if (sg.adopt(ensure_aux_streams(b))) {
            hipStream_t ss[zg_bases_s::NAUX + 1] = {st, b->aux[0], b->aux[1], b->aux[2]};
            ZG_STAGE(sg, hipEventRecord(b->ev_fork, st));
            for (int i = 0; i < zg_bases_s::NAUX && sg.ok(); i++) ZG_STAGE(sg, hipStreamWaitEvent(b->aux[i], b->ev_fork, 0));
            for (size_t i = 0; i < k && sg.ok(); i++) {
                hipStream_t si = ss[i % (zg_bases_s::NAUX + 1)];
                if (ZG_STAGE(sg, hipMemcpyAsync(d_sc + 4 * n * i, batches[i], n * 32, hipMemcpyHostToDevice, si)))
                    sg.adopt(msm_enqueue(b, 0, n, d_sc + 4 * n * i, si, 0, d_res + 9 * i, reinterpret_cast<uint8_t *>(d_res + 9 * i + 8)));
            }
            for (int i = 0; i < zg_bases_s::NAUX; i++) {  // join even after an error: sg waits for st alone
                hipError_t e = hipEventRecord(b->ev_join[i], b->aux[i]);
                if (e == hipSuccess) e = hipStreamWaitEvent(st, b->ev_join[i], 0);
                sg.check(e, "zg_msm_g1_batch: join of a helper stream");
            }
        }
    } else if (sg.ok()) {
        for (size_t i = 0; i < k && n && sg.ok(); i++) ZG_STAGE(sg, hipMemcpyAsync(d_sc + 4 * n * i, batches[i], n * 32, hipMemcpyHostToDevice, st));
        if (sg.ok()) sg.adopt(msm_batch_enqueue(b, n, d_sc, k, st, d_res));
    }
    std::vector<uint64_t> h_res(9 * k);
    sg.fetch(h_res.data(), d_res, 9 * 8 * k);
    if (sg.finish() != ZG_OK) return sg.rc;
    for (size_t i = 0; i < k; i++) {
        for (int j = 0; j < 8; j++) out_xy[8 * i + j] = h_res[9 * i + j];
        if (out_inf) out_inf[i] = (uint8_t)(h_res[9 * i + 8] & 0xff);
    }
    return ZG_OK;
}

int zg_g1_combine_partials_dev(const uint64_t *d_partials, size_t k, void *stream, uint64_t out_xy[8], uint8_t *out_inf) {
    ZG_INIT();
    if (!out_xy || (k && !d_partials)) return invalid("zg_g1_combine_partials_dev: invalid argument");
    Staging sg(pick_stream(stream));
    uint64_t *d_out = sg.out<uint64_t>(16 * 8);
    if (sg.ok()) {
        hipLaunchKernelGGL(msm_combine_kernel, dim3(1), dim3(64), 0, sg.st, d_partials, (uint32_t)k, 12u, d_out, reinterpret_cast<uint8_t *>(d_out + 8), 0u, 0u);
        sg.launched();
    }
    uint64_t h[9];
    sg.fetch(h, d_out, 9 * 8);
    if (sg.finish() != ZG_OK) return sg.rc;
    for (int i = 0; i < 8; i++) out_xy[i] = h[i];
    if (out_inf) *out_inf = (uint8_t)(h[8] & 0xff);
    return ZG_OK;
}

int zg_g1_combine_partials_dev_async(const uint64_t *d_partials, size_t k, void *stream, uint64_t *d_out_xy, uint8_t *d_out_inf) {
    ZG_INIT();
    if (!d_out_xy || !d_out_inf || (k && !d_partials)) return invalid("zg_g1_combine_partials_dev_async: invalid argument");
    hipLaunchKernelGGL(msm_combine_kernel, dim3(1), dim3(64), 0, pick_stream(stream), d_partials, (uint32_t)k, 12u, d_out_xy, d_out_inf, 0u, 0u);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int zg_g1_combine_partials_batch_dev_async(const uint64_t *d_partials, size_t ranks, size_t rank_stride, size_t m, void *stream, uint64_t *d_out9) {
    ZG_INIT();
    if ((m && (!d_partials || !d_out9)) || ranks == 0 || rank_stride < 12 * m || ranks > 0xffffffffu || rank_stride > 0xffffffffu)
        return invalid("zg_g1_combine_partials_batch_dev_async: invalid argument");
    return msm_combine_batch_enqueue(d_partials, ranks, rank_stride, m, pick_stream(stream), d_out9);
}

static FbPlan fb_plan(size_t n) {
    int c = n <= ((size_t)1 << 15) ? 8 : (n <= ((size_t)1 << 18) ? 10 : 11);
    int e = env_int("ZG_FB_WINDOW_BITS", 0);
    if (e >= 4 && e <= 14) c = e;
    return FbPlan{c, (254 + c - 1) / c, (1u << c) - 1u};
}

// the three launches of a fixed-base batch on st: window bases, table rows, n products (d_rows: W * 144 bytes, d_tab: W * rows * 64)
static void fb_enqueue(hipStream_t st, const FbPlan &fb, const uint64_t *d_base, char *d_rows, char *d_tab, const uint64_t *d_scalars, size_t n,
                       uint64_t *d_out_xy, uint8_t *d_out_inf) {
    const uint32_t n_rows = (uint32_t)fb.W * fb.rows;
    hipLaunchKernelGGL(fb_window_bases_kernel, dim3(1), dim3(4 * fb.W), 0, st, d_base, fb.c, d_rows);
    hipLaunchKernelGGL(fb_table_rows_kernel, dim3(div_up(n_rows, 256)), dim3(256), 0, st, d_rows, n_rows, fb.c, fb.rows, d_tab);
    hipLaunchKernelGGL(fb_mul_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_tab, d_scalars, n, fb.c, fb.W, fb.rows, d_out_xy, d_out_inf);
}

int zg_g1_fixed_base_mul_batch(const uint64_t base_xy[8], uint8_t base_inf, const uint64_t *scalars, size_t n, uint64_t *out_xy,
                               uint8_t *out_inf) {
    ZG_INIT();
    if (!base_xy || (n && (!scalars || !out_xy || !out_inf))) return invalid("zg_g1_fixed_base_mul_batch: invalid argument");
    if (n == 0) return ZG_OK;
    if (base_inf) {  // k * infinity = infinity (src/msm/mod.zig:504-506)
        memset(out_xy, 0, n * 64);
        memset(out_inf, 1, n);
        return ZG_OK;
    }
    const FbPlan fb = fb_plan(n);
    Staging sg(lib_stream());
    const uint64_t *d_base = sg.in(base_xy, 64), *d_sc = sg.in(scalars, n * 32);
    char *d_rows = sg.out<char>((size_t)fb.W * 144), *d_tab = sg.out<char>((size_t)fb.W * fb.rows * 64);
    uint64_t *d_out = sg.out<uint64_t>(n * 64);
    uint8_t *d_inf = sg.out<uint8_t>(n);
    if (sg.ok()) {
        fb_enqueue(sg.st, fb, d_base, d_rows, d_tab, d_sc, n, d_out, d_inf);
        sg.launched();
    }
    sg.fetch(out_xy, d_out, n * 64);
    sg.fetch(out_inf, d_inf, n);
    return sg.finish();
}

// HyperKZG.setup's G1 side on the device (generateMockSRS, src/poly/commitment/mod.zig:174-213: powers[i] = scalarMul(g1, tau^i)): the
// powers of tau, the fixed-base batch and the handle's table of multiples are built in HBM and stay there — the points cross PCIe only if
// the caller asks for them (out_xy). The compiled mirror spent 131 ms of a 2^20-cycle proof here (131 of 210 ms, tools/bench_prove_path):
// 2^20 host field products for the powers, 64 MB down, struct conversions, 64 MB up again.
int zg_hyperkzg_setup(const uint64_t base_xy[8], const uint64_t tau[4], size_t n, const zg_msm_config *cfg, uint64_t *out_xy, uint8_t *out_inf,
                      zg_bases_t *out) {
    ZG_INIT();
    if (!base_xy || !tau || !out || n >= ((size_t)1 << 27)) return invalid("zg_hyperkzg_setup: invalid argument (fewer than 2^27 powers, the most a handle holds)");
    const FbPlan fb = fb_plan(n);
    Staging sg(lib_stream());
    uint64_t *d_out = nullptr;
    uint8_t *d_inf = nullptr;
    if (n) {
        const uint64_t *d_base = sg.in(base_xy, 64);
        char *d_rows = sg.out<char>((size_t)fb.W * 144), *d_tab = sg.out<char>((size_t)fb.W * fb.rows * 64);
        uint64_t *d_pw = sg.out<uint64_t>(4 * 256 * 32), *d_sc = sg.out<uint64_t>(n * 32);
        d_out = sg.out<uint64_t>(n * 64);
        d_inf = sg.out<uint8_t>(n);
        if (sg.ok()) {
            hipLaunchKernelGGL(tau_tables_kernel, dim3(1), dim3(64), 0, sg.st, fe_arg(tau), d_pw);
            hipLaunchKernelGGL(tau_powers_kernel, dim3(div_up(n, 256)), dim3(256), 0, sg.st, d_pw, n, d_sc);
            fb_enqueue(sg.st, fb, d_base, d_rows, d_tab, d_sc, n, d_out, d_inf);
            sg.launched();
        }
        sg.fetch(out_xy, d_out, n * 64);
        sg.fetch(out_inf, d_inf, n);
    }
    // tau != 0: tau^i is never 0 mod r and the base has prime order, no power is the identity and the handle carries no infinity flags.
    // tau == 0 (canonical zero; the ABI accepts any field element): powers[i] = scalarMul(g1, 0) = identity for every i >= 1, as in the
    // reference — the flags fb_mul_kernel wrote travel into the handle, or its MSMs would take (0, 0) for a point (round-5 advisor)
    const bool tau_zero = !(tau[0] | tau[1] | tau[2] | tau[3]);
    // copies the points into the handle's table (and builds the side table beside it)
    if (sg.ok()) sg.adopt(bases_create(d_out, tau_zero ? d_inf : nullptr, n, cfg, sg.st, out));
    return sg.finish();
}

}  // extern "C"

namespace zg {
void fb_launch_shape(size_t n, uint32_t *out) {
    const FbPlan fb = fb_plan(n);
    out[0] = (uint32_t)fb.c;
    out[1] = (uint32_t)fb.W;
    out[2] = fb.rows;
}
}  // namespace zg
