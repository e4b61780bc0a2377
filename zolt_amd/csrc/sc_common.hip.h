// sc_common.hip.h — what the sumcheck kernels of poly.hip, psc.hip, rwc.hip and rrw.hip share: wave / block reductions of Fr pairs, the
// pinned-mailbox publication, and the end of a round — block partials, the hand-off to the last workgroup, the finish launch.
#pragma once
#include "common.hip.h"
#include "field.hip.h"
#include "fp29.hip.h"
#include "acc9.hip.h"

namespace zg {

typedef __attribute__((address_space(1))) uint64_t sc_gu64;
typedef __attribute__((address_space(1))) uint32_t sc_gu32;

ZG_DEV Fr fr_shfl_down(const Fr &v, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = __shfl_down(v.l[i], d, 64);
    return r;
}
ZG_DEV bool fr_eq(const Fr &a, const Fr &b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.l[i] ^ b.l[i];
    return d == 0;
}

template <int CTRL, int ROW_MASK>
ZG_DEV u32 dpp_take(u32 v) {  // lanes without a source (or outside ROW_MASK) read 0
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
// x += (x moved across lanes by a DPP control), nine limbs with the carry chain, the lane movement folded INTO the additions
// (v_add_co_u32_dpp / v_addc_co_u32_dpp): nine instructions. Left to the compiler the same step was a v_mov_b32_dpp, a hazard s_nop
// and a v_addc per limb (27). Lanes without a source add 0 (bound_ctrl), lanes of rows outside the row mask are not written.
// Hazards: a DPP read needs two wait states after a VALU write of the same register — inside the sequence every source limb was
// written nine instructions earlier; the leading s_nop 1 covers whatever the compiler scheduled in front.
#define ZG_ACC9_DPP_ADD(NAME, CTRL_TEXT)                                                                                              \
    ZG_DEV void NAME(Acc9 &x) {                                                                                                       \
        asm volatile("s_nop 1\n\t"                                                                                                    \
                     "v_add_co_u32_dpp %0, vcc, %0, %0 " CTRL_TEXT "\n\t"                                                             \
                     "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %2, vcc, %2, %2, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %3, vcc, %3, %3, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %4, vcc, %4, %4, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %5, vcc, %5, %5, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %6, vcc, %6, %6, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %7, vcc, %7, %7, vcc " CTRL_TEXT "\n\t"                                                       \
                     "v_addc_co_u32_dpp %8, vcc, %8, %8, vcc " CTRL_TEXT "\n\t"                                                       \
                     : "+v"(x.l[0]), "+v"(x.l[1]), "+v"(x.l[2]), "+v"(x.l[3]), "+v"(x.l[4]), "+v"(x.l[5]), "+v"(x.l[6]), "+v"(x.l[7]),  \
                       "+v"(x.l[8])                                                                                                   \
                     :                                                                                                                \
                     : "vcc");                                                                                                        \
    }
ZG_ACC9_DPP_ADD(acc9_row_shr1_add, "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
ZG_ACC9_DPP_ADD(acc9_row_shr2_add, "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
ZG_ACC9_DPP_ADD(acc9_row_shr4_add, "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
ZG_ACC9_DPP_ADD(acc9_row_shr8_add, "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
ZG_ACC9_DPP_ADD(acc9_row_bcast15_add, "row_bcast:15 row_mask:0xa bank_mask:0xf")  // rows 1 and 3 += lane 15 of the row before
#undef ZG_ACC9_DPP_ADD
// x += x shifted right by N lanes inside each row of 16 (lanes without a source add 0)
template <int N>
ZG_DEV void acc9_row_shr_add(Acc9 &x) {
    if (N == 1) acc9_row_shr1_add(x);
    else if (N == 2) acc9_row_shr2_add(x);
    else if (N == 4) acc9_row_shr4_add(x);
    else acc9_row_shr8_add(x);
}

// Sum of (g0, g1) over a wavefront without LDS traffic: one v_permlane32_swap per limb puts the g0 halves on lanes 0-31 and the g1
// halves on lanes 32-63 (one addition then serves both sums), four row_shr steps inside the rows of 16 and one row_bcast:15 step
// across the row pair. On return lane 31 holds the wave's g0 total and lane 63 its g1 total (in `g0`; g1 is scratch).
ZG_DEV void wave_sum_pair9(Acc9 &g0, Acc9 &g1) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        auto sw = __builtin_amdgcn_permlane32_swap(g0.l[i], g1.l[i], false, false);
        g0.l[i] = sw[0];
        g1.l[i] = sw[1];
    }
    acc9_add_acc(g0, g1);
    acc9_row_shr_add<1>(g0);
    acc9_row_shr_add<2>(g0);
    acc9_row_shr_add<4>(g0);
    acc9_row_shr_add<8>(g0);
    acc9_row_bcast15_add(g0);  // rows 1 and 3 += lane 15 of rows 0 and 2
}

// Block-wide sum of (g0, g1) (a multiple of 64 threads, at most 1024). `sh`: SC_RED_WORDS u32 of LDS. On return, in wave 0, lane
// SC_LANE_G0 holds the canonical g0 total and lane SC_LANE_G1 the canonical g1 total (both in the returned value; other lanes hold
// nothing useful). One barrier; the caller must put a barrier between two uses of the same `sh`.
constexpr u32 SC_RED_WORDS = 16 * 2 * 9, SC_LANE_G0 = 15, SC_LANE_G1 = 47;
ZG_DEV Fr block_sum_pair9(Acc9 g0, Acc9 g1, u32 *sh) {
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nwaves = blockDim.x >> 6;
    wave_sum_pair9(g0, g1);
    if (nwaves > 1) {
        if ((lane & 31u) == 31u) {
            u32 *dst = sh + (wave * 2 + (lane >> 5)) * 9;
#pragma unroll
            for (int i = 0; i < 9; i++) dst[i] = g0.l[i];
        }
        __syncthreads();
        if (wave != 0) return Fr::zero();
        // lanes 0..nwaves-1 (row 0) take the waves' g0 totals, lanes 32..32+nwaves-1 (row 2) their g1 totals
        const u32 w = lane & 31u;
        g0 = acc9_zero();
        if (w < nwaves) {
            const u32 *src = sh + (w * 2 + (lane >> 5)) * 9;
#pragma unroll
            for (int i = 0; i < 9; i++) g0.l[i] = src[i];
        }
        acc9_row_shr_add<1>(g0);
        acc9_row_shr_add<2>(g0);
        if (nwaves > 4) {
            acc9_row_shr_add<4>(g0);
            acc9_row_shr_add<8>(g0);
        } else {  // totals sit on lanes 3 / 35: move them to lanes 15 / 47 (row_shr:12)
#pragma unroll
            for (int i = 0; i < 9; i++) g0.l[i] = dpp_take<0x110 + 12, 0xf>(g0.l[i]);
        }
    } else {  // one wave: totals on lanes 31 / 63 -> lanes 15 / 47 (row_shr... crosses rows: read them through a shuffle)
#pragma unroll
        for (int i = 0; i < 9; i++) g0.l[i] = __shfl(g0.l[i], (int)((lane & 32u) | 31u), 64);
    }
    return acc9_reduce(g0);
}
// wave 0 only: lane SC_LANE_G0 also receives lane SC_LANE_G1's value (the pair in one lane for a verifier step / mailbox store)
ZG_DEV Fr pair_second_to_first(const Fr &v) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = __shfl(v.l[i], (int)SC_LANE_G1, 64);
    return r;
}

// A kernel that produces the final values of a round publishes them to the pinned host mailbox (hipHostMalloc, mapped + coherent:
// uncached on the device): values first as write-through system-scope stores, the wave's s_waitcnt vmcnt(0), then the round's sequence
// number, so the host can spin on the mailbox instead of paying a stream synchronisation per round. No release fence: round 3's
// __threadfence_system() here was a buffer_wbl2 — a write-back of the XCD's L2 right behind the fold that had just dirtied it — and the
// mailbox never sits in that L2. flag == nullptr: the values go to device memory with plain stores (read by a later launch or copy).
ZG_DEV void mailbox_store_fr(uint64_t *dst, const Fr &v, const uint64_t *flag) {
    if (flag) {
        sc_gu64 *d = (sc_gu64 *)dst;
#pragma unroll
        for (int i = 0; i < 4; i++)
            __hip_atomic_store(d + i, (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        fe_store(dst, v);
    }
}
ZG_DEV void publish_seq(uint64_t *flag, uint64_t seq) {  // by a lane of the wave that stored the values
    if (flag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store((sc_gu64 *)flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The same for two canonical values per thread. block_sum_fr returns the totals where block_sum_pair9 leaves them; block_sum_pair
// overwrites g0 and g1 with both totals in every lane of wave 0. `sh`: SC_RED_WORDS u32; a barrier between two calls that share it.
ZG_DEV Fr block_sum_fr(const Fr &g0, const Fr &g1, u32 *sh) {
    Acc9 a0 = acc9_zero(), a1 = acc9_zero();
    acc9_add(a0, g0);
    acc9_add(a1, g1);
    return block_sum_pair9(a0, a1, sh);
}
ZG_DEV void block_sum_pair(Fr &g0, Fr &g1, u32 *sh) {
    Fr tot = block_sum_fr(g0, g1, sh);
    if (threadIdx.x < 64) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            g0.l[i] = __shfl(tot.l[i], (int)SC_LANE_G0, 64);
            g1.l[i] = __shfl(tot.l[i], (int)SC_LANE_G1, 64);
        }
    }
}

// The block's NV sums (canonical Fr or lazy Acc9 per thread) to partials[blockIdx][NV] with plain stores, by the two lanes of wave 0
// that hold a pair's totals: read by a later launch (sc_finish_kernel).
ZG_DEV Acc9 acc9_of(const Acc9 &a) { return a; }
ZG_DEV Acc9 acc9_of(const Fr &v) {
    Acc9 a = acc9_zero();
    acc9_add(a, v);
    return a;
}
template <int NV, class T>
ZG_DEV void block_store_sums(const T (&acc)[NV], u32 *sh, uint64_t *partials) {
    const u32 lane = threadIdx.x & 63u;
#pragma unroll
    for (int a = 0; a < NV; a += 2) {
        if (a) __syncthreads();
        const T &odd = acc[a + 1 < NV ? a + 1 : a];
        const Fr tot = block_sum_pair9(acc9_of(acc[a]), a + 1 < NV ? acc9_of(odd) : acc9_zero(), sh);
        if (threadIdx.x < 64 && (lane == SC_LANE_G0 || (lane == SC_LANE_G1 && a + 1 < NV)))
            fe_store(partials + 4 * ((size_t)blockIdx.x * NV + a + (lane == SC_LANE_G1 ? 1 : 0)), tot);
    }
}

// ---- hand-off of a workgroup's partial sums to the workgroup that finishes the round (MI355X_MICROARCH.md, inter-workgroup
// visibility, "hand-offs measured with sc1 loads", first row): the partials are written with write-through (sc1) stores by ONE wave,
// that wave drains them (s_waitcnt vmcnt(0)), then ONE of its lanes adds to the arrival counter with a RELAXED agent-scope atomic;
// the workgroup whose add returns the last ticket reads the partials with sc1 loads (they bypass its L1; no line of the partials
// buffer is ever loaded any other way inside a launch). No release fence and no per-workgroup acquire: round 3's ACQ_REL arrival wrote
// back and invalidated the XCD's L2 behind a freshly written table once per workgroup. The LAST arriver alone runs one agent-scope
// acquire per launch (sc_arrive), on both arrival paths.
ZG_DEV void sc1_store_fr(uint64_t *dst, const Fr &v) {
    sc_gu64 *d = (sc_gu64 *)dst;
#pragma unroll
    for (int i = 0; i < 4; i++)
        __hip_atomic_store(d + i, (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
ZG_DEV Fr sc1_load_fr(const uint64_t *src) {
    const sc_gu64 *p = (const sc_gu64 *)src;
    Fr r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint64_t w = __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.l[2 * i] = (uint32_t)w;
        r.l[2 * i + 1] = (uint32_t)(w >> 32);
    }
    return r;
}
ZG_DEV void sc_drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Arrival (called by ONE lane, after the storing wave's sc_drain_stores()); true in the workgroup that arrives last. Up to
// SC_ARRIVE_FLAT workgroups add to one counter (the table row above, literally: the last adder is told by the value its add returned;
// 255 -> 1 arrivals cost ~3 us when they all come at once). Larger grids arrive in two levels — 16 counters on lines of their own
// (blockIdx mod 16), the last arrival of each line moves on to the top counter — which is outside that row, so the final arriver
// runs ONE agent-scope acquire (then s_waitcnt vmcnt(0); the caller's barrier follows) before anyone loads: the guide's "consumer,
// always" form, with the sc1 stores standing in for the release. Every counter is left at zero for the next launch (stream order).
constexpr uint32_t SC_ARRIVE_FLAT = 256, SC_ARRIVE_LINES = 16, SC_ARRIVE_STRIDE = 32;  // uint32 words between counters (128 bytes)
constexpr size_t SC_COUNTER_BYTES = 128 * (1 + SC_ARRIVE_LINES);
// scratch layout of a fold/sums launch (u64 words): [0, 8*SC_MAX_BLOCKS) block pairs | SC_COUNTER_BYTES: arrival counters (sc_arrive)
// (must be 0 before a launch; the kernels re-arm it) | 8 words: the round's pair when it is not sent to a host mailbox
constexpr unsigned SC_MAX_BLOCKS = 2048;
constexpr size_t SC_SUMS_OFF = 8 * (size_t)SC_MAX_BLOCKS + SC_COUNTER_BYTES / 8;
constexpr size_t SC_MISC_BYTES = (SC_SUMS_OFF + 8) * 8;
ZG_DEV bool sc_arrive(uint32_t *counter, uint32_t nb) {
    sc_gu32 *c = (sc_gu32 *)counter;
    if (nb <= SC_ARRIVE_FLAT) {
        if (__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nb - 1) return false;
        __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ONE agent-scope acquire per launch, in the last arriver only (round-4 advisor finding: the flat path relied on the measured
        // table row alone, the two-level path fenced). The fence is `s_waitcnt vmcnt(0); buffer_inv sc1`: the invalidate is queued in
        // front of every later vector-memory instruction of this wave, the other waves load after the caller's barrier.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        return true;
    }
    const uint32_t line = blockIdx.x % SC_ARRIVE_LINES;
    const uint32_t members = (nb - line + SC_ARRIVE_LINES - 1) / SC_ARRIVE_LINES;  // workgroups b < nb with b mod 16 == line
    sc_gu32 *lc = c + SC_ARRIVE_STRIDE * (1 + line);
    if (__hip_atomic_fetch_add(lc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return false;
    __hip_atomic_store(lc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != SC_ARRIVE_LINES - 1) return false;
    __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

// The hand-off itself, for NP pairs per workgroup. tot[p]: block_sum_pair9's return for the block's values 2p and 2p + 1 (wave 0,
// lanes SC_LANE_G0 / SC_LANE_G1), stored to partials[blockIdx][2 NP] by those two lanes. Called by every thread of every workgroup
// (more than one). False in every workgroup but the one that arrived last; there, take(k, a, v) has been called for value a of every
// workgroup k (the k strided over the threads) when it returns true.
template <int NP, class Take>
ZG_DEV bool sc_hand_off(const Fr (&tot)[NP], uint64_t *partials, uint32_t *counter, Take take) {
    const uint32_t tid = threadIdx.x, nb = gridDim.x, lane = tid & 63u;
    __shared__ uint32_t last;
    if (tid < 64) {
        if (lane == SC_LANE_G0 || lane == SC_LANE_G1) {
#pragma unroll
            for (int p = 0; p < NP; p++) sc1_store_fr(partials + 8 * ((size_t)blockIdx.x * NP + p) + (lane == SC_LANE_G1 ? 4 : 0), tot[p]);
        }
        sc_drain_stores();  // the one storing wave, before its lane signals
        if (lane == SC_LANE_G0) last = sc_arrive(counter, nb) ? 1u : 0u;
    }
    __syncthreads();  // (also orders a block reduction's LDS reads before the caller reuses its scratch)
    if (!last) return false;
    for (uint32_t k = tid; k < nb; k += blockDim.x) {
#pragma unroll
        for (int a = 0; a < 2 * NP; a++) take(k, a, sc1_load_fr(partials + 4 * ((size_t)k * 2 * NP + a)));
    }
    return true;
}
// End of a round inside the producing kernel (no second launch): the hand-off above, then the workgroup that arrived last adds all
// pairs up (lazy sums), writes the round's 2 NP values to `sums` (the pinned host mailbox) and publishes the sequence word. A grid of
// one workgroup publishes its own totals. `sh`: SC_RED_WORDS u32, free (behind a barrier or unused) on entry.
template <int NP>
ZG_DEV void sc_round_end(Fr (&tot)[NP], u32 *sh, uint64_t *partials, uint64_t *sums, uint32_t *counter, uint64_t *flag, uint64_t seq) {
    if (gridDim.x > 1) {
        Acc9 acc[2 * NP];
#pragma unroll
        for (int a = 0; a < 2 * NP; a++) acc[a] = acc9_zero();
        if (!sc_hand_off<NP>(tot, partials, counter, [&](uint32_t, int a, const Fr &v) { acc9_add(acc[a], v); })) return;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (p) __syncthreads();
            tot[p] = block_sum_pair9(acc[2 * p], acc[2 * p + 1], sh);
        }
    }
    if (threadIdx.x < 64) {
        Fr second[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) second[p] = pair_second_to_first(tot[p]);
        if ((threadIdx.x & 63u) == SC_LANE_G0) {
#pragma unroll
            for (int p = 0; p < NP; p++) {
                mailbox_store_fr(sums + 8 * p, tot[p], flag);
                mailbox_store_fr(sums + 8 * p + 4, second[p], flag);
            }
            publish_seq(flag, seq);
        }
    }
}

// End of a round in a launch of its own: out[a] = sum over b < nblocks of partials[b][a] for a < nv (the layout block_store_sums
// writes; a kernel that leaves one value per thread has nblocks = threads / nv). A workgroup takes the values two at a time, the
// workgroups of a grid share the pairs: one workgroup for a session's few values, div_up(nv, 2) for one pair each. With `flag` (one
// workgroup only) `out` is the pinned mailbox and the sequence word follows the values. A template (launched as sc_finish_kernel<>),
// like fr_fold_vec_kernel below, so that only the translation units that launch it carry a copy.
template <int = 0>
__global__ void __launch_bounds__(256) sc_finish_kernel(const uint64_t *partials, uint32_t nblocks, uint32_t nv, uint64_t *out, uint64_t *flag,
                                                               uint64_t seq) {
    __shared__ u32 sh[SC_RED_WORDS];
    const u32 lane = threadIdx.x & 63u;
    for (uint32_t a = 2 * blockIdx.x; a < nv; a += 2 * gridDim.x) {
        const bool two = a + 1 < nv;
        Acc9 g0 = acc9_zero(), g1 = acc9_zero();
        for (uint32_t b = threadIdx.x; b < nblocks; b += 256) {
            const uint64_t *src = partials + 4 * ((size_t)b * nv + a);
            acc9_add(g0, fe_load<FrParams>(src));
            if (two) acc9_add(g1, fe_load<FrParams>(src + 4));
        }
        const Fr tot = block_sum_pair9(g0, g1, sh);
        if (threadIdx.x < 64 && (lane == SC_LANE_G0 || (lane == SC_LANE_G1 && two))) mailbox_store_fr(out + 4 * (a + (lane == SC_LANE_G1 ? 1 : 0)), tot, flag);
        __syncthreads();
    }
    if (threadIdx.x == SC_LANE_G0) publish_seq(flag, seq);  // its s_waitcnt covers the wave's stores, the other lane's included
}

// The host side of that launch for a session with a device slot and a pinned buffer: the nv sums of the nblocks block partials at
// d_part arrive in h_out[0, 4 nv) — with d_extra, four more bytes of device memory in the word behind them — under one synchronisation.
template <int = 0>  // (as the kernel it launches: instantiated where it is called)
static inline int sc_collect(hipStream_t st, const uint64_t *d_part, uint32_t nblocks, uint32_t nv, uint64_t *d_out, uint64_t *h_out,
                             const void *d_extra = nullptr) {
    hipLaunchKernelGGL(sc_finish_kernel<>, dim3(1), dim3(256), 0, st, d_part, nblocks, nv, d_out, (uint64_t *)nullptr, (uint64_t)0);
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipMemcpyAsync(h_out, d_out, (size_t)nv * 32, hipMemcpyDeviceToHost, st));
    if (d_extra) ZG_HIP(hipMemcpyAsync(h_out + 4 * nv, d_extra, 4, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}

// LowToHigh fold of one or two vectors by one challenge: out[i] = t[2i] + r (t[2i+1] - t[2i])
ZG_DEV Fr fr_fold1(const Fr &lo, const Fr &hi, const FrMul &rm) {
    Fr d = fe_sub(hi, lo);
    if (d.is_zero()) return lo;  // (also every pair of zeros of a one-hot table)
    return fe_add(lo, frmul_apply(d, rm));
}
template <int = 0>
__global__ void __launch_bounds__(256) fr_fold_vec_kernel(const uint64_t *a, uint64_t *a_out, const uint64_t *b, uint64_t *b_out, size_t half, FeArg r_a) {
    const FrMul rm = frmul_prepare(fe_from_arg<FrParams>(r_a));
    size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < half; i += step) {
        fe_store(a_out + 4 * i, fr_fold1(fe_load<FrParams>(a + 8 * i), fe_load<FrParams>(a + 8 * i + 4), rm));
        if (b) fe_store(b_out + 4 * i, fr_fold1(fe_load<FrParams>(b + 8 * i), fe_load<FrParams>(b + 8 * i + 4), rm));
    }
}

}  // namespace zg
