// hyperkzg.hip — HyperKZG.open and batchOpen on gfx950: the quotient / fold chain of an opening, the commits of its quotients, and
// batchOpen's random linear combination. The level plan behind the chain and the commits is hk_plan.h.
//
// Reference functions replaced (paths in the reference's tree):
//   HyperKZG.open        src/poly/commitment/mod.zig:261-324
//   HyperKZG.batchOpen   src/poly/commitment/mod.zig:607-732
#include <utility>
#include <vector>

#include "common.hip.h"
#include "field.hip.h"
#include "fp29.hip.h"
#include "hk_plan.h"
#include "sc_common.hip.h"

namespace zg {

// One level of HyperKZG.open (src/poly/commitment/mod.zig:296-310) in one pass over the table: the quotient
// q[j] = t[j + half] - t[j] (the first q_count entries are kept: commit() uses min(half, srs_len) of them) and the fold
// out[j] = (1 - r) t[j] + r t[j + half] = t[j] + r q[j]. It replaces a quotient launch plus a fold launch that also produced round
// sums nobody reads, and stays below the 112 registers per SIMD that a resident bucket accumulation leaves free: the open's serial
// quotient -> fold chain then runs beside the commits of the earlier levels instead of waiting for their workgroups to retire.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(56))) hk_quot_fold_kernel(const uint64_t *t, size_t half, FeArg r, uint64_t *q,
                                                                                               size_t q_count, uint64_t *out) {
    __builtin_amdgcn_s_setprio(3);
    const Fr rv = fe_from_arg<FrParams>(r);
    FrMul rp = frmul_prepare(rv);
    size_t stride = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < half; j += stride) {
        Fr lo = fe_load<FrParams>(t + 4 * j), hi = fe_load<FrParams>(t + 4 * (j + half));
        Fr d = fe_sub(hi, lo);
        if (j < q_count) fe_store(q + 4 * j, d);
        fe_store(out + 4 * j, fe_add(lo, frmul_apply(d, rp)));
    }
}

// workgroups of one level of HyperKZG.open (hk_quot_fold_kernel, 256 threads, grid-stride) over `half` pairs: one pair per thread up to 1024
unsigned hk_fold_grid(size_t half) {
    const unsigned cap = sc_block_cap(1024u), b = div_up(half ? half : 1, 256);
    return b > cap ? cap : b;
}

}  // namespace zg

using namespace zg;

extern "C" {

// The fold / quotient / commit loop of HyperKZG.open and batchOpen (src/poly/commitment/mod.zig:283-317, :684-712) on a table
// already resident at d_a (n_evals entries; d_a, d_b: ping-pong buffers of >= n_evals and n_evals/2 entries).
// Quotient i is commit(cur[half..] - cur[..half]); levels the fold cannot reach (half == 0, :289 / :686) are reported as
// identity and not counted in *n_quot. Where each level's quotient goes and which commits take it is hk_plan's decision (hk_plan.h).
// The caller's Staging carries the table buffers; the loop's own scratch joins them, and the call ends in sg's wait.
static int hk_open_device(Staging &sg, zg_bases_t srs, uint64_t *d_a, uint64_t *d_b, size_t n_evals, const uint64_t *point, size_t num_vars,
                          uint64_t *q_xy, uint8_t *q_inf, uint64_t final_eval[4], size_t *n_quot) {
    hipStream_t st = sg.st;
    // The commits are independent of the folds that follow them: every quotient has its own place in the arena and the MSMs are
    // issued on three helper streams (forked / joined by events), never on the caller's stream, so the latency-bound tail of one
    // commit runs under the accumulation of the next.
    constexpr int NAUX = 3;
    // the helper streams belong to THIS call: a GROUP taken from the runtime's per-device free list (creating a stream costs ~3 ms) and
    // handed back on return, so concurrent opens from different caller threads do not serialise through a shared set (round-2 review).
    // A group's streams were created back to back and therefore sit on different hardware queues (HIP hands its four queues out in
    // creation order): three streams taken one by one from the common free list put the first long level and the fused long levels
    // on ONE queue in a trace of round 4 — the two launch sets that are meant to overlap ran one after the other (2.69 ms per open).
    struct AuxStreams {
        hipStream_t s[NAUX] = {nullptr, nullptr, nullptr};
        int dev;
        AuxStreams() : dev(current_device()) { (void)stream_group_acquire(s); }
        ~AuxStreams() {
            if (s[0]) stream_group_release(s, dev);
        }
    } aux_streams;
    hipStream_t *aux = aux_streams.s;
    const bool fork = aux[0] && aux[1] && aux[2];
    const HkPlan p = hk_plan(n_evals, num_vars, zg_g1_bases_len(srs), env_uint("ZG_HK_FUSE_LONG", 1, 0, 2), fork);  // read per call: tests switch it
    std::vector<hipEvent_t> events;
    struct EventGuard {
        std::vector<hipEvent_t> &ev;
        ~EventGuard() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    } guard{events};
    uint64_t *d_res = sg.out<uint64_t>((9 * num_vars + 4) * 8), *d_misc = sg.out<uint64_t>(SC_MISC_BYTES),
             *d_q = sg.out<uint64_t>((p.arena + 1) * 32);  // the quotient arena
    // an event recorded on s (nullptr: the failure is sg's)
    auto mark = [&](hipStream_t s) -> hipEvent_t {
        hipEvent_t ev = nullptr;
        if (!ZG_STAGE(sg, hipEventCreateWithFlags(&ev, hipEventDisableTiming))) return nullptr;
        events.push_back(ev);
        return ZG_STAGE(sg, hipEventRecord(ev, s)) ? ev : nullptr;
    };
    if (sg.ok()) ZG_STAGE(sg, hipMemsetAsync(d_res, 0, (9 * num_vars + 4) * 8, st));
    if (sg.ok()) ZG_STAGE(sg, hipMemsetAsync(d_misc + 8 * (size_t)SC_MAX_BLOCKS, 0, SC_COUNTER_BYTES, st));
    for (const HkMatrix *m : {&p.small, &p.lng})  // a row keeps zeros beyond the entries its fold writes
        if (sg.ok() && m->rows) ZG_STAGE(sg, hipMemsetAsync(d_q + 4 * m->off, 0, m->entries() * 32, st));
    // 1. The fold chain, on the caller's stream. The whole chain is enqueued (and, being a few short kernels, finished) before the first
    // commit starts: kernels of different streams share the dispatch pipes, and a commit's sort kernels (whole-CU workgroups that launch
    // as accumulate workgroups retire) held the chain's next link back by 0.5-1 ms per level when both were in flight.
    uint64_t *cur = d_a, *nxt = d_b;
    for (size_t i = 0; i < p.computed && sg.ok(); i++) {
        const HkLevel &l = p.level[i];
        hipLaunchKernelGGL(hk_quot_fold_kernel, dim3(hk_fold_grid(l.half)), dim3(256), 0, st, cur, l.half, fe_arg(point + 4 * i), d_q + 4 * l.off, l.count, nxt);
        std::swap(cur, nxt);
    }
    // 2. The commits. Helper a waits for the end of the chain before its first commit; without helper streams (no group could be
    // taken) every commit follows the chain on the caller's stream.
    bool aux_used[NAUX] = {false, false, false};
    hipEvent_t chain_end = nullptr;
    auto helper = [&](int a) -> hipStream_t {  // nullptr: the failure is sg's
        if (!fork) return st;
        if (!aux_used[a]) {
            if (!chain_end) chain_end = mark(st);
            if (!chain_end || !ZG_STAGE(sg, hipStreamWaitEvent(aux[a], chain_end, 0))) return nullptr;
            aux_used[a] = true;
        }
        return aux[a];
    };
    // The short levels' fused commit depends on the chain only: it runs beside the long commits, on the group's third stream (the
    // caller's stream may share a hardware queue with one of the helpers; it only carries the chain, the joins and the result copy),
    // and it is enqueued FIRST: its short kernels start right behind the chain and are done before the long levels' accumulation needs
    // the chip (enqueued last, they ran under that accumulation's sort and stretched it: 616 -> 531 us in the trace of 2^20 evaluations).
    if (sg.ok() && p.small.rows)
        if (hipStream_t s = helper(NAUX - 1)) sg.adopt(zg_msm_g1_batch_dev(srs, p.small.len, d_q + 4 * p.small.off, p.small.rows, s, d_res + 9 * p.small.first));
    // the levels with a buffer of their own go out on the three helper streams in turn, largest first
    for (size_t i = 0, k = 0; i < p.computed && sg.ok(); i++) {
        const HkLevel &l = p.level[i];
        if (l.dest != HkDest::OWN) continue;
        if (hipStream_t s = helper((int)(k++ % NAUX)))
            sg.adopt(zg_msm_g1_dev_async(srs, 0, l.nc, d_q + 4 * l.off, s, d_res + 9 * i, reinterpret_cast<uint8_t *>(d_res + 9 * i + 8)));
    }
    if (sg.ok() && p.lng.rows)  // mode 2: the lone first level took helper 0
        if (hipStream_t s = helper(p.lng.first ? 1 : 0))
            sg.adopt(msm_batch_dev_wide(srs, p.lng.len, d_q + 4 * p.lng.off, p.lng.rows, s, d_res + 9 * p.lng.first, p.long_row_len));
    // 3. The join, the final value, the results.
    for (int a = 0; a < NAUX; a++)  // join the helper streams (also after an error, so that they never run ahead of later work)
        if (aux_used[a]) {
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
                events.push_back(ev);
                if (hipEventRecord(ev, aux[a]) == hipSuccess) (void)hipStreamWaitEvent(st, ev, 0);
            } else {
                (void)hipStreamSynchronize(aux[a]);
            }
        }
    if (sg.ok() && n_evals) ZG_STAGE(sg, hipMemcpyAsync(d_res + 9 * num_vars, cur, 32, hipMemcpyDeviceToDevice, st));  // final = current[0], :317
    std::vector<uint64_t> dev_res(9 * num_vars + 4);
    sg.fetch(dev_res.data(), d_res, (9 * num_vars + 4) * 8);
    if (sg.finish() != ZG_OK) return sg.rc;
    for (size_t i = 0; i < num_vars; i++) {
        const bool skipped = i >= p.computed;  // the reference stops folding; the remaining quotients stay unset -> identity here
        for (int j = 0; j < 8; j++) q_xy[8 * i + j] = skipped ? 0 : dev_res[9 * i + j];
        if (q_inf) q_inf[i] = skipped ? 1 : (uint8_t)(dev_res[9 * i + 8] & 0xff);
    }
    for (int j = 0; j < 4; j++) final_eval[j] = n_evals ? dev_res[9 * num_vars + j] : 0;
    if (n_quot) *n_quot = p.computed;
    return ZG_OK;
}

int zg_hyperkzg_open(zg_bases_t srs, const uint64_t *evals, size_t n_evals, const uint64_t *point, size_t num_vars,
                     const uint64_t value[4], uint64_t *q_xy, uint8_t *q_inf, uint64_t final_eval[4]) {
    ZG_INIT();
    if (!final_eval || (num_vars && (!point || !q_xy)) || (n_evals && !evals) || (num_vars == 0 && !value)) return invalid("zg_hyperkzg_open: invalid argument");
    if (num_vars == 0) {  // :270-276
        for (int i = 0; i < 4; i++) final_eval[i] = value[i];
        return ZG_OK;
    }
    if (!srs) return invalid("zg_hyperkzg_open: invalid argument");
    DeviceGuard dg(bases_device(srs));
    Staging sg(lib_stream());
    const size_t cap = n_evals ? n_evals : 1;
    uint64_t *d_a = n_evals ? sg.in(evals, n_evals * 32) : sg.out<uint64_t>(32);
    uint64_t *d_b = sg.out<uint64_t>((cap / 2 + 1) * 32);
    return hk_open_device(sg, srs, d_a, d_b, n_evals, point, num_vars, q_xy, q_inf, final_eval, nullptr);
}

// ---- HyperKZG.batchOpen (src/poly/commitment/mod.zig:607-732)
// gpow[i] = gamma^i for i < k, gpow[k] = gamma;  gamma = fromU64(0x9a8b7c6d) * prod_j (point[j] + fromU64(11)), 0 -> 1 (:633-640)
__global__ void hk_gamma_kernel(const uint64_t *point, uint32_t v, uint32_t k, uint64_t *gpow) {
    Fr g = Fr::zero(), e11 = Fr::zero();
    g.l[0] = 0x9a8b7c6du;
    e11.l[0] = 11u;
    g = fe_to_mont(g);
    e11 = fe_to_mont(e11);
    for (uint32_t j = 0; j < v; j++) g = fe_mul(g, fe_add(fe_load<FrParams>(point + 4 * j), e11));
    if (fr_eq(g, Fr::zero())) g = Fr::one();
    Fr pw = Fr::one();
    for (uint32_t i = 0; i < k; i++) {
        fe_store(gpow + 4 * (size_t)i, pw);
        pw = fe_mul(pw, g);
    }
    fe_store(gpow + 4 * (size_t)k, g);
}

// out[j] (+)= g * p[j] for j < n_p; entries of out beyond n_p keep their value (zero on the first pass)  (:646-654)
__global__ void __launch_bounds__(256) hk_axpy_kernel(uint64_t *out, size_t n_out, const uint64_t *p, size_t n_p, const uint64_t *g, int first) {
    F29 gp = fr29_prescale(fe_load<FrParams>(g));
    size_t stride = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n_out; j += stride) {
        Fr acc = first ? Fr::zero() : fe_load<FrParams>(out + 4 * j);
        if (j < n_p) acc = fe_add(acc, fr_mul29(fe_load<FrParams>(p + 4 * j), gp));
        fe_store(out + 4 * j, acc);
    }
}

// evaluateMultilinear's monomial sum (:796-813): sum_idx a[idx] * eq[idx & mask] (eq indexed LSB-first via the reversed point)
__global__ void __launch_bounds__(256) hk_dot_mask_kernel(const uint64_t *a, size_t n, const uint64_t *eq, size_t mask, uint64_t *partials) {
    __shared__ u32 sh[SC_RED_WORDS];
    Fr g0 = Fr::zero(), g1 = Fr::zero();
    size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        g0 = fe_add(g0, fr_mul29v(fe_load<FrParams>(a + 4 * i), fe_load<FrParams>(eq + 4 * (i & mask))));
    block_sum_pair(g0, g1, sh);
    if (threadIdx.x == 0) {
        fe_store(partials + 8 * (size_t)blockIdx.x, g0);
        fe_store(partials + 8 * (size_t)blockIdx.x + 4, g1);
    }
}

// combined_eval = sum_i gamma^i * evaluations[i] (:657-662)
__global__ void hk_combined_eval_kernel(const uint64_t *evals, const uint64_t *gpow, uint32_t k, uint64_t *out) {
    Fr acc = Fr::zero();
    for (uint32_t i = 0; i < k; i++) acc = fe_add(acc, fe_mul(fe_load<FrParams>(gpow + 4 * (size_t)i), fe_load<FrParams>(evals + 4 * (size_t)i)));
    fe_store(out, acc);
}

int zg_hyperkzg_open_dev(zg_bases_t srs, const uint64_t *d_evals, size_t n_evals, const uint64_t *point, size_t num_vars,
                         const uint64_t value[4], void *stream, uint64_t *q_xy, uint8_t *q_inf, uint64_t final_eval[4]) {
    ZG_INIT();
    if (!srs || !final_eval || (num_vars && (!point || !q_xy)) || (n_evals && !d_evals) || (num_vars == 0 && !value))
        return invalid("zg_hyperkzg_open_dev: invalid argument");
    if (num_vars == 0) {  // :270-276
        for (int i = 0; i < 4; i++) final_eval[i] = value[i];
        return ZG_OK;
    }
    DeviceGuard dg(bases_device(srs));
    Staging sg(pick_stream(stream));
    const size_t cap = n_evals ? n_evals : 1;
    uint64_t *d_a = sg.out<uint64_t>(cap * 32), *d_b = sg.out<uint64_t>((cap / 2 + 1) * 32);
    // the loop folds its table in place: work on a copy, the caller's polynomial stays intact (open() takes evals by const slice)
    if (n_evals && sg.ok()) ZG_STAGE(sg, hipMemcpyAsync(d_a, d_evals, n_evals * 32, hipMemcpyDeviceToDevice, sg.st));
    return hk_open_device(sg, srs, d_a, d_b, n_evals, point, num_vars, q_xy, q_inf, final_eval, nullptr);
}

int zg_fr_scale(const uint64_t *a, size_t n, const uint64_t sc[4], uint64_t *out) {
    ZG_INIT();
    if (n && (!a || !sc || !out)) return invalid("zg_fr_scale: invalid argument");
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const uint64_t *d_a = sg.in(a, n * 32), *d_s = sg.in(sc, 32);
    uint64_t *d_o = sg.out<uint64_t>(n * 32);
    if (sg.ok()) {
        unsigned nb = div_up(n, 256);
        if (nb > 4096) nb = 4096;
        // out = 0 + a * s: the axpy kernel of HyperKZG.batchOpen's random linear combination with an empty accumulator
        hipLaunchKernelGGL(hk_axpy_kernel, dim3(nb), dim3(256), 0, sg.st, d_o, n, d_a, n, d_s, 1);
        sg.launched();
    }
    sg.fetch(out, d_o, n * 32);
    return sg.finish();
}

int zg_hyperkzg_batch_open(zg_bases_t srs, const uint64_t *const *polys, const size_t *lens, size_t k, const uint64_t *point,
                           size_t num_vars, uint64_t *q_xy, uint8_t *q_inf, size_t *n_quot, uint64_t *evaluations,
                           uint64_t final_eval[4], uint64_t gamma[4]) {
    ZG_INIT();
    if (!final_eval || !gamma || !n_quot || (k && (!polys || !lens || !evaluations)) || (num_vars && (!point || !q_xy)) || num_vars > 34)
        return invalid("zg_hyperkzg_batch_open: invalid argument");
    *n_quot = 0;
    if (k == 0) {  // :613-621
        for (int i = 0; i < 4; i++) {
            final_eval[i] = 0;
            gamma[i] = (uint64_t)FrParams::ONE[2 * i] | ((uint64_t)FrParams::ONE[2 * i + 1] << 32);
        }
        return ZG_OK;
    }
    for (size_t i = 0; i < k; i++)
        if (lens[i] && !polys[i]) return invalid("zg_hyperkzg_batch_open: null polynomial");
    if (!srs) return invalid("zg_hyperkzg_batch_open: invalid argument");
    DeviceGuard dg(bases_device(srs));
    size_t poly_size = lens[0], max_len = 1;
    for (size_t i = 0; i < k; i++) max_len = lens[i] > max_len ? lens[i] : max_len;
    const size_t cap = poly_size ? poly_size : 1;
    Staging sg(lib_stream());
    hipStream_t st = sg.st;
    const uint64_t *d_pt = num_vars ? sg.in(point, num_vars * 32) : sg.out<uint64_t>(32);
    uint64_t *d_g = sg.out<uint64_t>((k + 1) * 32), *d_p = sg.out<uint64_t>(max_len * 32), *d_a = sg.out<uint64_t>(cap * 32),
             *d_b = sg.out<uint64_t>((cap / 2 + 1) * 32), *d_ev = sg.out<uint64_t>((k + 1) * 32),
             *d_misc = sg.out<uint64_t>(SC_MISC_BYTES), *d_eq = sg.out<uint64_t>(((size_t)1 << (num_vars <= 10 ? num_vars : 0)) * 32);
    std::vector<uint64_t> h_ev(4 * k, 0), d2h(4 * (k + 1));
    std::vector<char> on_dev(k, 0);
    if (sg.ok()) {
        hipLaunchKernelGGL(hk_gamma_kernel, dim3(1), dim3(1), 0, st, d_pt, (uint32_t)num_vars, (uint32_t)k, d_g);
        // evaluateMultilinear (:788-817): the direct sum only for point.len <= 10 and len <= 1024, else evals[0]; empty -> 0
        bool any_small = false;
        for (size_t i = 0; i < k; i++) any_small = any_small || (lens[i] && num_vars && num_vars <= 10 && lens[i] <= 1024);
        if (any_small) {  // eq(point, .) with index bit j <-> point[j]: the big-endian table of the reversed point
            std::vector<uint64_t> rev(4 * num_vars);
            for (size_t j = 0; j < num_vars; j++)
                for (int l = 0; l < 4; l++) rev[4 * j + l] = point[4 * (num_vars - 1 - j) + l];
            sg.adopt(eq_table_enqueue(rev.data(), num_vars, nullptr, d_eq, st));
        }
    }
    for (size_t i = 0; i < k && sg.ok(); i++) {
        if (lens[i] && !ZG_STAGE(sg, hipMemcpyAsync(d_p, polys[i], lens[i] * 32, hipMemcpyHostToDevice, st))) break;
        unsigned nb = div_up(cap, 256);
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(hk_axpy_kernel, dim3(nb), dim3(256), 0, st, d_a, poly_size, d_p, lens[i] < poly_size ? lens[i] : poly_size,
                           d_g + 4 * i, i == 0 ? 1 : 0);
        if (lens[i] && num_vars && num_vars <= 10 && lens[i] <= 1024) {
            unsigned nd = sc_blocks(lens[i]);
            hipLaunchKernelGGL(hk_dot_mask_kernel, dim3(nd), dim3(256), 0, st, d_p, lens[i], d_eq, ((size_t)1 << num_vars) - 1, d_misc);
            hipLaunchKernelGGL(sc_finish_kernel<>, dim3(1), dim3(256), 0, st, d_misc, nd, 2u, d_misc + SC_SUMS_OFF, (uint64_t *)nullptr, (uint64_t)0);
            ZG_STAGE(sg, hipMemcpyAsync(d_ev + 4 * i, d_misc + SC_SUMS_OFF, 32, hipMemcpyDeviceToDevice, st));
            on_dev[i] = 1;
        } else if (lens[i]) {
            for (int l = 0; l < 4; l++) h_ev[4 * i + l] = polys[i][l];  // point.len == 0 or the large-polynomial fallback: evals[0]
        }
        sg.launched();  // d_p is reused by the next polynomial: its upload is ordered behind these kernels on the same stream
    }
    sg.fetch(d2h.data(), d_ev, 4 * 8 * k);
    sg.fetch(gamma, d_g + 4 * k, 32);
    if (sg.ok()) ZG_STAGE(sg, hipStreamSynchronize(st));  // the evaluations are the caller's before the quotients are computed
    if (!sg.ok()) return sg.finish();
    for (size_t i = 0; i < k; i++)
        for (int l = 0; l < 4; l++) evaluations[4 * i + l] = on_dev[i] ? d2h[4 * i + l] : h_ev[4 * i + l];
    if (num_vars == 0) {  // :665-673: no quotients, final_eval = combined_eval
        if (ZG_STAGE(sg, hipMemcpyAsync(d_ev, evaluations, 4 * 8 * k, hipMemcpyHostToDevice, st))) {
            hipLaunchKernelGGL(hk_combined_eval_kernel, dim3(1), dim3(1), 0, st, d_ev, d_g, (uint32_t)k, d_ev + 4 * k);
            sg.launched();
        }
        sg.fetch(final_eval, d_ev + 4 * k, 32);
        return sg.finish();
    }
    return hk_open_device(sg, srs, d_a, d_b, poly_size, point, num_vars, q_xy, q_inf, final_eval, n_quot);
}

}  // extern "C"
