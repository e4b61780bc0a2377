// dory.hip — a Dory opening proof as a device-resident session: DoryCommitmentScheme.openWithTranscript's reduce-and-fold loop
// (src/poly/commitment/dory.zig:1404-1669) with v1, v2, s1, s2 and the generators in HBM from begin to final. A round sends two messages
// to the host (218 and 148 words) and takes its two to four challenge scalars back; nothing else crosses, and no MSM handle is built
// after begin. The transcript stays the host's.
//
// The arithmetic is the library's — pair_miller (pairing.hip.h), the XYZZ group law (xyzz.hip.h), the small bucket MSM
// (small_msm.hip.h), the G1 MSM over a handle (msm.hip) — and what is new here removes copies and launches around it:
//   DorySegPairs         the pair set (pair_set.hip.h) of a TABLE of up to 8 segments, each a slice of some G1 array against a slice of
//                        some G2 array (v1 halves x g2_vec, g1_vec x v2 halves, v1 halves x v2 halves): no gather; the Miller values
//                        are written segment-major, so the product and final-exponentiation launches follow as they are. A lane per
//                        pair, or a wavefront per pair for a session begun under the wave engine
//   dory_update_kernel   v1[i] += beta * g1_vec[i] and v2[i] += beta_inv * g2_vec[i] (:1578-1584) in one launch, in place
//   dory_fold_kernel     v1, v2, s1, s2 folded by alpha / alpha_inv (:1615-1632) in one launch, in place
//   dory_final_kernel    final_e1 = v1[0] + (gamma s1[0]) G, final_e2 = v2[0] + (gamma_inv s2[0]) H (:1641-1650)
// Everything is latency-bound at these lengths (2^sigma <= 2^13): 64-lane workgroups, a wave per SIMD, as in pairing.hip and points.hip.
// In place: xyzz_axpy_at reads index i of its operands and writes index i of the output in one lane; the folds write [0, n2) and read
// [n2, 2 n2) of what no lane writes.
#include <string.h>

#include <algorithm>
#include <unordered_set>

#include "common.hip.h"
#include "pair_set.hip.h"
#include "small_msm.hip.h"

namespace zg {

static constexpr int DORY_MAX_SEGS = 8;
struct DorySeg {
    const uint64_t *g1;   // count affine G1 points
    const uint8_t *g1_inf;
    const uint64_t *g2;   // count affine G2 points
    const uint8_t *g2_inf;
    uint32_t count;
};
struct DorySegs {
    DorySeg seg[DORY_MAX_SEGS];  // the unused entries have count 0
};

// Pair i of the launch set is entry i - start(k) of segment k, k the segment whose range [start(k), start(k) + count(k)) holds i; its
// Miller value goes to out[i]: segment-major. The table is read with constant indices only (selects, no private array). The one
// `writer` of the grid also writes the DORY_MAX_SEGS + 1 segment offsets that pair_product_kernel reads.
struct DoryPick {
    const uint64_t *g1, *g2;
    const uint8_t *g1_inf, *g2_inf;
    uint32_t j;
    bool live;
};
ZG_DEV DoryPick dory_seg_decode(const DorySegs &t, uint32_t i, bool writer, size_t *seg_off) {
    DoryPick pk = {nullptr, nullptr, nullptr, nullptr, 0, false};
    uint32_t start = 0;
#pragma unroll
    for (int k = 0; k < DORY_MAX_SEGS; k++) {
        if (writer) seg_off[k] = start;
        const bool in = i >= start && i - start < t.seg[k].count;
        pk.g1 = in ? t.seg[k].g1 : pk.g1;
        pk.g1_inf = in ? t.seg[k].g1_inf : pk.g1_inf;
        pk.g2 = in ? t.seg[k].g2 : pk.g2;
        pk.g2_inf = in ? t.seg[k].g2_inf : pk.g2_inf;
        pk.j = in ? i - start : pk.j;
        pk.live = pk.live || in;
        start += t.seg[k].count;
    }
    if (writer) seg_off[DORY_MAX_SEGS] = start;
    return pk;
}

// the session's pair set. The writer is lane 0 of workgroup 0: lane 0 of the grid under LANE, lane 0 of wave 0 under WAVE
struct DorySegPairs {
    DorySegs t;
    size_t *seg_off;
    ZG_DEV PairOperands operator()(uint32_t i) const {
        const DoryPick pk = dory_seg_decode(t, i, blockIdx.x == 0 && threadIdx.x == 0, seg_off);
        return {pk.g1 + 8 * (size_t)pk.j, pk.g2 + 16 * (size_t)pk.j, !pk.live || (pk.g1_inf && pk.g1_inf[pk.j]) || (pk.g2_inf && pk.g2_inf[pk.j])};
    }
};

// blocks [0, nb): the G1 update, blocks [nb, 2 nb): the G2 update, nb = ceil(cur / 64); a wave is in one group
__global__ void __launch_bounds__(64) dory_update_kernel(const uint64_t *g1, const uint8_t *g1_inf, uint64_t *v1, uint8_t *v1_inf, const uint64_t *g2,
                                                         const uint8_t *g2_inf, uint64_t *v2, uint8_t *v2_inf, FeArg beta, FeArg beta_inv, uint32_t cur) {
    const uint32_t nb = (cur + 63u) / 64u;
    const bool second = blockIdx.x >= nb;
    const size_t i = (size_t)(blockIdx.x - (second ? nb : 0u)) * 64u + threadIdx.x;
    if (i >= cur) return;
    if (!second) xyzz_axpy_at<Fp>(g1, g1_inf, v1, v1_inf, fe_from_mont(fe_from_arg<FrParams>(beta)), i, v1, v1_inf);
    else xyzz_axpy_at<Fp2>(g2, g2_inf, v2, v2_inf, fe_from_mont(fe_from_arg<FrParams>(beta_inv)), i, v2, v2_inf);
}

// blocks [0, nb): v1[i] = alpha v1[i] + v1[i + n2]; [nb, 2 nb): v2[i] = alpha_inv v2[i] + v2[i + n2]; the rest, a lane per scalar:
// s1[i] = alpha s1[i] + s1[i + n2] and s2[i] = alpha_inv s2[i] + s2[i + n2]; nb = ceil(n2 / 64)
__global__ void __launch_bounds__(64) dory_fold_kernel(uint64_t *v1, uint8_t *v1_inf, uint64_t *v2, uint8_t *v2_inf, uint64_t *s1, uint64_t *s2, FeArg alpha,
                                                       FeArg alpha_inv, uint32_t n2) {
    const uint32_t nb = (n2 + 63u) / 64u;
    const uint32_t part = blockIdx.x < nb ? 0u : blockIdx.x < 2u * nb ? 1u : 2u;
    const size_t i = (size_t)(blockIdx.x - part * nb) * 64u + threadIdx.x;
    if (part == 0) {
        if (i < n2) xyzz_axpy_at<Fp>(v1, v1_inf, v1 + 8 * (size_t)n2, v1_inf + n2, fe_from_mont(fe_from_arg<FrParams>(alpha)), i, v1, v1_inf);
    } else if (part == 1) {
        if (i < n2) xyzz_axpy_at<Fp2>(v2, v2_inf, v2 + 16 * (size_t)n2, v2_inf + n2, fe_from_mont(fe_from_arg<FrParams>(alpha_inv)), i, v2, v2_inf);
    } else if (i < 2 * (size_t)n2) {
        const bool second = i >= n2;
        uint64_t *s = second ? s2 : s1;
        const size_t k = second ? i - n2 : i;
        const Fr c = fe_from_arg<FrParams>(second ? alpha_inv : alpha);
        fe_store(s + 4 * k, fe_add(fe_mul(c, fe_load<FrParams>(s + 4 * k)), fe_load<FrParams>(s + 4 * (k + n2))));
    }
}

// G2Point.generator() (src/field/pairing.zig:770-818): x.c0, x.c1, y.c0, y.c1, Montgomery limbs
__device__ const u32 DORY_G2_GEN[4][8] = {
    {0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u},
    {0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u},
    {0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu},
    {0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u}};

template <class F>
static __device__ void dory_final_point(const AffineT<F> &gen, const uint64_t *v_xy, const uint8_t *v_inf, const Fr &s_mont, uint64_t *rec) {
    XyzzT<F> acc = xyzz_scalar_mul(gen, false, fe_from_mont(s_mont));
    if (!v_inf[0]) acc = xyzz_madd(acc, affine_load<F>(v_xy));
    AffineT<F> r;
    const bool isinf = xyzz_to_affine(acc, r);
    affine_store(rec, r);
    rec[2 * F::BYTES / 8] = isinf ? 1 : 0;
}

// block 0: final_e1 = v1[0].add(scalarMul(G1 generator, gamma * s1[0])); block 1: final_e2 = v2[0].add(H.scalarMul(gamma_inv * s2[0]))
__global__ void __launch_bounds__(64) dory_final_kernel(const uint64_t *v1, const uint8_t *v1_inf, const uint64_t *v2, const uint8_t *v2_inf, const uint64_t *s1,
                                                        const uint64_t *s2, FeArg gamma, FeArg gamma_inv, uint64_t *rec_e1, uint64_t *rec_e2) {
    if (threadIdx.x != 0) return;
    if (blockIdx.x == 0) {
        Affine g;  // AffinePoint.generator() = (1, 2) (src/msm/mod.zig:43-49)
        g.x = Fp::one();
        g.y = fe_dbl(g.x);
        dory_final_point<Fp>(g, v1, v1_inf, fe_mul(fe_from_arg<FrParams>(gamma), fe_load<FrParams>(s1)), rec_e1);
    } else {
        G2Affine h;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            h.x.c0.l[k] = DORY_G2_GEN[0][k]; h.x.c1.l[k] = DORY_G2_GEN[1][k];
            h.y.c0.l[k] = DORY_G2_GEN[2][k]; h.y.c1.l[k] = DORY_G2_GEN[3][k];
        }
        dory_final_point<Fp2>(h, v2, v2_inf, fe_mul(fe_from_arg<FrParams>(gamma_inv), fe_load<FrParams>(s2)), rec_e2);
    }
}

// the reference's identity carries x = y = 0 (AffinePoint.identity()): a row commitment flagged as one loses whatever the caller left in xy
__global__ void __launch_bounds__(64) dory_g1_clear_identities_kernel(uint64_t *xy, const uint8_t *inf, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !inf[i]) return;
    affine_store(xy + 8 * (size_t)i, Affine::identity());
}

// n G2 identities as the reference writes them, flags set (v2 past v_vec, :1516-1518)
__global__ void __launch_bounds__(64) dory_g2_identity_kernel(uint64_t *xy, uint8_t *inf, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    affine_store(xy + 16 * (size_t)i, G2Affine::identity());
    inf[i] = 1;
}

}  // namespace zg

// what a message is staged in on the device: four GT values, then four point records of 32 words each (16-byte aligned whatever their
// length); the host packs them into the message layouts of zolt_gpu.h
static constexpr int DORY_STAGE_REC = 192, DORY_STAGE_REC_WORDS = 32, DORY_STAGE_WORDS = DORY_STAGE_REC + 4 * DORY_STAGE_REC_WORDS;
static constexpr uint32_t DORY_MAX_SIGMA = 20;

enum DoryPhase { DORY_FIRST, DORY_SECOND, DORY_FOLD, DORY_FINAL, DORY_DONE };

struct zg_dory_s {
    int device = 0;
    uint32_t nu = 0, sigma = 0, round = 0;
    size_t cap = 0, cur = 0;  // 2^sigma; the live length
    DoryPhase phase = DORY_DONE;
    int engine = ZG_PAIRING_ENGINE_LANE;  // read at begin, kept until close
    hipStream_t st = nullptr;
    zg_bases_t g1_bases = nullptr;  // over g1_vec, built once: e1_beta's fixed prefix
    uint64_t *g1 = nullptr, *g2 = nullptr, *v1 = nullptr, *v2 = nullptr, *s1 = nullptr, *s2 = nullptr;
    uint8_t *g1_inf = nullptr, *g2_inf = nullptr, *v1_inf = nullptr, *v2_inf = nullptr;
    uint64_t *miller = nullptr, *prod = nullptr, *stage = nullptr;  // 2 * cap Miller values, 4 products, the message staging area
    size_t *seg_off = nullptr;
    zg::SmallMsmScratch sc1, sc2;  // the small MSMs' workspaces: three jobs of G1, two of G2
    uint64_t *h_stage = nullptr;   // pinned image of `stage`
    std::vector<void *> blocks;    // every pool block of the session
    std::mutex mu;
};

using namespace zg;

// the sessions that are open: what tells a handle from a stray word in the self-test read-back, which takes its handle as data
static std::mutex g_dory_mu;
static std::unordered_set<zg_dory_s *> g_dory_live;

// the stream has been synchronised (or never used) by the time the blocks go back to the pool
static void dory_free(zg_dory_s *s) {
    if (!s) return;
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->g1_bases) (void)zg_g1_bases_free(s->g1_bases);
    for (void *p : s->blocks) pool_free(p);
    if (s->h_stage) pinned_put(s->h_stage);
    if (s->st) stream_release(s->st, s->device);
    delete s;
}

static uint64_t *stage_rec(const zg_dory_s *s, int r) { return s->stage + DORY_STAGE_REC + DORY_STAGE_REC_WORDS * r; }

// the Miller values of n_seg segments, their n_seg products and final exponentiations -> stage[48 j ..), on the session's stream
static int dory_pairings_enqueue(zg_dory_s *s, const DorySeg *seg, int n_seg) {
    DorySegs t = {};
    size_t total = 0;
    for (int k = 0; k < n_seg; k++) {
        t.seg[k] = seg[k];
        total += seg[k].count;
    }
    // an empty launch set has no Miller launch and so no writer, and pair_product_kernel still reads the offsets: all are zero then,
    // and the host writes them
    if (!total) ZG_HIP(hipMemsetAsync(s->seg_off, 0, (DORY_MAX_SEGS + 1) * sizeof(size_t), s->st));
    pair_set_miller_enqueue(DorySegPairs{t, s->seg_off}, total, s->st, s->miller, s->engine);
    pair_product_final_enqueue(s->miller, total, s->seg_off, (size_t)n_seg, s->st, s->prod, s->stage, s->engine);
    return ZG_OK;
}

// the staging area comes back: one copy and the message's host synchronisation
static int dory_fetch(zg_dory_s *s) {
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipMemcpyAsync(s->h_stage, s->stage, DORY_STAGE_WORDS * 8, hipMemcpyDeviceToHost, s->st));
    ZG_HIP(hipStreamSynchronize(s->st));
    return ZG_OK;
}
static void dory_take_rec(const zg_dory_s *s, int r, int words, uint64_t *out) {
    memcpy(out, s->h_stage + DORY_STAGE_REC + DORY_STAGE_REC_WORDS * r, (size_t)words * 8);
    out[words - 1] &= 1;  // the flag word
}

static int dory_begin(zg_dory_s *s, const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, const uint64_t *rows_xy,
                      const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec, size_t n_v, const uint64_t *right_vec, const uint64_t *left_vec,
                      uint64_t *out_vmv) {
    const size_t N = s->cap, n_left = (size_t)1 << s->nu;
    uint64_t *d_v = nullptr;
    bool ok = pool_grab(s->blocks, s->g1, N * 64) && pool_grab(s->blocks, s->g1_inf, N) && pool_grab(s->blocks, s->g2, N * 128) && pool_grab(s->blocks, s->g2_inf, N) &&
              pool_grab(s->blocks, s->v1, N * 64) && pool_grab(s->blocks, s->v1_inf, N) && pool_grab(s->blocks, s->v2, N * 128) && pool_grab(s->blocks, s->v2_inf, N) &&
              pool_grab(s->blocks, s->s1, N * 32) && pool_grab(s->blocks, s->s2, N * 32) && pool_grab(s->blocks, d_v, N * 32) &&
              pool_grab(s->blocks, s->miller, 2 * N * Fp12::BYTES) && pool_grab(s->blocks, s->prod, 4 * Fp12::BYTES) && pool_grab(s->blocks, s->stage, DORY_STAGE_WORDS * 8) &&
              pool_grab(s->blocks, s->seg_off, (DORY_MAX_SEGS + 1) * sizeof(size_t)) &&
              pool_grab(s->blocks, s->sc1.dig, SmallMsmScratch::dig_bytes(N, 3)) && pool_grab(s->blocks, s->sc1.idx, SmallMsmScratch::idx_bytes(N, 3)) &&
              pool_grab(s->blocks, s->sc1.buckets, SmallMsmScratch::bucket_bytes(sizeof(XYZZ), 3)) && pool_grab(s->blocks, s->sc1.sums, SmallMsmScratch::sum_bytes(sizeof(XYZZ), 3)) &&
              pool_grab(s->blocks, s->sc2.dig, SmallMsmScratch::dig_bytes(N, 2)) && pool_grab(s->blocks, s->sc2.idx, SmallMsmScratch::idx_bytes(N, 2)) &&
              pool_grab(s->blocks, s->sc2.buckets, SmallMsmScratch::bucket_bytes(sizeof(G2XYZZ), 2)) && pool_grab(s->blocks, s->sc2.sums, SmallMsmScratch::sum_bytes(sizeof(G2XYZZ), 2));
    if (!ok) return ZG_ERR_NOMEM;
    s->h_stage = reinterpret_cast<uint64_t *>(pinned_get(DORY_STAGE_WORDS * 8));
    if (!s->h_stage) return ZG_ERR_NOMEM;
    hipStream_t st = s->st;
    const size_t rows = n_rows < N ? n_rows : N;
    // the generators; v1 = the row commitments, identities up to 2^sigma (:1438-1453); s1 = right_vec, s2 = left_vec, zeros up to 2^sigma
    ZG_HIP(hipMemcpyAsync(s->g1, g1_xy, N * 64, hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemcpyAsync(s->g2, g2_xy, N * 128, hipMemcpyHostToDevice, st));
    if (g1_inf) ZG_HIP(hipMemcpyAsync(s->g1_inf, g1_inf, N, hipMemcpyHostToDevice, st));
    else ZG_HIP(hipMemsetAsync(s->g1_inf, 0, N, st));
    if (g2_inf) ZG_HIP(hipMemcpyAsync(s->g2_inf, g2_inf, N, hipMemcpyHostToDevice, st));
    else ZG_HIP(hipMemsetAsync(s->g2_inf, 0, N, st));
    ZG_HIP(hipMemsetAsync(s->v1, 0, N * 64, st));
    ZG_HIP(hipMemsetAsync(s->v1_inf, 1, N, st));
    if (rows) {
        ZG_HIP(hipMemcpyAsync(s->v1, rows_xy, rows * 64, hipMemcpyHostToDevice, st));
        if (rows_inf) {
            ZG_HIP(hipMemcpyAsync(s->v1_inf, rows_inf, rows, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(dory_g1_clear_identities_kernel, dim3(div_up(rows, 64)), dim3(64), 0, st, s->v1, s->v1_inf, (uint32_t)rows);
        } else {
            ZG_HIP(hipMemsetAsync(s->v1_inf, 0, rows, st));
        }
    }
    ZG_HIP(hipMemcpyAsync(s->s1, right_vec, N * 32, hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemsetAsync(s->s2, 0, N * 32, st));
    ZG_HIP(hipMemcpyAsync(s->s2, left_vec, n_left * 32, hipMemcpyHostToDevice, st));
    if (n_v) ZG_HIP(hipMemcpyAsync(d_v, v_vec, n_v * 32, hipMemcpyHostToDevice, st));
    // v2[i] = g2_vec[0].scalarMul(v_vec[i]), identities past v_vec (:1511-1519)
    hipLaunchKernelGGL(dory_g2_identity_kernel, dim3(div_up(N, 64)), dim3(64), 0, st, s->v2, s->v2_inf, (uint32_t)N);
    if (n_v && !(g2_inf && g2_inf[0])) {
        Staging sg(st);
        g2_fixed_base_enqueue(sg, s->g2, d_v, n_v, s->v2, s->v2_inf);
        ZG_TRY(sg.finish());
    }
    // e1_beta's handle serves one MSM a round, over a prefix that halves: sigma MSMs, and sigma + 2 told to the planner as the issue
    // sizes it. The planner weighs a table of multiples against expected_uses; an opening at sigma = 20 must plan like one at 13, the
    // largest size the sections around this one are laid out for, so the figure stops at 13 + 2
    zg_msm_config cfg = {0, 0, (int)(s->sigma < 13 ? s->sigma + 2 : 15)};
    ZG_TRY(zg_g1_bases_upload_dev(s->g1, s->g1_inf, N, &cfg, st, &s->g1_bases));
    // the VMV message (:1456-1495): T = MSM(v1, v_vec), Gamma = MSM(g1_vec[0..len], v_vec), e1 = MSM(v1[0..2^nu], left_vec) as one launch
    // set; c = e(T, g2_vec[0]), d2 = e(Gamma, g2_vec[0]) as one more
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, st));
    uint64_t *r0 = stage_rec(s, 0), *r1 = stage_rec(s, 1), *r2 = stage_rec(s, 2);
    const SmallMsmJob jobs[3] = {{s->v1, s->v1_inf, d_v, r0, (uint32_t)n_v}, {s->g1, s->g1_inf, d_v, r1, (uint32_t)n_v}, {s->v1, s->v1_inf, s->s2, r2, (uint32_t)n_left}};
    small_msm_enqueue<Fp>(jobs, 3, st, s->sc1);
    const DorySeg segs[2] = {{r0, reinterpret_cast<const uint8_t *>(r0 + 8), s->g2, s->g2_inf, 1}, {r1, reinterpret_cast<const uint8_t *>(r1 + 8), s->g2, s->g2_inf, 1}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 2));
    ZG_TRY(dory_fetch(s));
    memcpy(out_vmv, s->h_stage, 96 * 8);
    dory_take_rec(s, 2, 9, out_vmv + 96);
    // v_vec's device copy has served (v2 and the VMV message; the stream is idle): it does not stay for the rounds
    s->blocks.erase(std::find(s->blocks.begin(), s->blocks.end(), (void *)d_v));
    pool_free(d_v);
    s->cur = N;
    s->round = 0;
    s->phase = s->sigma ? DORY_FIRST : DORY_FINAL;
    return ZG_OK;
}

extern "C" {

int zg_dory_open_begin(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n_gens, const uint64_t *rows_xy,
                       const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec, size_t n_v, const uint64_t *right_vec, const uint64_t *left_vec, uint32_t nu,
                       uint32_t sigma, uint64_t *out_vmv, zg_dory_t *out) {
    const int engine = pairing_engine();
    ZG_INIT();
    const char *who = "zg_dory_open_begin";
    if (!out) return invalid(who, "no session pointer");
    *out = nullptr;
    if (nu > sigma || sigma > DORY_MAX_SIGMA) return invalid(who, "nu <= sigma <= 20 required");
    const size_t N = (size_t)1 << sigma;
    if (n_gens < N) return invalid(who, "g1_vec and g2_vec must hold 2^sigma entries");
    if (n_v > N) return invalid(who, "v_vec holds more than 2^sigma entries");
    if (!g1_xy || !g2_xy || !right_vec || !left_vec || !out_vmv || (n_rows && !rows_xy) || (n_v && !v_vec)) return invalid(who, "null data");
    zg_dory_s *s = new zg_dory_s();
    s->device = current_device();
    s->engine = engine;
    s->nu = nu;
    s->sigma = sigma;
    s->cap = N;
    s->st = stream_acquire();
    int rc = s->st ? dory_begin(s, g1_xy, g1_inf, g2_xy, g2_inf, rows_xy, rows_inf, n_rows, v_vec, n_v, right_vec, left_vec, out_vmv) : ZG_ERR_HIP;
    if (rc != ZG_OK) {
        if (!s->st) set_error("zg_dory_open_begin: no stream");
        dory_free(s);
        return rc;
    }
    {
        std::lock_guard<std::mutex> lk(g_dory_mu);
        g_dory_live.insert(s);
    }
    *out = s;
    return ZG_OK;
}

#define DORY_ENTER(who, want)                                                                   \
    ZG_INIT();                                                                                  \
    if (!s) return invalid(who, "null session");                                                \
    DeviceGuard _dg(s->device);                                                                 \
    std::lock_guard<std::mutex> _lk(s->mu);                                                     \
    if (s->phase != (want)) return invalid(who, "called out of order")

int zg_dory_open_first_message(zg_dory_t s, uint64_t *out218) {
    const char *who = "zg_dory_open_first_message";
    DORY_ENTER(who, DORY_FIRST);
    if (!out218) return invalid(who, "null output");
    const uint32_t cur = (uint32_t)s->cur, n2 = cur / 2;
    hipStream_t st = s->st;
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, st));
    // d1_left, d1_right, d2_left, d2_right (:1549-1552)
    const DorySeg segs[4] = {{s->v1, s->v1_inf, s->g2, s->g2_inf, n2},
                             {s->v1 + 8 * (size_t)n2, s->v1_inf + n2, s->g2, s->g2_inf, n2},
                             {s->g1, s->g1_inf, s->v2, s->v2_inf, n2},
                             {s->g1, s->g1_inf, s->v2 + 16 * (size_t)n2, s->v2_inf + n2, n2}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 4));
    // e1_beta = MSM(g1_vec[0..cur], s2) over the handle, e2_beta = msmG2(g2_vec[0..cur], s1) (:1553-1554)
    uint64_t *r0 = stage_rec(s, 0), *r1 = stage_rec(s, 1);
    ZG_TRY(zg_msm_g1_dev_async(s->g1_bases, 0, cur, s->s2, st, r0, reinterpret_cast<uint8_t *>(r0 + 8)));
    const SmallMsmJob job = {s->g2, s->g2_inf, s->s1, r1, cur};
    small_msm_enqueue<Fp2>(&job, 1, st, s->sc2);
    ZG_TRY(dory_fetch(s));
    memcpy(out218, s->h_stage, 192 * 8);
    dory_take_rec(s, 0, 9, out218 + 192);
    dory_take_rec(s, 1, 17, out218 + 201);
    s->phase = DORY_SECOND;
    return ZG_OK;
}

int zg_dory_open_second_message(zg_dory_t s, const uint64_t beta[4], const uint64_t beta_inv[4], uint64_t *out148) {
    const char *who = "zg_dory_open_second_message";
    DORY_ENTER(who, DORY_SECOND);
    if (!beta || !beta_inv || !out148) return invalid(who, "null argument");
    const uint32_t cur = (uint32_t)s->cur, n2 = cur / 2;
    hipStream_t st = s->st;
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, st));
    hipLaunchKernelGGL(dory_update_kernel, dim3(2 * div_up(cur, 64)), dim3(64), 0, st, s->g1, s->g1_inf, s->v1, s->v1_inf, s->g2, s->g2_inf, s->v2, s->v2_inf,
                       fe_arg(beta), fe_arg(beta_inv), cur);
    uint64_t *v1_hi = s->v1 + 8 * (size_t)n2, *v2_hi = s->v2 + 16 * (size_t)n2, *s1_hi = s->s1 + 4 * (size_t)n2, *s2_hi = s->s2 + 4 * (size_t)n2;
    uint8_t *v1i_hi = s->v1_inf + n2, *v2i_hi = s->v2_inf + n2;
    // c_plus = <v1[..n2], v2[n2..]>, c_minus = <v1[n2..], v2[..n2]> (:1587-1588)
    const DorySeg segs[2] = {{s->v1, s->v1_inf, v2_hi, v2i_hi, n2}, {v1_hi, v1i_hi, s->v2, s->v2_inf, n2}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 2));
    // e1_plus, e1_minus (:1589-1590) and e2_plus, e2_minus (:1591-1592): two launch sets of two MSMs
    const SmallMsmJob j1[2] = {{s->v1, s->v1_inf, s2_hi, stage_rec(s, 0), n2}, {v1_hi, v1i_hi, s->s2, stage_rec(s, 1), n2}};
    small_msm_enqueue<Fp>(j1, 2, st, s->sc1);
    const SmallMsmJob j2[2] = {{v2_hi, v2i_hi, s->s1, stage_rec(s, 2), n2}, {s->v2, s->v2_inf, s1_hi, stage_rec(s, 3), n2}};
    small_msm_enqueue<Fp2>(j2, 2, st, s->sc2);
    ZG_TRY(dory_fetch(s));
    memcpy(out148, s->h_stage, 96 * 8);
    dory_take_rec(s, 0, 9, out148 + 96);
    dory_take_rec(s, 1, 9, out148 + 105);
    dory_take_rec(s, 2, 17, out148 + 114);
    dory_take_rec(s, 3, 17, out148 + 131);
    s->phase = DORY_FOLD;
    return ZG_OK;
}

int zg_dory_open_fold(zg_dory_t s, const uint64_t alpha[4], const uint64_t alpha_inv[4]) {
    const char *who = "zg_dory_open_fold";
    DORY_ENTER(who, DORY_FOLD);
    if (!alpha || !alpha_inv) return invalid(who, "null argument");
    const uint32_t n2 = (uint32_t)(s->cur / 2);
    hipLaunchKernelGGL(dory_fold_kernel, dim3(2 * div_up(n2, 64) + div_up(2 * (size_t)n2, 64)), dim3(64), 0, s->st, s->v1, s->v1_inf, s->v2, s->v2_inf, s->s1,
                       s->s2, fe_arg(alpha), fe_arg(alpha_inv), n2);
    ZG_HIP(hipGetLastError());
    s->cur = n2;
    s->round++;
    s->phase = s->round == s->sigma ? DORY_FINAL : DORY_FIRST;
    return ZG_OK;
}

int zg_dory_open_final(zg_dory_t s, const uint64_t gamma[4], const uint64_t gamma_inv[4], uint64_t *out26) {
    const char *who = "zg_dory_open_final";
    DORY_ENTER(who, DORY_FINAL);
    if (!gamma || !gamma_inv || !out26) return invalid(who, "null argument");
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, s->st));
    hipLaunchKernelGGL(dory_final_kernel, dim3(2), dim3(64), 0, s->st, s->v1, s->v1_inf, s->v2, s->v2_inf, s->s1, s->s2, fe_arg(gamma), fe_arg(gamma_inv),
                       stage_rec(s, 0), stage_rec(s, 1));
    ZG_TRY(dory_fetch(s));
    dory_take_rec(s, 0, 9, out26);
    dory_take_rec(s, 1, 17, out26 + 9);
    s->phase = DORY_DONE;
    return ZG_OK;
}

size_t zg_dory_open_len(zg_dory_t s) { return s ? s->cur : 0; }

int zg_dory_open_close(zg_dory_t s) {
    if (!s) return ZG_OK;
    ZG_INIT();
    DeviceGuard dg(s->device);
    {
        std::lock_guard<std::mutex> lk(g_dory_mu);
        g_dory_live.erase(s);
    }
    dory_free(s);
    return ZG_OK;
}

}  // extern "C"

// runtime.hip's zg_field_op forwards the ZG_OP_DORY_* codes here (zolt_gpu_internal.h): waits for the session's enqueued work, then
// copies the first min(live length, n) entries of one of its four vectors to the host as records. The handle arrives as a data word of
// an entry point that otherwise takes field elements, so it is looked up among the open sessions before anything is read through it, and
// the registry stays locked for the read: no close runs under it.
int zg::dory_state_read(int field, int op, const uint64_t *handle_word, const uint64_t *b, uint64_t *out, size_t n) {
    const char *what = "Dory state hooks: Fr, a = one word holding the handle of an open session, b = NULL, out = n records";
    zg_dory_s *s = handle_word ? reinterpret_cast<zg_dory_s *>((uintptr_t)handle_word[0]) : nullptr;
    if (field != ZG_FIELD_FR || b || !s || (n && !out)) return invalid("zg_field_op", what);
    std::lock_guard<std::mutex> reg(g_dory_mu);
    if (!g_dory_live.count(s)) return invalid("zg_field_op", what);
    DeviceGuard dg(s->device);
    std::lock_guard<std::mutex> lk(s->mu);
    if (n > s->cur) n = s->cur;
    const bool g1 = op == ZG_OP_DORY_V1, g2 = op == ZG_OP_DORY_V2;
    if (n && (g1 || g2)) {  // point records: the coordinates, then a flag word
        const size_t w = g1 ? 8 : 16;
        std::vector<uint64_t> xy(n * w);
        std::vector<uint8_t> inf(n);
        ZG_HIP(hipMemcpyAsync(xy.data(), g1 ? s->v1 : s->v2, n * w * 8, hipMemcpyDeviceToHost, s->st));
        ZG_HIP(hipMemcpyAsync(inf.data(), g1 ? s->v1_inf : s->v2_inf, n, hipMemcpyDeviceToHost, s->st));
        ZG_HIP(hipStreamSynchronize(s->st));
        for (size_t i = 0; i < n; i++) {
            memcpy(out + (w + 1) * i, &xy[w * i], w * 8);
            out[(w + 1) * i + w] = inf[i] ? 1 : 0;
        }
        return ZG_OK;
    }
    if (n) ZG_HIP(hipMemcpyAsync(out, op == ZG_OP_DORY_S1 ? s->s1 : s->s2, n * 32, hipMemcpyDeviceToHost, s->st));
    ZG_HIP(hipStreamSynchronize(s->st));
    return ZG_OK;
}
