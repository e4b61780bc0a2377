// dory.hip — a Dory opening proof as a device-resident session: DoryCommitmentScheme.openWithTranscript's reduce-and-fold loop
// (src/poly/commitment/dory.zig:1404-1669) with v1, v2, s1, s2 and the generators in HBM from begin to final. A round sends two messages
// to the host (218 and 148 words) and takes its two to four challenge scalars back; nothing else crosses, and no MSM handle is built
// after begin. The transcript stays the host's.
// The same session runs DoryCommitmentScheme.open (:1052-1378), the opening the prover calls, when it is begun over a resident key
// (zg_dory_open_key_begin): 2^sigma G1 against 2^nu G2 generators, read where dory_commit.hip's key holds them, on the two live lengths
// of dory_round_shape (dory_shape.h); a session begun with equal generator vectors is that schedule at nu = sigma. open's challenges are
// constants, so zg_dory_open_run enqueues every round of a session back to back and synchronises once.
//
// The arithmetic is the library's — pair_miller (pairing.hip.h), the XYZZ group law (xyzz.hip.h), the small bucket MSM
// (small_msm.hip.h), the G1 MSM over a handle (msm.hip) — and what is new here removes copies and launches around it:
//   DorySegPairs         the pair set (pair_set.hip.h) of a TABLE of up to 8 segments, each a slice of some G1 array against a slice of
//                        some G2 array (v1 halves x g2_vec, g1_vec x v2 halves, v1 halves x v2 halves): no gather; the Miller values
//                        are written segment-major, so the product and final-exponentiation launches follow as they are. A lane per
//                        pair, or a wavefront per pair for a session begun under the wave engine
//   dory_update_kernel   v1[i] += beta * g1_vec[i], i < cur, and v2[i] += beta_inv * g2_vec[i], i < row (:1578-1584; :1279-1286) in one
//                        launch, in place
//   dory_fold_kernel     v1 and s2 over n2 entries, v2 and s1 over h entries, folded by alpha / alpha_inv (:1615-1632; :1321-1340) in one
//                        launch, in place
//   dory_final_kernel    final_e1 = v1[0] + (gamma s1[0]) G, final_e2 = v2[0] + (gamma_inv s2[0]) H (:1641-1650)
// Everything is latency-bound at these lengths (2^sigma <= 2^13): 64-lane workgroups, a wave per SIMD, as in pairing.hip and points.hip.
// In place: xyzz_axpy_at reads index i of its operands and writes index i of the output in one lane; the folds write [0, n2) and read
// [n2, 2 n2) of what no lane writes.
#include <string.h>

#include <algorithm>
#include <unordered_set>

#include "common.hip.h"
#include "dory_shape.h"
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

// blocks [0, nb1): the G1 update over `cur` entries, blocks [nb1, nb1 + nb2): the G2 update over `row` entries (dory_shape.h; row = cur
// for equal generator vectors), nb1 = ceil(cur / 64), nb2 = ceil(row / 64); a wave is in one group
__global__ void __launch_bounds__(64) dory_update_kernel(const uint64_t *g1, const uint8_t *g1_inf, uint64_t *v1, uint8_t *v1_inf, const uint64_t *g2,
                                                         const uint8_t *g2_inf, uint64_t *v2, uint8_t *v2_inf, FeArg beta, FeArg beta_inv, uint32_t cur, uint32_t row) {
    const uint32_t nb = (cur + 63u) / 64u;
    const bool second = blockIdx.x >= nb;
    const size_t i = (size_t)(blockIdx.x - (second ? nb : 0u)) * 64u + threadIdx.x;
    if (i >= (second ? row : cur)) return;
    if (!second) xyzz_axpy_at<Fp>(g1, g1_inf, v1, v1_inf, fe_from_mont(fe_from_arg<FrParams>(beta)), i, v1, v1_inf);
    else xyzz_axpy_at<Fp2>(g2, g2_inf, v2, v2_inf, fe_from_mont(fe_from_arg<FrParams>(beta_inv)), i, v2, v2_inf);
}

// blocks [0, nb1): v1[i] = alpha v1[i] + v1[i + n2], i < n2; [nb1, nb1 + nb2): v2[i] = alpha_inv v2[i] + v2[i + n2], i < h; the rest, a
// lane per scalar: s1[i] = alpha s1[i] + s1[i + n2], i < h, then s2[i] = alpha_inv s2[i] + s2[i + n2], i < n2; nb1 = ceil(n2 / 64),
// nb2 = ceil(h / 64). The right half starts at n2 on both sides (dory_shape.h; h = n2 for equal generator vectors)
__global__ void __launch_bounds__(64) dory_fold_kernel(uint64_t *v1, uint8_t *v1_inf, uint64_t *v2, uint8_t *v2_inf, uint64_t *s1, uint64_t *s2, FeArg alpha,
                                                       FeArg alpha_inv, uint32_t n2, uint32_t h) {
    const uint32_t nb1 = (n2 + 63u) / 64u, nb2 = (h + 63u) / 64u;
    const uint32_t part = blockIdx.x < nb1 ? 0u : blockIdx.x < nb1 + nb2 ? 1u : 2u;
    const size_t i = (size_t)(blockIdx.x - (part == 0 ? 0u : part == 1 ? nb1 : nb1 + nb2)) * 64u + threadIdx.x;
    if (part == 0) {
        if (i < n2) xyzz_axpy_at<Fp>(v1, v1_inf, v1 + 8 * (size_t)n2, v1_inf + n2, fe_from_mont(fe_from_arg<FrParams>(alpha)), i, v1, v1_inf);
    } else if (part == 1) {
        if (i < h) xyzz_axpy_at<Fp2>(v2, v2_inf, v2 + 16 * (size_t)n2, v2_inf + n2, fe_from_mont(fe_from_arg<FrParams>(alpha_inv)), i, v2, v2_inf);
    } else if (i < (size_t)h + n2) {
        const bool second = i >= h;
        uint64_t *s = second ? s2 : s1;
        const size_t k = second ? i - h : i;
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
// length); the host packs them into the message layouts of zolt_gpu.h. A session holds 2 sigma + 1 such areas, one per message of the
// proof: the stepwise calls use area 0, zg_dory_open_run all of them
static constexpr int DORY_STAGE_REC = 192, DORY_STAGE_REC_WORDS = 32, DORY_STAGE_WORDS = DORY_STAGE_REC + 4 * DORY_STAGE_REC_WORDS;
static constexpr uint32_t DORY_MAX_SIGMA = 20;

enum DoryPhase { DORY_FIRST, DORY_SECOND, DORY_FOLD, DORY_FINAL, DORY_DONE };

struct zg_dory_s {
    int device = 0;
    uint32_t nu = 0, sigma = 0, round = 0;
    uint32_t sched_nu = 0;    // the nu of dory_round_shape: nu over a key (open's schedule), sigma for equal generator vectors
    size_t cap = 0, cur = 0;  // 2^sigma; the live length
    DoryPhase phase = DORY_DONE;
    int engine = ZG_PAIRING_ENGINE_LANE;  // read at begin, kept until close
    hipStream_t st = nullptr;
    zg_dory_key_s *key = nullptr;   // a session begun over a key reads g1 / g2 / msm where the key holds them, and counts in its `sessions`
    zg_bases_t g1_bases = nullptr;  // zg_dory_open_begin's own handle over g1_vec, built once
    zg_bases_t msm = nullptr;       // e1_beta's fixed prefix: g1_bases, or the key's handle
    uint64_t *g1 = nullptr, *g2 = nullptr, *v1 = nullptr, *v2 = nullptr, *s1 = nullptr, *s2 = nullptr;
    uint8_t *g1_inf = nullptr, *g2_inf = nullptr, *v1_inf = nullptr, *v2_inf = nullptr;
    uint64_t *miller = nullptr, *prod = nullptr, *stage = nullptr;  // 2 * cap Miller values, 4 products, the message staging areas
    size_t *seg_off = nullptr;
    zg::SmallMsmScratch sc1, sc2;  // the small MSMs' workspaces: three jobs of G1, two of G2
    uint64_t *h_stage = nullptr;   // pinned image of `stage`
    std::vector<void *> blocks;    // every pool block of the session
    std::mutex mu;
    size_t areas() const { return 2 * (size_t)sigma + 1; }
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
    if (s->key) {
        std::lock_guard<std::mutex> lk(s->key->mu);
        s->key->sessions--;
    }
    delete s;
}

static uint64_t *stage_rec(uint64_t *area, int r) { return area + DORY_STAGE_REC + DORY_STAGE_REC_WORDS * r; }

// the Miller values of n_seg segments, their n_seg products and final exponentiations -> area[48 j ..), on the session's stream
static int dory_pairings_enqueue(zg_dory_s *s, const DorySeg *seg, int n_seg, uint64_t *area) {
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
    pair_product_final_enqueue(s->miller, total, s->seg_off, (size_t)n_seg, s->st, s->prod, area, s->engine);
    return ZG_OK;
}

// the first n_areas staging areas come back: one copy and one host synchronisation
static int dory_fetch(zg_dory_s *s, size_t n_areas = 1) {
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipMemcpyAsync(s->h_stage, s->stage, n_areas * DORY_STAGE_WORDS * 8, hipMemcpyDeviceToHost, s->st));
    ZG_HIP(hipStreamSynchronize(s->st));
    return ZG_OK;
}
static void dory_take_rec(const uint64_t *h_area, int r, int words, uint64_t *out) {
    memcpy(out, h_area + DORY_STAGE_REC + DORY_STAGE_REC_WORDS * r, (size_t)words * 8);
    out[words - 1] &= 1;  // the flag word
}

// the four enqueue steps of a round and the final one, each into the staging area it is given (zeroed by the caller); the lengths
// are dory_round_shape's. Nothing here waits for the device.
static int dory_first_enqueue(zg_dory_s *s, const DoryRoundShape &sh, uint64_t *area) {
    hipStream_t st = s->st;
    const uint32_t n2 = sh.n2, h = sh.h;
    // d1_left, d1_right over the rows that are left, d2_left, d2_right over a half (:1245-1252; :1549-1552)
    const DorySeg segs[4] = {{s->v1, s->v1_inf, s->g2, s->g2_inf, h},
                             {s->v1 + 8 * (size_t)n2, s->v1_inf + n2, s->g2, s->g2_inf, h},
                             {s->g1, s->g1_inf, s->v2, s->v2_inf, n2},
                             {s->g1, s->g1_inf, s->v2 + 16 * (size_t)n2, s->v2_inf + n2, n2}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 4, area));
    // e1_beta = MSM(g1_vec[0..cur], s2) over the handle, e2_beta = msmG2(g2_vec[0..row], s1) (:1255-1261; :1553-1554)
    uint64_t *r0 = stage_rec(area, 0), *r1 = stage_rec(area, 1);
    ZG_TRY(zg_msm_g1_dev_async(s->msm, 0, sh.cur, s->s2, st, r0, reinterpret_cast<uint8_t *>(r0 + 8)));
    const SmallMsmJob job = {s->g2, s->g2_inf, s->s1, r1, sh.row};
    small_msm_enqueue<Fp2>(&job, 1, st, s->sc2);
    return ZG_OK;
}

static int dory_second_enqueue(zg_dory_s *s, const DoryRoundShape &sh, const uint64_t *beta, const uint64_t *beta_inv, uint64_t *area) {
    hipStream_t st = s->st;
    const uint32_t n2 = sh.n2, h = sh.h;
    hipLaunchKernelGGL(dory_update_kernel, dim3(div_up(sh.cur, 64) + div_up(sh.row, 64)), dim3(64), 0, st, s->g1, s->g1_inf, s->v1, s->v1_inf, s->g2, s->g2_inf,
                       s->v2, s->v2_inf, fe_arg(beta), fe_arg(beta_inv), sh.cur, sh.row);
    uint64_t *v1_hi = s->v1 + 8 * (size_t)n2, *v2_hi = s->v2 + 16 * (size_t)n2, *s1_hi = s->s1 + 4 * (size_t)n2, *s2_hi = s->s2 + 4 * (size_t)n2;
    uint8_t *v1i_hi = s->v1_inf + n2, *v2i_hi = s->v2_inf + n2;
    // c_plus = <v1[..h], v2[n2..n2+h]>, c_minus = <v1[n2..n2+h], v2[..h]>: the shorter slice (:1293-1294; :1587-1588)
    const DorySeg segs[2] = {{s->v1, s->v1_inf, v2_hi, v2i_hi, h}, {v1_hi, v1i_hi, s->v2, s->v2_inf, h}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 2, area));
    // e1_plus, e1_minus over a half (:1298-1299) and e2_plus, e2_minus over h (:1303-1304): two launch sets of two MSMs
    const SmallMsmJob j1[2] = {{s->v1, s->v1_inf, s2_hi, stage_rec(area, 0), n2}, {v1_hi, v1i_hi, s->s2, stage_rec(area, 1), n2}};
    small_msm_enqueue<Fp>(j1, 2, st, s->sc1);
    const SmallMsmJob j2[2] = {{v2_hi, v2i_hi, s->s1, stage_rec(area, 2), h}, {s->v2, s->v2_inf, s1_hi, stage_rec(area, 3), h}};
    small_msm_enqueue<Fp2>(j2, 2, st, s->sc2);
    return ZG_OK;
}

static void dory_fold_enqueue(zg_dory_s *s, const DoryRoundShape &sh, const uint64_t *alpha, const uint64_t *alpha_inv) {
    hipLaunchKernelGGL(dory_fold_kernel, dim3(div_up(sh.n2, 64) + div_up(sh.h, 64) + div_up((size_t)sh.h + sh.n2, 64)), dim3(64), 0, s->st, s->v1, s->v1_inf, s->v2,
                       s->v2_inf, s->s1, s->s2, fe_arg(alpha), fe_arg(alpha_inv), sh.n2, sh.h);
}

static void dory_final_enqueue(zg_dory_s *s, const uint64_t *gamma, const uint64_t *gamma_inv, uint64_t *area) {
    hipLaunchKernelGGL(dory_final_kernel, dim3(2), dim3(64), 0, s->st, s->v1, s->v1_inf, s->v2, s->v2_inf, s->s1, s->s2, fe_arg(gamma), fe_arg(gamma_inv),
                       stage_rec(area, 0), stage_rec(area, 1));
}

static void dory_take_first(const uint64_t *h_area, uint64_t *out218) {
    memcpy(out218, h_area, 192 * 8);
    dory_take_rec(h_area, 0, 9, out218 + 192);
    dory_take_rec(h_area, 1, 17, out218 + 201);
}
static void dory_take_second(const uint64_t *h_area, uint64_t *out148) {
    memcpy(out148, h_area, 96 * 8);
    dory_take_rec(h_area, 0, 9, out148 + 96);
    dory_take_rec(h_area, 1, 9, out148 + 105);
    dory_take_rec(h_area, 2, 17, out148 + 114);
    dory_take_rec(h_area, 3, 17, out148 + 131);
}
static void dory_take_final(const uint64_t *h_area, uint64_t *out26) {
    dory_take_rec(h_area, 0, 9, out26);
    dory_take_rec(h_area, 1, 17, out26 + 9);
}

// begin, after s->g1 / g2 (with their flags, on the device) and s->msm are in place — uploaded by zg_dory_open_begin, or the key's:
// the working vectors, the VMV message. g2_0_inf: g2_vec[0] is the identity
static int dory_begin(zg_dory_s *s, bool own_gens, const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, bool g2_0_inf,
                      const uint64_t *rows_xy, const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec, size_t n_v, const uint64_t *right_vec,
                      const uint64_t *left_vec, uint64_t *out_vmv) {
    const size_t N = s->cap, n_left = (size_t)1 << s->nu;
    uint64_t *d_v = nullptr;
    bool ok = true;
    if (own_gens)
        ok = pool_grab(s->blocks, s->g1, N * 64) && pool_grab(s->blocks, s->g1_inf, N) && pool_grab(s->blocks, s->g2, N * 128) && pool_grab(s->blocks, s->g2_inf, N);
    ok = ok && pool_grab(s->blocks, s->v1, N * 64) && pool_grab(s->blocks, s->v1_inf, N) && pool_grab(s->blocks, s->v2, N * 128) && pool_grab(s->blocks, s->v2_inf, N) &&
         pool_grab(s->blocks, s->s1, N * 32) && pool_grab(s->blocks, s->s2, N * 32) && pool_grab(s->blocks, d_v, N * 32) &&
         pool_grab(s->blocks, s->miller, 2 * N * Fp12::BYTES) && pool_grab(s->blocks, s->prod, 4 * Fp12::BYTES) &&
         pool_grab(s->blocks, s->stage, s->areas() * DORY_STAGE_WORDS * 8) && pool_grab(s->blocks, s->seg_off, (DORY_MAX_SEGS + 1) * sizeof(size_t)) &&
         pool_grab(s->blocks, s->sc1.dig, SmallMsmScratch::dig_bytes(N, 3)) && pool_grab(s->blocks, s->sc1.idx, SmallMsmScratch::idx_bytes(N, 3)) &&
         pool_grab(s->blocks, s->sc1.buckets, SmallMsmScratch::bucket_bytes(sizeof(XYZZ), 3)) && pool_grab(s->blocks, s->sc1.sums, SmallMsmScratch::sum_bytes(sizeof(XYZZ), 3)) &&
         pool_grab(s->blocks, s->sc2.dig, SmallMsmScratch::dig_bytes(N, 2)) && pool_grab(s->blocks, s->sc2.idx, SmallMsmScratch::idx_bytes(N, 2)) &&
         pool_grab(s->blocks, s->sc2.buckets, SmallMsmScratch::bucket_bytes(sizeof(G2XYZZ), 2)) && pool_grab(s->blocks, s->sc2.sums, SmallMsmScratch::sum_bytes(sizeof(G2XYZZ), 2));
    if (!ok) return ZG_ERR_NOMEM;
    s->h_stage = reinterpret_cast<uint64_t *>(pinned_get(s->areas() * DORY_STAGE_WORDS * 8));
    if (!s->h_stage) return ZG_ERR_NOMEM;
    hipStream_t st = s->st;
    const size_t rows = n_rows < N ? n_rows : N;
    if (own_gens) {  // the generators
        ZG_HIP(hipMemcpyAsync(s->g1, g1_xy, N * 64, hipMemcpyHostToDevice, st));
        ZG_HIP(hipMemcpyAsync(s->g2, g2_xy, N * 128, hipMemcpyHostToDevice, st));
        if (g1_inf) ZG_HIP(hipMemcpyAsync(s->g1_inf, g1_inf, N, hipMemcpyHostToDevice, st));
        else ZG_HIP(hipMemsetAsync(s->g1_inf, 0, N, st));
        if (g2_inf) ZG_HIP(hipMemcpyAsync(s->g2_inf, g2_inf, N, hipMemcpyHostToDevice, st));
        else ZG_HIP(hipMemsetAsync(s->g2_inf, 0, N, st));
    }
    // v1 = the row commitments, identities up to 2^sigma (:1438-1453); s1 = right_vec, s2 = left_vec, zeros up to 2^sigma
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
    if (n_v && !g2_0_inf) {
        Staging sg(st);
        g2_fixed_base_enqueue(sg, s->g2, d_v, n_v, s->v2, s->v2_inf);
        ZG_TRY(sg.finish());
    }
    if (own_gens) {
        // e1_beta's handle serves one MSM a round, over a prefix that halves: sigma MSMs, and sigma + 2 told to the planner as the issue
        // sizes it. The planner weighs a table of multiples against expected_uses; an opening at sigma = 20 must plan like one at 13, the
        // largest size the sections around this one are laid out for, so the figure stops at 13 + 2
        zg_msm_config cfg = {0, 0, (int)(s->sigma < 13 ? s->sigma + 2 : 15)};
        ZG_TRY(zg_g1_bases_upload_dev(s->g1, s->g1_inf, N, &cfg, st, &s->g1_bases));
        s->msm = s->g1_bases;
    }
    // the VMV message (:1456-1495): T = MSM(v1, v_vec), Gamma = MSM(g1_vec[0..len], v_vec), e1 = MSM(v1[0..2^nu], left_vec) as one launch
    // set; c = e(T, g2_vec[0]), d2 = e(Gamma, g2_vec[0]) as one more
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, st));
    uint64_t *r0 = stage_rec(s->stage, 0), *r1 = stage_rec(s->stage, 1), *r2 = stage_rec(s->stage, 2);
    const SmallMsmJob jobs[3] = {{s->v1, s->v1_inf, d_v, r0, (uint32_t)n_v}, {s->g1, s->g1_inf, d_v, r1, (uint32_t)n_v}, {s->v1, s->v1_inf, s->s2, r2, (uint32_t)n_left}};
    small_msm_enqueue<Fp>(jobs, 3, st, s->sc1);
    const DorySeg segs[2] = {{r0, reinterpret_cast<const uint8_t *>(r0 + 8), s->g2, s->g2_inf, 1}, {r1, reinterpret_cast<const uint8_t *>(r1 + 8), s->g2, s->g2_inf, 1}};
    ZG_TRY(dory_pairings_enqueue(s, segs, 2, s->stage));
    ZG_TRY(dory_fetch(s));
    memcpy(out_vmv, s->h_stage, 96 * 8);
    dory_take_rec(s->h_stage, 2, 9, out_vmv + 96);
    // v_vec's device copy has served (v2 and the VMV message; the stream is idle): it does not stay for the rounds
    s->blocks.erase(std::find(s->blocks.begin(), s->blocks.end(), (void *)d_v));
    pool_free(d_v);
    s->cur = N;
    s->round = 0;
    s->phase = s->sigma ? DORY_FIRST : DORY_FINAL;
    return ZG_OK;
}

// the session object of either begin, with its stream; registered once begin has gone through
static int dory_open(zg_dory_s *s, const char *who, int rc, zg_dory_t *out) {
    if (rc != ZG_OK) {
        if (!s->st) set_error(std::string(who) + ": no stream");
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
    s->sigma = s->sched_nu = sigma;
    s->cap = N;
    s->st = stream_acquire();
    const int rc = s->st ? dory_begin(s, true, g1_xy, g1_inf, g2_xy, g2_inf, g2_inf && g2_inf[0], rows_xy, rows_inf, n_rows, v_vec, n_v, right_vec, left_vec, out_vmv)
                         : ZG_ERR_HIP;
    return dory_open(s, who, rc, out);
}

int zg_dory_open_key_begin(zg_dory_key_t key, const uint64_t *rows_xy, const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec, size_t n_v,
                           const uint64_t *right_vec, const uint64_t *left_vec, uint32_t nu, uint32_t sigma, uint64_t *out_vmv, zg_dory_t *out) {
    const int engine = pairing_engine();
    ZG_INIT();
    const char *who = "zg_dory_open_key_begin";
    if (!out) return invalid(who, "no session pointer");
    *out = nullptr;
    if (!key) return invalid(who, "null key");
    if (nu > sigma || sigma > DORY_MAX_SIGMA) return invalid(who, "nu <= sigma <= 20 required");
    const size_t N = (size_t)1 << sigma;
    if (key->n_g1 < N) return invalid(who, "the key's g1_vec must hold 2^sigma entries");
    if (key->n_g2 < ((size_t)1 << nu)) return invalid(who, "the key's g2_vec must hold 2^nu entries");
    if (n_v > N) return invalid(who, "v_vec holds more than 2^sigma entries");
    if (!right_vec || !left_vec || !out_vmv || (n_rows && !rows_xy) || (n_v && !v_vec)) return invalid(who, "null data");
    DeviceGuard dg(key->device);
    zg_dory_s *s = new zg_dory_s();
    s->device = key->device;
    s->engine = engine;
    s->nu = s->sched_nu = nu;
    s->sigma = sigma;
    s->cap = N;
    {
        std::lock_guard<std::mutex> lk(key->mu);
        key->sessions++;
    }
    s->key = key;
    s->g1 = key->g1;
    s->g1_inf = key->g1_inf;
    s->g2 = key->g2;
    s->g2_inf = key->g2_inf;
    s->msm = key->bases;
    s->st = stream_acquire();
    const int rc = s->st ? dory_begin(s, false, nullptr, nullptr, nullptr, nullptr, key->g2_0_inf, rows_xy, rows_inf, n_rows, v_vec, n_v, right_vec, left_vec, out_vmv)
                         : ZG_ERR_HIP;
    return dory_open(s, who, rc, out);
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
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, s->st));
    ZG_TRY(dory_first_enqueue(s, dory_round_shape(s->sched_nu, s->sigma, s->round), s->stage));
    ZG_TRY(dory_fetch(s));
    dory_take_first(s->h_stage, out218);
    s->phase = DORY_SECOND;
    return ZG_OK;
}

int zg_dory_open_second_message(zg_dory_t s, const uint64_t beta[4], const uint64_t beta_inv[4], uint64_t *out148) {
    const char *who = "zg_dory_open_second_message";
    DORY_ENTER(who, DORY_SECOND);
    if (!beta || !beta_inv || !out148) return invalid(who, "null argument");
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, s->st));
    ZG_TRY(dory_second_enqueue(s, dory_round_shape(s->sched_nu, s->sigma, s->round), beta, beta_inv, s->stage));
    ZG_TRY(dory_fetch(s));
    dory_take_second(s->h_stage, out148);
    s->phase = DORY_FOLD;
    return ZG_OK;
}

int zg_dory_open_fold(zg_dory_t s, const uint64_t alpha[4], const uint64_t alpha_inv[4]) {
    const char *who = "zg_dory_open_fold";
    DORY_ENTER(who, DORY_FOLD);
    if (!alpha || !alpha_inv) return invalid(who, "null argument");
    const DoryRoundShape sh = dory_round_shape(s->sched_nu, s->sigma, s->round);
    dory_fold_enqueue(s, sh, alpha, alpha_inv);
    ZG_HIP(hipGetLastError());
    s->cur = sh.n2;
    s->round++;
    s->phase = s->round == s->sigma ? DORY_FINAL : DORY_FIRST;
    return ZG_OK;
}

int zg_dory_open_final(zg_dory_t s, const uint64_t gamma[4], const uint64_t gamma_inv[4], uint64_t *out26) {
    const char *who = "zg_dory_open_final";
    DORY_ENTER(who, DORY_FINAL);
    if (!gamma || !gamma_inv || !out26) return invalid(who, "null argument");
    ZG_HIP(hipMemsetAsync(s->stage, 0, DORY_STAGE_WORDS * 8, s->st));
    dory_final_enqueue(s, gamma, gamma_inv, s->stage);
    ZG_TRY(dory_fetch(s));
    dory_take_final(s->h_stage, out26);
    s->phase = DORY_DONE;
    return ZG_OK;
}

// every round's launches back to back on the session's stream, message m of the proof into staging area m (first and second messages
// of round t: 2 t, 2 t + 1; the final message: 2 sigma), then one copy and one synchronisation. The Miller values, the products, the
// segment offsets and the small MSMs' workspaces are reused from launch set to launch set in stream order, as the stepwise calls
// reuse them from call to call.
int zg_dory_open_run(zg_dory_t s, const uint64_t *challenges, uint64_t *out_first, uint64_t *out_second, uint64_t *out_final) {
    const char *who = "zg_dory_open_run";
    ZG_INIT();
    if (!s) return invalid(who, "null session");
    DeviceGuard dg(s->device);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->round != 0 || s->phase != (s->sigma ? DORY_FIRST : DORY_FINAL)) return invalid(who, "callable only right after begin");
    if (!challenges || !out_final || (s->sigma && (!out_first || !out_second))) return invalid(who, "null argument");
    const uint32_t sigma = s->sigma;
    ZG_HIP(hipMemsetAsync(s->stage, 0, s->areas() * DORY_STAGE_WORDS * 8, s->st));
    for (uint32_t t = 0; t < sigma; t++) {
        const DoryRoundShape sh = dory_round_shape(s->sched_nu, sigma, t);
        const uint64_t *c = challenges + 16 * (size_t)t;  // beta, beta_inv, alpha, alpha_inv
        ZG_TRY(dory_first_enqueue(s, sh, s->stage + (size_t)DORY_STAGE_WORDS * (2 * t)));
        ZG_TRY(dory_second_enqueue(s, sh, c, c + 4, s->stage + (size_t)DORY_STAGE_WORDS * (2 * t + 1)));
        dory_fold_enqueue(s, sh, c + 8, c + 12);
    }
    const uint64_t *g = challenges + 16 * (size_t)sigma;  // gamma, gamma_inv
    dory_final_enqueue(s, g, g + 4, s->stage + (size_t)DORY_STAGE_WORDS * (2 * sigma));
    s->cur = 1;
    s->round = sigma;
    s->phase = DORY_DONE;
    ZG_TRY(dory_fetch(s, s->areas()));
    for (uint32_t t = 0; t < sigma; t++) {
        dory_take_first(s->h_stage + (size_t)DORY_STAGE_WORDS * (2 * t), out_first + (size_t)ZG_DORY_FIRST_WORDS * t);
        dory_take_second(s->h_stage + (size_t)DORY_STAGE_WORDS * (2 * t + 1), out_second + (size_t)ZG_DORY_SECOND_WORDS * t);
    }
    dory_take_final(s->h_stage + (size_t)DORY_STAGE_WORDS * (2 * sigma), out_final);
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
