// dory_vsetup.hip — DoryVerifierSetup.fromSRS (src/zkvm/preprocessing.zig:889-973) for every level of a key in ONE launch set. The
// reference walks k = 1..K and runs three multiPair calls per level (:929, :932, :935), each pairing with its own final exponentiation
// (:833-850): 3 * 2^K - 2 pairings one after another. All pairs are known before the first of them runs, so here they are
//   DvPairs                     the pair set (pair_set.hip.h), a lane or a wavefront per pair: (family, level, offset) from the pair index
//                               (dory_vsetup.hip.h), the two generators read where the key holds them, the Miller value written segment-major
//   pair_product_kernel         pairing.hip's, unchanged, over the 3K + 1 segments of dv_seg: K + 1 diagonal, K upper, K lower
//   dory_vsetup_chi_kernel      one lane: the running product of the K + 1 diagonal products, chi_unreduced[k] = P_0 ... P_k — K serial
//                               Fp12 products, the only serial step fromSRS has (:935)
//   pair_final_exp_kernel       pairing.hip's, unchanged, once over the 3K + 1 values
// The final exponentiation is a homomorphism and values are canonical, so exponentiating the products gives the bits the reference gets
// from multiplying exponentiated pairings (the argument of pairing.hip). delta_1r[0] = delta_2r[0] = one (:906-907) are written by the
// host: no lane computes them.
// Shape of the lane engine's Miller launch: 64-lane workgroups. A lane keeps its tower values in 3.4 KB of private segment
// and the kernel allows one wave per SIMD; 3 * 2^10 - 2 lanes are 48 waves on 256 compute units, so every wave has a SIMD, an L1 and
// its scratch lines to itself and the launch lasts one lane's serial depth whatever K is (up to 2^14 generators, where the device fills).
#include <string.h>

#include <vector>

#include "common.hip.h"
#include "pair_set.hip.h"
#include "dory_vsetup.hip.h"

namespace zg {

// pair i = dv_decode(K, i) over the generators; g1_inf / g2_inf may be null (the points form without flags), the key's are not. An
// identity gives one: multiPair's `continue` (:839), pairingFp's rule for chi[0]
struct DvPairs {
    const uint64_t *g1_xy;
    const uint8_t *g1_inf;
    const uint64_t *g2_xy;
    const uint8_t *g2_inf;
    uint32_t K;
    ZG_DEV PairOperands operator()(uint32_t i) const {
        const DvPair pr = dv_decode(K, i);
        return {g1_xy + 8 * (size_t)pr.i1, g2_xy + 16 * (size_t)pr.i2, (g1_inf && g1_inf[pr.i1]) || (g2_inf && g2_inf[pr.i2])};
    }
};

// prod[k] = prod[0] * ... * prod[k] for k <= K, in place: chi[k] = chi[k-1] * (level k's product) before the final exponentiation
__global__ void __launch_bounds__(64) dory_vsetup_chi_kernel(uint64_t *prod, uint32_t K) {
    if (blockIdx.x || threadIdx.x) return;
    Fp12 acc = fp12_load(prod);
#pragma unroll 1
    for (uint32_t k = 1; k <= K; k++) {
        const Fp12 v = fp12_load(prod + 48 * (size_t)k);
        fp12_mul(acc, acc, v);
        fp12_store(prod + 48 * (size_t)k, acc);
    }
}

static constexpr size_t DV_MAX_G1 = (size_t)1 << 16;  // zg_dory_key_create's bound

// GT one: Fp's Montgomery one, then eleven zeros
static void dv_gt_one(uint64_t *out) {
    static const uint64_t ONE[4] = {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full};
    memset(out, 0, Fp12::BYTES);
    memcpy(out, ONE, sizeof ONE);
}

static int dv_validate(const char *who, size_t n_g1, size_t n_g2, const void *out_gt, size_t levels_cap, uint32_t &K) {
    if (n_g1 < 1 || n_g1 > DV_MAX_G1) return invalid(who, "1 <= n_g1 <= 2^16 required");
    K = dv_log2((uint32_t)n_g1);
    if (n_g2 < ((size_t)1 << K)) return invalid(who, "g2_vec is shorter than 2^floor(log2 n_g1)");
    if (levels_cap < (size_t)K + 1) return invalid(who, "levels_cap is less than floor(log2 n_g1) + 1");
    if (!out_gt) return invalid(who, "no output");
    return ZG_OK;
}

// the launch set over DEVICE generators on sg.st, the fetches into the three arrays of out_gt, the wait
static int dv_run(Staging &sg, const uint64_t *d_g1, const uint8_t *d_g1i, const uint64_t *d_g2, const uint8_t *d_g2i, uint32_t K, uint64_t *out_gt) {
    const size_t lanes = dv_lanes(K), segs = dv_segments(K), levels = (size_t)K + 1;
    const int engine = pairing_engine();
    std::vector<size_t> seg(segs + 1);  // outlives the wait below
    for (size_t s = 0; s <= segs; s++) seg[s] = dv_seg(K, (uint32_t)s);
    const size_t *d_seg = sg.in(seg.data(), (segs + 1) * sizeof(size_t));
    uint64_t *d_miller = sg.out<uint64_t>(lanes * Fp12::BYTES), *d_prod = sg.out<uint64_t>(segs * Fp12::BYTES), *d_fe = sg.out<uint64_t>(segs * Fp12::BYTES);
    if (sg.ok()) {
        pair_set_miller_enqueue(DvPairs{d_g1, d_g1i, d_g2, d_g2i, K}, lanes, sg.st, d_miller, engine);
        pair_product_enqueue(d_miller, lanes, d_seg, segs, sg.st, d_prod);
        if (K) hipLaunchKernelGGL(dory_vsetup_chi_kernel, dim3(1), dim3(64), 0, sg.st, d_prod, K);
        pair_final_exp_enqueue(d_prod, segs, sg.st, d_fe, engine);
        sg.launched();
    }
    // chi[0..K] | delta_1r[1..K] | delta_2r[1..K] on the device; the two k = 0 slots of the deltas are the host's
    sg.fetch(out_gt, d_fe, levels * Fp12::BYTES);
    if (K) {
        sg.fetch(out_gt + 48 * (levels + 1), d_fe + 48 * levels, K * Fp12::BYTES);
        sg.fetch(out_gt + 48 * (2 * levels + 1), d_fe + 48 * (levels + K), K * Fp12::BYTES);
    }
    ZG_TRY(sg.finish());
    dv_gt_one(out_gt + 48 * levels);
    dv_gt_one(out_gt + 48 * 2 * levels);
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

size_t zg_dory_verifier_setup_levels(size_t n_g1) {
    size_t levels = 0;
    while (n_g1 >> levels) levels++;  // floor(log2 n_g1) + 1; 0 for 0
    return levels;
}

int zg_dory_verifier_setup(zg_dory_key_t key, uint64_t *out_gt, size_t levels_cap, size_t *out_levels) {
    const char *who = "zg_dory_verifier_setup";
    if (!key) return invalid(who, "null key");
    uint32_t K = 0;
    ZG_TRY(dv_validate(who, key->n_g1, key->n_g2, out_gt, levels_cap, K));
    ZG_INIT();
    DeviceGuard dg(key->device);
    std::lock_guard<std::mutex> lk(key->mu);
    Staging sg(lib_stream());
    ZG_TRY(dv_run(sg, key->g1, key->g1_inf, key->g2, key->g2_inf, K, out_gt));
    if (out_levels) *out_levels = (size_t)K + 1;
    return ZG_OK;
}

int zg_dory_verifier_setup_points(const uint64_t *g1_xy, const uint8_t *g1_inf, size_t n_g1, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n_g2,
                                  uint64_t *out_gt, size_t levels_cap, size_t *out_levels) {
    const char *who = "zg_dory_verifier_setup_points";
    if (!g1_xy || !g2_xy) return invalid(who, "null points");
    uint32_t K = 0;
    ZG_TRY(dv_validate(who, n_g1, n_g2, out_gt, levels_cap, K));
    ZG_INIT();
    const size_t N = (size_t)1 << K;  // the generators beyond are not read, so they do not cross
    Staging sg(lib_stream());
    const uint64_t *d_g1 = sg.in(g1_xy, N * 64), *d_g2 = sg.in(g2_xy, N * 128);
    const uint8_t *d_g1i = sg.in(g1_inf, N), *d_g2i = sg.in(g2_inf, N);
    ZG_TRY(dv_run(sg, d_g1, d_g1i, d_g2, d_g2i, K, out_gt));
    if (out_levels) *out_levels = (size_t)K + 1;
    return ZG_OK;
}

}  // extern "C"
