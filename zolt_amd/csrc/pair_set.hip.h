// pair_set.hip.h — the Miller loops of a SET of pairs, for both pairing engines: one kernel template per engine and the one enqueue
// that chooses between them. What differs between the library's pair sets is only how pair i names its operands, so each set is a
// picker: a small struct passed to the kernel BY VALUE whose device-side operator()(uint32_t i) returns a PairOperands. The pickers live
// with their decoders — PlainPairs (pairing.hip), DorySegPairs (dory.hip), DcRowPairs (dory_commit.hip), DvPairs (dory_vsetup.hip).
// Miller value i goes to out + 48 i, so pair_product_kernel and the final exponentiation follow whatever the set. A set has at most
// 2^24 pairs: the pair index is 32 bits wide, and a picker widens it where it scales it into an address.
#pragma once
#include "common.hip.h"
#include "pairing.hip.h"
#include "pairing_wave.hip.h"

namespace zg {

struct PairOperands {
    const uint64_t *p, *q;  // an affine G1 point (8 words) and an affine G2 point (16 words); not read when `one`
    bool one;               // the pair's value is one without a loop: an identity on either side (src/field/pairing.zig:1562-1564)
};

// LANE: a lane per pair, the value of millerLoopArkworks (src/field/pairing.zig:1561-1628) by pair_miller
template <class Pick>
__global__ void __launch_bounds__(64) pair_set_miller_kernel(Pick pick, uint32_t n, uint64_t *out /* n * 48 */) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const PairOperands pr = pick(i);
    Fp12 f = fp12_one();
    if (!pr.one) {
        const Affine p = affine_load(pr.p);
        const G2Affine q = affine_load<Fp2>(pr.q);
        pair_miller(f, p, q);
        if (fp12_is_zero(f)) f = fp12_one();  // no point of the curves gives zero; what finalExponentiation would answer for it
    }
    fp12_store(out + 48 * (size_t)i, f);
}

// WAVE: a wavefront per pair, one wave per workgroup; the pair is blockIdx.x, a scalar, so `one` and every branch on it are uniform
template <class Pick>
__global__ void __launch_bounds__(64) pair_set_millerw_kernel(Pick pick, uint32_t n, uint64_t *out /* n * 48 */) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const PairOperands pr = pick(i);
    const int lane = fpw_lane();
    Fp2 f = fpw_one(lane);
    if (!pr.one) {
        f = pairw_miller(affine_load(pr.p), affine_load<Fp2>(pr.q));
        if (fpw_is_zero(f)) f = fpw_one(lane);  // as the lane engine
    }
    fpw_store(out + 48 * (size_t)i, f, lane);
}

// The n Miller values of `pick`'s set into d_out on st; nothing is launched for n == 0. `engine` is what the entry point read from
// pairing_engine() when it was called; this is the one place that chooses a Miller kernel by it.
template <class Pick>
static void pair_set_miller_enqueue(const Pick &pick, size_t n, hipStream_t st, uint64_t *d_out, int engine) {
    if (!n) return;
    if (engine == ZG_PAIRING_ENGINE_WAVE) hipLaunchKernelGGL(pair_set_millerw_kernel<Pick>, dim3((unsigned)n), dim3(64), 0, st, pick, (uint32_t)n, d_out);
    else hipLaunchKernelGGL(pair_set_miller_kernel<Pick>, dim3(div_up(n, 64)), dim3(64), 0, st, pick, (uint32_t)n, d_out);
}

}  // namespace zg
