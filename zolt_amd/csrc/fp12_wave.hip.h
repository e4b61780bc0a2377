// fp12_wave.hip.h — the tower of fp12.hip.h held by a WAVEFRONT instead of a lane (device side, gfx950, wave64).
//
// An Fp12 value is one Fp2 per lane: lane L holds the coefficient of w^(L % 6), Fp12 = Fp2[w] / (w^6 - xi), the coefficient of w^k
// being c_{k & 1}.c_{k >> 1} of fp12.hip.h (the order fp12_frobenius uses). fp12_wave_map.hip.h has the lane map. A product is
// schoolbook over w: 36 lanes form one Fp2 product each, the partial products with i + j >= 6 are multiplied by xi, and six of them are
// summed per column — one Fp2 product deep (3 Fp products) where fp12_mul is 54 deep. The square is the product of a value with
// itself and the sparse product is the product with the zero-padded line: the depth is the same and there is one index algebra.
//
// Bounds: none to state. Every partial product is reduced by fe_mul and every sum is fe_add's, so each intermediate is a canonical
// element (< p) and the result has the bits of fp12.hip.h's whatever the order of the six additions.
//
// Exchange: __shfl (ds_bpermute_b32), 16 words per Fp2 — 16 to fetch a_i and 96 to gather a column's six terms. No LDS allocation, no
// barrier, no inline assembly. Every branch is on a launch constant or on a value all 64 lanes hold: the functions must be entered by
// whole wavefronts (blockDim.x a multiple of 64, a wave per element).
//
// One real function, a leaf: the Fp product, whose two operands and result travel as 8-word vectors in argument registers (an Fp2
// struct past a call's first travels through the private segment — fp2.hip.h's fe_mul does — and a function that calls another saves
// registers there). Everything else is inlined into the kernel, with its loops kept rolled, so a kernel built on this header has no
// private segment at all.
#pragma once
#include "fp12.hip.h"
#include "fp12_wave_map.hip.h"

namespace zg {

#ifndef ZG_WAVE_CALL
#define ZG_WAVE_CALL static __device__ __noinline__
#endif

typedef u32 FpwV __attribute__((ext_vector_type(8)));
ZG_DEV FpwV fpw_pack(const Fp &a) {
    FpwV v;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = a.l[i];
    return v;
}
ZG_DEV Fp fpw_unpack(const FpwV &v) {
    Fp a;
#pragma unroll
    for (int i = 0; i < 8; i++) a.l[i] = v[i];
    return a;
}
ZG_WAVE_CALL FpwV fpw_fp_mul_v(FpwV x, FpwV y) { return fpw_pack(fe_mul(fpw_unpack(x), fpw_unpack(y))); }
ZG_DEV Fp fpw_fp_mul(const Fp &x, const Fp &y) { return fpw_unpack(fpw_fp_mul_v(fpw_pack(x), fpw_pack(y))); }

// (a + bu)(c + du) = (ac - bd) + ((a + b)(c + d) - ac - bd) u, as fe_mul(Fp2, Fp2)
ZG_DEV Fp2 fpw_fp2_mul(const Fp2 &x, const Fp2 &y) {
    const Fp ac = fpw_fp_mul(x.c0, y.c0), bd = fpw_fp_mul(x.c1, y.c1);
    const Fp k = fpw_fp_mul(fe_add(x.c0, x.c1), fe_add(y.c0, y.c1));
    return Fp2{fe_sub(ac, bd), fe_sub(fe_sub(k, ac), bd)};
}

struct FpwPair {
    Fp2 f, t;  // an Fp12 column, and the lane's raw product
};

ZG_DEV int fpw_lane() { return (int)(threadIdx.x & 63u); }

ZG_DEV Fp2 fpw_shfl(const Fp2 &v, int src) {
    Fp2 r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r.c0.l[i] = __shfl(v.c0.l[i], src, 64);
        r.c1.l[i] = __shfl(v.c1.l[i], src, 64);
    }
    return r;
}
ZG_DEV Fp2 fpw_sel(bool c, const Fp2 &a, const Fp2 &b) {
    Fp2 r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r.c0.l[i] = c ? a.c0.l[i] : b.c0.l[i];
        r.c1.l[i] = c ? a.c1.l[i] : b.c1.l[i];
    }
    return r;
}

ZG_DEV Fp2 fpw_zero() { return Fp2::zero(); }
ZG_DEV Fp2 fpw_one(int lane) { return fpw_sel(fpw_col(lane) == 0, Fp2::one(), Fp2::zero()); }
// zero iff every column is: a vote, the same answer in all lanes
ZG_DEV bool fpw_is_zero(const Fp2 &a) { return !__any(!a.is_zero()); }
ZG_DEV Fp2 fpw_conj(const Fp2 &a, int lane) { return fpw_sel(fpw_col(lane) & 1, fe_neg(a), a); }  // the odd powers of w change sign

// GT word order: lane L reads the Fp2 of its column; lanes 0..5 write
ZG_DEV Fp2 fpw_load(const uint64_t *p, int lane) { return Fp2::load(p + 8 * fpw_mem_slot(fpw_col(lane))); }
ZG_DEV void fpw_store(uint64_t *p, const Fp2 &v, int lane) {
    if (lane < FPW_DEG) fe_store(p + 8 * fpw_mem_slot(lane), v);
}

// the lane's partial product t -> its column's coefficient
ZG_DEV Fp2 fpw_gather(Fp2 t, int lane) {
    t = fpw_sel(fpw_xi(lane), fp2_mul_xi(t), t);
    const int col = fpw_col(lane);
    Fp2 s = fpw_shfl(t, fpw_src(col, 0));
#pragma unroll
    for (int k = 1; k < FPW_DEG; k++) s = fe_add(s, fpw_shfl(t, fpw_src(col, k)));
    return s;
}

ZG_DEV Fp2 fpw_mul(const Fp2 &a, const Fp2 &b) {
    const int lane = fpw_lane();
    return fpw_gather(fpw_fp2_mul(fpw_shfl(a, fpw_row(lane)), b), lane);
}
ZG_DEV Fp2 fpw_sqr(const Fp2 &a) { return fpw_mul(a, a); }

// a * b in the busy lanes and, in the same instructions, the product u * v of every lane past them (a level of a Miller step): .f is
// the Fp12 product's column, .t the lane's own raw product
ZG_DEV FpwPair fpw_mul_side(const Fp2 &a, const Fp2 &b, const Fp2 &u, const Fp2 &v) {
    const int lane = fpw_lane();
    const bool busy = fpw_busy(lane);
    const Fp2 t = fpw_fp2_mul(fpw_sel(busy, fpw_shfl(a, fpw_row(lane)), u), fpw_sel(busy, b, v));
    return FpwPair{fpw_gather(t, lane), t};
}

// f times the sparse c0 + c3 w + c4 v w: the three coefficients are the same in all lanes
ZG_DEV Fp2 fpw_line(const Fp2 &c0, const Fp2 &c3, const Fp2 &c4, int lane) {
    const int slot = fpw_sparse_slot(fpw_col(lane));
    return fpw_sel(slot == 0, c0, fpw_sel(slot == 1, c3, fpw_sel(slot == 2, c4, Fp2::zero())));
}
ZG_DEV Fp2 fpw_mul_by_034(const Fp2 &f, const Fp2 &c0, const Fp2 &c3, const Fp2 &c4, int lane) { return fpw_mul(f, fpw_line(c0, c3, c4, lane)); }

// a^(p^n), n = 1, 2, 3: column k is conjugated n times and multiplied by xi^(k (p^n - 1) / 6) — one Fp2 product per lane, no exchange
ZG_DEV Fp2 fpw_frobenius(const Fp2 &a, int n) {
    const int col = fpw_col(fpw_lane());
    const Fp2 c = (n & 1) ? fp2_conj(a) : a;
    const Fp2 t = fpw_fp2_mul(c, pair_gamma(n, col ? col : 1));
    return fpw_sel(col != 0, t, c);
}

// 1 / a = conj(a) / (a conj(a)): a conj(a) = c0^2 - v c1^2 lies in Fp6 (the even columns), whose inverse — fp6_inv's formulas, one Fp
// inversion — every lane computes for itself from the three columns: the latency of one lane, once per final exponentiation.
// inverse(0) -> 0, as fp12_inv.
ZG_DEV Fp2 fpw_inv(const Fp2 &a) {
    const int lane = fpw_lane(), col = fpw_col(lane);
    const Fp2 ac = fpw_conj(a, lane);
    const Fp2 nrm = fpw_mul(a, ac);
    const Fp2 n0 = fpw_shfl(nrm, 0), n1 = fpw_shfl(nrm, 2), n2 = fpw_shfl(nrm, 4);
    const Fp2 A = fe_sub(fpw_fp2_mul(n0, n0), fp2_mul_xi(fpw_fp2_mul(n1, n2)));
    const Fp2 B = fe_sub(fp2_mul_xi(fpw_fp2_mul(n2, n2)), fpw_fp2_mul(n0, n1));
    const Fp2 C = fe_sub(fpw_fp2_mul(n1, n1), fpw_fp2_mul(n0, n2));
    const Fp2 F = fe_add(fpw_fp2_mul(n0, A), fp2_mul_xi(fe_add(fpw_fp2_mul(n2, B), fpw_fp2_mul(n1, C))));
    const Fp2 fi = fe_inv_safegcd(F);
    const Fp2 num = fpw_sel(col == 0, A, fpw_sel(col == 2, B, C));
    const Fp2 ni = fpw_sel(col & 1, Fp2::zero(), fpw_fp2_mul(num, fi));
    return fpw_mul(ac, ni);
}

// f^x, x = 4965661367192848881: plain squarings, any input (fp12_exp_by_x)
ZG_DEV Fp2 fpw_exp_by_x(const Fp2 &f) {
    Fp2 acc = f;
#pragma unroll 1
    for (int bit = 61; bit >= 0; bit--) {
        acc = fpw_mul(acc, acc);
        if ((PAIR_BN_X >> bit) & 1ull) acc = fpw_mul(acc, f);
    }
    return acc;
}

}  // namespace zg
