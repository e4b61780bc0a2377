// pairing_wave.hip.h — the optimal ate pairing of BN254 as one WAVEFRONT computes it (device side): pair_miller and pair_final_exp of
// pairing.hip.h over the cooperative tower of fp12_wave.hip.h. The same step formulas — double_in_place, add_in_place, mulByChar, the
// line at w^0, w^1, w^3, the 65 signed digits, the same hard-part chain — so every value, the unreduced Miller value included, has the
// bits of the lane engine's: all of them are canonical field elements.
//
// The Miller value f is an Fp12 column per lane. The point R = (x, y, z), P and Q are REPLICATED: every lane holds them. The Fp2
// products of a step are grouped into levels of independent products (fp12_wave_map.hip.h: 5, 3, 4 for a doubling, 2, 6, 3, 4 for an
// addition, the line's scalings by x_P and y_P among them); product s of a level is formed by lane 36 + s and read back by all lanes,
// which then do the step's additions for themselves. The first level of a doubling runs in the instructions of f^2, and the first level
// of an addition in those of f * line, in lanes the Fp12 product leaves idle. A doubling turn (f^2, the step, f * line) is 4 Fp2 products
// deep where the lane engine runs about 39 one after another; an addition 4 more where it runs 28.
//
// The two halvings of double_in_place (products by 1/2 in the lane engine) are a conditional addition of p and a shift: the same element.
#pragma once
#include "fp12_wave.hip.h"
#include "pairing.hip.h"

namespace zg {

// x / 2: x even -> x >> 1, x odd -> (x + p) >> 1; x + p < 2^255. The Montgomery form of x / 2 is half the Montgomery form of x.
ZG_DEV Fp pw_half(const Fp &a) {
    const u32 mask = 0u - (a.l[0] & 1u);
    u32 s[8], carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = __builtin_addc(a.l[i], FpParams::MOD[i] & mask, carry, &carry);
    Fp r;
#pragma unroll
    for (int i = 0; i < 7; i++) r.l[i] = (s[i] >> 1) | (s[i + 1] << 31);
    r.l[7] = s[7] >> 1;
    return r;
}
ZG_DEV Fp2 pw_half(const Fp2 &a) { return Fp2{pw_half(a.c0), pw_half(a.c1)}; }

// the operand of product s of a level, in lane 36 + s (any value elsewhere: nobody reads those products)
ZG_DEV Fp2 pw_pick(int s, const Fp2 &a0, const Fp2 &a1) { return fpw_sel(s == 1, a1, a0); }
ZG_DEV Fp2 pw_pick(int s, const Fp2 &a0, const Fp2 &a1, const Fp2 &a2) { return fpw_sel(s == 2, a2, pw_pick(s, a0, a1)); }
ZG_DEV Fp2 pw_pick(int s, const Fp2 &a0, const Fp2 &a1, const Fp2 &a2, const Fp2 &a3) { return fpw_sel(s == 3, a3, pw_pick(s, a0, a1, a2)); }
ZG_DEV Fp2 pw_pick(int s, const Fp2 &a0, const Fp2 &a1, const Fp2 &a2, const Fp2 &a3, const Fp2 &a4) {
    return fpw_sel(s == 4, a4, pw_pick(s, a0, a1, a2, a3));
}
ZG_DEV Fp2 pw_pick(int s, const Fp2 &a0, const Fp2 &a1, const Fp2 &a2, const Fp2 &a3, const Fp2 &a4, const Fp2 &a5) {
    return fpw_sel(s == 5, a5, pw_pick(s, a0, a1, a2, a3, a4));
}
ZG_DEV Fp2 pw_take(const Fp2 &t, int s) { return fpw_shfl(t, pw_side_lane(s)); }
ZG_DEV Fp2 pw_embed(const Fp &a) { return Fp2{a, Fp::zero()}; }

// millerLoopArkworks for P, Q that are not the identity, a wavefront per pair: the lane's column of the value. The closing steps with
// pi(Q) and -pi^2(Q) are two more turns of the one loop (idx 0 and -1) that have an addition and no doubling.
ZG_DEV Fp2 pairw_miller(const Affine &p, const G2Affine &q) {
    const int lane = fpw_lane(), s = lane - FPW_SIDE0;
    const Fp2 px = pw_embed(p.x), py = pw_embed(p.y);
    Fp2 x = q.x, y = q.y, z = Fp2::one();
    Fp2 f = fpw_one(lane);
    G2Affine qc = q;  // pi(Q), then -pi^2(Q)
#pragma unroll 1
    for (int idx = 64; idx >= -1; idx--) {
        const bool dbl = idx >= 1;
        Fp2 line = Fp2::zero();
        if (dbl) {
            // level 0, with f^2 (one squared at the top digit is one): x y, y^2, z^2, (y + z)^2, x^2
            const Fp2 yz = fe_add(y, z);
            const FpwPair m0 = fpw_mul_side(f, f, pw_pick(s, x, y, z, yz, x), pw_pick(s, y, y, z, yz, x));
            f = m0.f;
            const Fp2 xy = pw_take(m0.t, 0), b = pw_take(m0.t, 1), c = pw_take(m0.t, 2), yz2 = pw_take(m0.t, 3), j = pw_take(m0.t, 4);
            const Fp2 h = fe_sub(yz2, fe_add(b, c));
            // level 1: e = 3 c b', the line's -h y_P and 3 j x_P
            const Fp2 t1 = fpw_fp2_mul(pw_pick(s, fp2_mul3(c), fe_neg(h), fp2_mul3(j)), pw_pick(s, g2_b_twist(), py, px));
            const Fp2 e = pw_take(t1, 0), l0 = pw_take(t1, 1), l1 = pw_take(t1, 2);
            // level 2: e^2, a (b - f), g^2, b h
            const Fp2 a = pw_half(xy), f3 = fp2_mul3(e), g = pw_half(fe_add(b, f3));
            const Fp2 t2 = fpw_fp2_mul(pw_pick(s, e, a, g, b), pw_pick(s, e, fe_sub(b, f3), g, h));
            x = pw_take(t2, 1);
            y = fe_sub(pw_take(t2, 2), fp2_mul3(pw_take(t2, 0)));
            z = pw_take(t2, 3);
            line = fpw_line(l0, l1, fe_sub(e, b), lane);
        }
        bool add = true;
        G2Affine qa = qc;
        if (dbl) {  // uniform: the digits are constants
            const bool plus = (PAIR_LOOP_PLUS >> (idx - 1)) & 1ull, minus = (PAIR_LOOP_MINUS >> (idx - 1)) & 1ull;
            add = plus || minus;
            qa = G2Affine{q.x, minus ? fe_neg(q.y) : q.y};
        } else {
            qc = G2Affine{fpw_fp2_mul(fp2_conj(qc.x), pair_gamma(1, 2)), fpw_fp2_mul(fp2_conj(qc.y), pair_gamma(1, 3))};  // mulByChar
            qa = G2Affine{qc.x, idx == 0 ? qc.y : fe_neg(qc.y)};
        }
        // level 0 of the addition, q.y z and q.x z, with f * line where there is one
        const Fp2 u0 = pw_pick(s, qa.y, qa.x);
        Fp2 t0;
        if (dbl) {
            const FpwPair m = fpw_mul_side(f, line, u0, z);
            f = m.f;
            t0 = m.t;
        } else {
            t0 = fpw_fp2_mul(u0, z);
        }
        if (!add) continue;
        const Fp2 theta = fe_sub(y, pw_take(t0, 0)), lambda = fe_sub(x, pw_take(t0, 1));
        // level 1: theta^2, lambda^2, theta q.x, lambda q.y, the line's lambda y_P and -theta x_P
        const Fp2 t1 = fpw_fp2_mul(pw_pick(s, theta, lambda, theta, lambda, lambda, fe_neg(theta)), pw_pick(s, theta, lambda, qa.x, qa.y, py, px));
        const Fp2 c = pw_take(t1, 0), d = pw_take(t1, 1);
        line = fpw_line(pw_take(t1, 4), pw_take(t1, 5), fe_sub(pw_take(t1, 2), pw_take(t1, 3)), lane);
        // level 2: e = lambda d, f = z c, g = x d
        const Fp2 t2 = fpw_fp2_mul(pw_pick(s, lambda, z, x), pw_pick(s, d, c, d));
        const Fp2 e = pw_take(t2, 0), g = pw_take(t2, 2);
        const Fp2 h = fe_sub(fe_add(e, pw_take(t2, 1)), fe_dbl(g));
        // level 3: lambda h, theta (g - h), e y, z e
        const Fp2 t3 = fpw_fp2_mul(pw_pick(s, lambda, theta, e, z), pw_pick(s, h, fe_sub(g, h), y, e));
        x = pw_take(t3, 0);
        y = fe_sub(pw_take(t3, 1), pw_take(t3, 2));
        z = pw_take(t3, 3);
        f = fpw_mul(f, line);
    }
    return f;
}

// finalExponentiation, a wavefront per value: pair_final_exp's chain step for step
ZG_DEV Fp2 pairw_final_exp(const Fp2 &f) {
    const int lane = fpw_lane();
    if (fpw_is_zero(f)) return fpw_one(lane);
    Fp2 r, t, y1, y3, y4, y6, y8, y9;
    t = fpw_inv(f);
    r = fpw_conj(f, lane);
    t = fpw_mul(r, t);             // f^(p^6 - 1)
    r = fpw_frobenius(t, 2);
    r = fpw_mul(r, t);             // r = f^((p^6 - 1)(p^2 + 1))
    t = fpw_conj(fpw_exp_by_x(r), lane);   // y0
    y1 = fpw_mul(t, t);            // y1 = y0^2
    t = fpw_mul(y1, y1);           // y2
    y3 = fpw_mul(t, y1);           // y3 = y2 y1
    y4 = fpw_conj(fpw_exp_by_x(y3), lane); // y4 = y3^-x
    t = fpw_mul(y4, y4);           // y5
    y6 = fpw_exp_by_x(t);
    y3 = fpw_conj(y3, lane);
    t = fpw_mul(y6, y4);           // y7
    y8 = fpw_mul(t, y3);           // y8
    y9 = fpw_mul(y8, y1);          // y9
    t = fpw_mul(y8, y4);           // y10
    t = fpw_mul(t, r);             // y11
    y1 = fpw_frobenius(y9, 1);     // y12
    t = fpw_mul(y1, t);            // y13
    y8 = fpw_frobenius(y8, 2);
    t = fpw_mul(y8, t);            // y14
    r = fpw_conj(r, lane);
    y9 = fpw_mul(r, y9);           // y15
    y9 = fpw_frobenius(y9, 3);
    return fpw_mul(y9, t);         // y16
}

}  // namespace zg
