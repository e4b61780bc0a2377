// pairing.hip.h — the optimal ate pairing of BN254 as one lane computes it (device side): the Miller loop and the final exponentiation of
// src/field/pairing.zig over the tower of fp12.hip.h. pairing.hip has the kernels and the entry points; tests/cpp/pairing_host.cpp
// compiles this header for the host.
//
// The steps restate the reference's formulas one for one — double_in_place (:948-997), add_in_place (:1001-1032), mulByChar (:1088-1100),
// the line placed at w^0, w^1, w^3, the 65 signed digits of 6x + 2 — so the UNREDUCED Miller value is the reference's too, not only the
// pairing. Real functions, references, no recursion, as fp12.hip.h explains.
#pragma once
#include "fp12.hip.h"
#include "g1.hip.h"
#include "g2.hip.h"

namespace zg {

// G2HomProjective (pairing.zig:933-1033): (x, y, z) with affine x/z, y/z; EllCoeff: a line's three coefficients
struct G2Hom {
    Fp2 x, y, z;
};
struct Ell {
    Fp2 c0, c1, c2;
};

ZG_DEV Fp pair_two_inv() {
    Fp h;
#pragma unroll
    for (int i = 0; i < 8; i++) h.l[i] = PAIR_TWO_INV[i];
    return h;
}

// double_in_place (:948-997): R = 2R, line (-h, 3j, i)
ZG_DEV_CALL void pair_double_step(G2Hom &r, Ell &l) {
    const Fp half = pair_two_inv();
    const Fp2 a = fp2_scale(fe_mul(r.x, r.y), half);
    const Fp2 b = fe_sqr(r.y), c = fe_sqr(r.z);
    const Fp2 e = fe_mul(fp2_mul3(c), g2_b_twist());
    const Fp2 f = fp2_mul3(e);
    const Fp2 g = fp2_scale(fe_add(b, f), half);
    const Fp2 h = fe_sub(fe_sqr(fe_add(r.y, r.z)), fe_add(b, c));
    const Fp2 j = fe_sqr(r.x);
    const Fp2 e2 = fe_sqr(e);
    r.x = fe_mul(a, fe_sub(b, f));
    r.y = fe_sub(fe_sqr(g), fp2_mul3(e2));
    r.z = fe_mul(b, h);
    l.c0 = fe_neg(h);
    l.c1 = fp2_mul3(j);
    l.c2 = fe_sub(e, b);
}

// add_in_place (:1001-1032): R = R + Q for an affine Q, line (lambda, -theta, theta q.x - lambda q.y)
ZG_DEV_CALL void pair_add_step(G2Hom &r, const G2Affine &q, Ell &l) {
    const Fp2 theta = fe_sub(r.y, fe_mul(q.y, r.z));
    const Fp2 lambda = fe_sub(r.x, fe_mul(q.x, r.z));
    const Fp2 c = fe_sqr(theta), d = fe_sqr(lambda);
    const Fp2 e = fe_mul(lambda, d);
    const Fp2 f = fe_mul(r.z, c);
    const Fp2 g = fe_mul(r.x, d);
    const Fp2 h = fe_sub(fe_add(e, f), fe_dbl(g));
    r.x = fe_mul(lambda, h);
    r.y = fe_sub(fe_mul(theta, fe_sub(g, h)), fe_mul(e, r.y));
    r.z = fe_mul(r.z, e);
    l.c0 = lambda;
    l.c1 = fe_neg(theta);
    l.c2 = fe_sub(fe_mul(theta, q.x), fe_mul(lambda, q.y));
}

// the line at P into f: c0 * y_P at w^0, c1 * x_P at w, c2 at v w (:1586-1589)
ZG_DEV_CALL void pair_ell(Fp12 &f, const Ell &l, const Affine &p) {
    const Fp2 c0 = fp2_scale(l.c0, p.y), c1 = fp2_scale(l.c1, p.x);
    fp12_mul_by_034(f, c0, c1, l.c2);
}

// mulByChar (:1088-1100): (x, y) -> (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))
ZG_DEV G2Affine pair_mul_by_char(const G2Affine &q) {
    return G2Affine{fe_mul(fp2_conj(q.x), pair_gamma(1, 2)), fe_mul(fp2_conj(q.y), pair_gamma(1, 3))};
}

// millerLoopArkworks (:1561-1628) for P, Q that are not the identity: 64 doubling steps from the top digit of 6x + 2 down, an addition
// step of +-Q at every non-zero digit, then the two closing steps with pi(Q) and -pi^2(Q)
ZG_DEV_CALL void pair_miller(Fp12 &out, const Affine &p, const G2Affine &q) {
    G2Hom r = G2Hom{q.x, q.y, Fp2::one()};
    const G2Affine neg_q = G2Affine{q.x, fe_neg(q.y)};
    Fp12 f = fp12_one();
    Ell l;
#pragma unroll 1
    for (int idx = 64; idx >= 1; idx--) {
        if (idx != 64) fp12_sqr(f, f);
        pair_double_step(r, l);
        pair_ell(f, l, p);
        const bool plus = (PAIR_LOOP_PLUS >> (idx - 1)) & 1ull, minus = (PAIR_LOOP_MINUS >> (idx - 1)) & 1ull;
        if (plus || minus) {  // uniform over the launch: the digits are constants
            pair_add_step(r, plus ? q : neg_q, l);
            pair_ell(f, l, p);
        }
    }
    const G2Affine q1 = pair_mul_by_char(q);
    pair_add_step(r, q1, l);
    pair_ell(f, l, p);
    G2Affine q2 = pair_mul_by_char(q1);
    q2.y = fe_neg(q2.y);
    pair_add_step(r, q2, l);
    pair_ell(f, l, p);
    out = f;
}

// finalExponentiation (:1653-1681): zero -> one; f^((p^6 - 1)(p^2 + 1)), then the hard part (:1812-1880) step by step — the
// Fuentes-Castaneda chain, which realises 2x(6x^2 + 3x + 1) (p^4 - p^2 + 1) / r, NOT (p^4 - p^2 + 1) / r
ZG_DEV_CALL void pair_final_exp(Fp12 &out, const Fp12 &f) {
    if (fp12_is_zero(f)) {  // a non-zero element of the field is invertible: the reference's second guard (:1664) is this one
        out = fp12_one();
        return;
    }
    Fp12 r, t, y1, y3, y4, y6, y8, y9;
    fp12_inv(t, f);
    r = fp12_conj(f);
    fp12_mul(t, r, t);         // f^(p^6 - 1)
    fp12_frobenius(r, t, 2);
    fp12_mul(r, r, t);         // r = f^((p^6 - 1)(p^2 + 1)): cyclotomic, conj = inverse
    fp12_exp_by_x(t, r);
    t = fp12_conj(t);          // y0 = r^-x
    fp12_sqr(y1, t);           // y1 = y0^2
    fp12_sqr(t, y1);           // y2 = y1^2
    fp12_mul(y3, t, y1);       // y3 = y2 y1
    fp12_exp_by_x(y4, y3);
    y4 = fp12_conj(y4);        // y4 = y3^-x
    fp12_sqr(t, y4);           // y5 = y4^2
    fp12_exp_by_x(y6, t);      // conj(y6 of the reference) = y5^x
    y3 = fp12_conj(y3);
    fp12_mul(t, y6, y4);       // y7 = y6 y4
    fp12_mul(y8, t, y3);       // y8 = y7 y3
    fp12_mul(y9, y8, y1);      // y9 = y8 y1
    fp12_mul(t, y8, y4);       // y10 = y8 y4
    fp12_mul(t, t, r);         // y11 = y10 r
    fp12_frobenius(y1, y9, 1); // y12
    fp12_mul(t, y1, t);        // y13 = y12 y11
    fp12_frobenius(y8, y8, 2);
    fp12_mul(t, y8, t);        // y14 = y8^(p^2) y13
    r = fp12_conj(r);
    fp12_mul(y9, r, y9);       // y15 = r^-1 y9
    fp12_frobenius(y9, y9, 3);
    fp12_mul(out, y9, t);      // y16
}

}  // namespace zg
