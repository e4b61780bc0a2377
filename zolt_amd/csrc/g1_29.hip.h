// g1_29.hip.h — the MSM inner loop's group law on lazy 29-bit-limb field elements (fp29.hip.h).
//
// Same madd-2008-s formulas as g1.hip.h:xyzz_madd (the reference's addAffine, src/msm/mod.zig:229-274),
// with the reduction bounds tracked statically instead of conditional subtractions:
//
//   class            bound      where
//   point x, y       < 1.1 p    table rows (f29_from_fp outputs); negated y = 2p - y <= 2p
//   M (mul output)   < 1.6 p    every f29_mul / f29_sqr below has input classes A*B <= 101
//   acc.x            < 6.6 p    X3 = R^2 + 5p - PPP - 2Q
//   acc.y            < 1.4 p    Y3 = (R*(Q - X3) + (4p - Y1)*PPP) * 2^-261, one reduction: (5.6*8.6 + 4*1.6)/168.9 + 1
//   P  = U2 + 7p - X1  < 8.6 p,  R = S2 + 4p - Y1 < 5.6 p,  Q + 7p - X3 < 8.6 p
//   R for a subtracted point (the accumulate loop folds the digit's sign in here instead of negating y): 5p - S2 - Y1, in (1.4p, 5p)
//   for S2 < 1.6p and Y1 <= 2p. The 5p bias covers two near-normalised subtrahends (< 2^29 + 8 each) without underflow, and its top
//   limb (0xf1f584 or more) exceeds the top limbs of S2 + Y1 < 3.6p (< 0xae3600; fp29.hip.h: f29_pmsub45), so R stays < 5.6 p for
//   either sign.
//
// Limbs. Those are bounds on VALUES. The mixed addition (xyzz29_madd_nz) feeds three of its linear forms to the multiplier
// un-carried: P, R and 4p - Y1 (fp29.hip.h: f29_sub7_raw, f29_pmsub45_raw, f29_neg4_raw), whose limbs 0..7 reach Li(kp) + 2^30
// (< 3 * 2^29) instead of 2^29 + 8. The values, and so every product, are what the carried forms give. What the larger limbs cost
// is column headroom: every column of the ten products (terms, reduction terms and carry-in) stays < 2^64, UNSIGNED — not < 2^63
// as with near-normalised operands. The largest, in units of 2^58 against a limit of 64 (tests/test_lazy_g1_headroom.py computes
// them from per-limb maxima, every reduction term counted as 2^58, and is the authority): PP = P^2 53.5, R^2 53.3, PPP 27.0,
// Y3 38.0; Q, ZZ3, ZZZ3, U2, S2 16.0 as before. Nothing signed touches an accumulator: u64 in the compiler forms (>> is logical),
// v_mad_u64_u32 and v_lshrrev_b64 in the asm forms, and only the low 32 bits are ever read otherwise. Q + 7p - X3 keeps its carry
// pass: un-carried, the same accounting puts a column of Y3 at 64.6. X3 keeps its own because it is stored as acc.x and
// multiplied in the next addition.
//
// The exceptional cases of a mixed add (acc == P -> double, acc == -P -> infinity) are detected
// exactly (f29_is_zero_modp on P, then on R) and finished from the point through the canonical-form code (xyzz29_madd_except).
#pragma once
#include "fp29.hip.h"
#include "g1.hip.h"

namespace zg {

struct XYZZ29 {
    F29 x, y, zz, zzz;
};

ZG_DEV XYZZ xyzz29_to_std(const XYZZ29 &a, bool inf) {
    if (inf) return XYZZ::identity();
    XYZZ r;
    r.x = f29_to_fp(a.x); r.y = f29_to_fp(a.y); r.zz = f29_to_fp(a.zz); r.zzz = f29_to_fp(a.zzz);
    return r;
}
ZG_DEV void xyzz29_from_std(const XYZZ &s, XYZZ29 &a, bool &inf) {
    inf = s.is_identity();
    a.x = f29_from_fp(s.x); a.y = f29_from_fp(s.y); a.zz = f29_from_fp(s.zz); a.zzz = f29_from_fp(s.zzz);
}

// acc = (px, py): the first addition of a bucket run
ZG_DEV void xyzz29_start(XYZZ29 &a, const F29 &px, const F29 &py) {
    a.x = px; a.y = py;
#pragma unroll
    for (int i = 0; i < 9; i++) { a.zz.l[i] = Fp29::ONE[i]; a.zzz.l[i] = Fp29::ONE[i]; }
}

// acc += (px, +-py) for an accumulator that is not the identity; (px, py) is an affine point in lazy form, never infinity, and
// neg is 0 or ~0 (subtract the point). The sign enters at R = +-S2 - Y1 only (f29_pmsub45): Y1 * PPP in Y3 does not depend on it.
// Returns 0 in the regular case. Otherwise acc was +-P, the formulas do not apply and `a` holds nothing useful: 1 = acc was -P (the
// sum is infinity), 2 = acc was P (the sum is 2P). The caller then finishes with xyzz29_madd_except, which needs the point only, not
// the old accumulator — so that case can run AFTER the regular one, and the regular one may overwrite the accumulator in place.
// CARRY_ALL: P, R and 4p - Y1 through the carried forms (f29_sub7, f29_pmsub45, f29_neg4), as before the un-carried ones: the same
// results limb for limb, 70 vector instructions more on the loop's steady path. The build switch ZG_F29_CARRY_ALL selects it for A/B runs, and the self-test
// runs both from one binary (lazy_selftest.hip.h).
template <bool CARRY_ALL>
ZG_DEV u32 xyzz29_madd_nz_t(XYZZ29 &a, const F29 &px, const F29 &py, u32 neg) {
#ifdef ZG_F29_SERIAL  // build switch: the products one at a time (the schedule before the interleaved groups), for A/B runs
    F29 U2 = f29_mul(px, a.zz);
    F29 S2 = f29_mul(py, a.zzz);
#else
    F29 U2, S2;
    f29_mul_x2(U2, px, a.zz, S2, py, a.zzz);
#endif
    F29 Pp = CARRY_ALL ? f29_sub7(U2, a.x) : f29_sub7_raw(U2, a.x);
    F29 R = CARRY_ALL ? f29_pmsub45(S2, a.y, neg) : f29_pmsub45_raw(S2, a.y, neg);
    u32 exc = 0;
#ifndef ZG_EXP_NOSLOW
    // same x: P == acc (double) or P == -acc (infinity) — rare. The zero test takes P and R carried or not (fp29.hip.h).
    if (f29_is_zero_modp(Pp)) exc = f29_is_zero_modp(R) ? 2u : 1u;
#endif
#ifdef ZG_F29_SERIAL
    F29 PP = f29_sqr(Pp);
    F29 PPP = f29_mul(Pp, PP);
    F29 Q = f29_mul(a.x, PP);
    F29 X3 = f29_x3(f29_sqr(R), PPP, Q);
    F29 Y3 = f29_mul2(R, f29_sub7(Q, X3), CARRY_ALL ? f29_neg4(a.y) : f29_neg4_raw(a.y), PPP);  // R*(Q - X3) - Y1*PPP, one reduction
    a.zz = f29_mul(a.zz, PP);
    a.zzz = f29_mul(a.zzz, PPP);
    a.x = X3;
    a.y = Y3;
#else
    // the same ten products in four groups of independent ones (fp29.hip.h: f29_mul_x2 ...): (U2, S2) above, then
    // (PP, R^2), (PPP, Q, ZZ3), (Y3, ZZZ3)
    F29 PP, RR, PPP, Q, ZZ3, Y3, ZZZ3;
    f29_sqr_x2(PP, Pp, RR, R);
    f29_mul_x3(PPP, Pp, PP, Q, a.x, PP, ZZ3, a.zz, PP);
    F29 X3 = f29_x3(RR, PPP, Q);
    f29_mul2_mul(Y3, R, f29_sub7(Q, X3), CARRY_ALL ? f29_neg4(a.y) : f29_neg4_raw(a.y), PPP, ZZZ3, a.zzz, PPP);  // Y3 = R*(Q - X3) - Y1*PPP, one reduction
    a.x = X3;
    a.y = Y3;
    a.zz = ZZ3;
    a.zzz = ZZZ3;
#endif
    return exc;
}
ZG_DEV u32 xyzz29_madd_nz(XYZZ29 &a, const F29 &px, const F29 &py, u32 neg) {
#ifdef ZG_F29_CARRY_ALL  // build switch: the carried forms of P, R and 4p - Y1, for A/B runs
    return xyzz29_madd_nz_t<true>(a, px, py, neg);
#else
    return xyzz29_madd_nz_t<false>(a, px, py, neg);
#endif
}
// the exceptional cases of xyzz29_madd_nz (exc != 0), through the canonical-form code
ZG_DEV void xyzz29_madd_except(XYZZ29 &a, bool &inf, const F29 &px, const F29 &py, u32 neg, u32 exc) {
    if (exc == 2u) {
        Affine q;
        q.x = f29_to_fp(px); q.y = f29_to_fp(neg ? f29_neg2(py) : py);
        xyzz29_from_std(xyzz_dbl_affine(q), a, inf);
    } else {
        inf = true;
    }
}

// acc += (px, py); (px, py) is an affine point in lazy form, never infinity
ZG_DEV void xyzz29_madd(XYZZ29 &a, bool &inf, const F29 &px, const F29 &py) {
    if (inf) {
        xyzz29_start(a, px, py);
        inf = false;
        return;
    }
    u32 exc = xyzz29_madd_nz(a, px, py, 0u);
    if (exc) xyzz29_madd_except(a, inf, px, py, 0u, exc);
}

// ---- full group law on lazy elements, for the bucket-reduction kernels.
// Identity is encoded as zz = all-zero limbs (a non-identity ZZ is a non-zero field element, whose lazy
// representative cannot be 0). Classes as above: X < 6.6p, Y < 1.4p, ZZ, ZZZ < 1.6p.
ZG_DEV XYZZ29 xyzz29_identity() {
    XYZZ29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) { r.x.l[i] = 0; r.y.l[i] = 0; r.zz.l[i] = 0; r.zzz.l[i] = 0; }
    return r;
}
ZG_DEV bool xyzz29_is_identity(const XYZZ29 &a) { return f29_all_zero(a.zz); }

ZG_DEV XYZZ29 xyzz29_from_std_val(const XYZZ &s) {
    if (s.is_identity()) return xyzz29_identity();
    XYZZ29 a;
    a.x = f29_from_fp(s.x); a.y = f29_from_fp(s.y); a.zz = f29_from_fp(s.zz); a.zzz = f29_from_fp(s.zzz);
    return a;
}
ZG_DEV XYZZ xyzz29_to_std_val(const XYZZ29 &a) { return xyzz29_to_std(a, xyzz29_is_identity(a)); }

// 2*P (dbl-2008-s-1)
ZG_DEV XYZZ29 xyzz29_dbl(const XYZZ29 &p) {
    if (xyzz29_is_identity(p)) return p;
    F29 U = f29_times2(p.y);            // < 2.8p
    F29 V = f29_sqr(U);
    F29 W = f29_mul(U, V);
    F29 S = f29_mul(p.x, V);
    F29 M = f29_times3(f29_sqr(p.x));   // < 4.8p
    XYZZ29 r;
    r.x = f29_sub4_2c(f29_sqr(M), S);   // < 5.6p
    r.y = f29_mul2(M, f29_sub7(S, r.x), W, f29_neg4(p.y));
    r.zz = f29_mul(V, p.zz);
    r.zzz = f29_mul(W, p.zzz);
    return r;
}

// Jacobian doubling on y^2 = x^3 + b for the table build's chains of doublings (msm_precompute_kernel): three squarings, two products and
// one two-product sum — 945 multiply-adds against the 1269 of xyzz29_dbl, which carries ZZ and ZZZ separately.
//   A = X^2, B = Y^2, D = 4 X B, E = 3 A, F = E^2:  X3 = F - 2 D,  Y3 = E (D - X3) - 8 B^2,  Z3 = 2 Y Z
// Classes (closed under the map, and an affine table row x, y < 1.1p with Z = one starts inside them): X < 5.3p, Y < 1.3p, Z < 1.1p;
// A < 1.2p, B < 1.1p, 4B < 4.1p, D < 1.2p, E < 3.6p, F < 1.1p, D + 7p - X3 < 8.2p, 8B < 8.2p:
// Y3 < ((3.6 * 8.2 + 2 * 8.2) / 168.9 + 1) p. Never called on the identity (the group has odd prime order: Y is never 0).
struct Jac29 {
    F29 x, y, z;
};
ZG_DEV Jac29 jac29_dbl(const Jac29 &p) {
    F29 A = f29_sqr(p.x);
    F29 B = f29_sqr(p.y);
    F29 B4 = f29_times4(B);
    F29 D = f29_mul(p.x, B4);
    F29 E = f29_times3(A);
    F29 F = f29_sqr(E);
    Jac29 r;
    r.x = f29_sub4_2c(F, D);  // F + 4p - 2D
    r.y = f29_mul2(E, f29_sub7(D, r.x), f29_neg2(B), f29_times2(B4));  // E (D - X3) + (2p - B) * 8B, one reduction
    r.z = f29_mul(f29_times2(p.y), p.z);
    return r;
}

// a + b (add-2008-s), complete
ZG_DEV XYZZ29 xyzz29_add(const XYZZ29 &a, const XYZZ29 &b) {
    if (xyzz29_is_identity(a)) return b;
    if (xyzz29_is_identity(b)) return a;
    F29 U1 = f29_mul(a.x, b.zz);
    F29 U2 = f29_mul(b.x, a.zz);
    F29 S1 = f29_mul(a.y, b.zzz);
    F29 S2 = f29_mul(b.y, a.zzz);
    F29 Pp = f29_sub2(U2, U1);
    F29 R = f29_sub2(S2, S1);
    if (f29_is_zero_modp(Pp)) {
        if (f29_is_zero_modp(R)) return xyzz29_dbl(a);
        return xyzz29_identity();
    }
    F29 PP = f29_sqr(Pp);
    F29 PPP = f29_mul(Pp, PP);
    F29 Q = f29_mul(U1, PP);
    XYZZ29 r;
    r.x = f29_x3(f29_sqr(R), PPP, Q);
    r.y = f29_mul2(R, f29_sub7(Q, r.x), f29_neg2(S1), PPP);
    r.zz = f29_mul(f29_mul(a.zz, b.zz), PP);
    r.zzz = f29_mul(f29_mul(a.zzz, b.zzz), PPP);
    return r;
}

// 144-byte records (4 x 9 u32), 16-byte aligned
ZG_DEV XYZZ29 xyzz29_load(const void *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    u32 w[36];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint4 v = q[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    XYZZ29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) { r.x.l[i] = w[i]; r.y.l[i] = w[9 + i]; r.zz.l[i] = w[18 + i]; r.zzz.l[i] = w[27 + i]; }
    return r;
}
ZG_DEV void xyzz29_store(void *p, const XYZZ29 &v) {
    u32 w[36];
#pragma unroll
    for (int i = 0; i < 9; i++) { w[i] = v.x.l[i]; w[9 + i] = v.y.l[i]; w[18 + i] = v.zz.l[i]; w[27 + i] = v.zzz.l[i]; }
    uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
ZG_DEV XYZZ29 xyzz29_shfl_down(const XYZZ29 &v, int delta) {
    XYZZ29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        r.x.l[i] = __shfl_down(v.x.l[i], delta, 64);
        r.y.l[i] = __shfl_down(v.y.l[i], delta, 64);
        r.zz.l[i] = __shfl_down(v.zz.l[i], delta, 64);
        r.zzz.l[i] = __shfl_down(v.zzz.l[i], delta, 64);
    }
    return r;
}

}  // namespace zg
