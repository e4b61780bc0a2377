// fp12.hip.h — the BN254 pairing tower Fp6 = Fp2[v] / (v^3 - xi), xi = 9 + u, and Fp12 = Fp6[w] / (w^2 - v), for gfx950 (device side).
//
// The values of the reference's Fp6 / Fp12 (src/field/pairing.zig:279-620), fp12MulBy034 (:1156-1189) and expByX (:1786-1800) on the
// canonical 8 x 32-bit Montgomery Fp of field.hip.h and the Fp2 of fp2.hip.h: every component of every result is canonical, so a
// value has the reference's bytes whatever sequence of field operations reaches it (Karatsuba products here, schoolbook there).
//
// Everything heavier than an addition is a REAL function (ZG_DEV_CALL), with operands and results behind references — an Fp12 is 96
// registers, three of them do not fit a call — so a lane's tower values live in its private segment. No recursion, no indirect call:
// every kernel built on these has a fixed private-segment size. An output may alias an input everywhere.
//
// In memory an Fp12 is 12 Fp elements in the order of Fp12.toBytes (:632-633): c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1 — the order
// of the struct's members.
#pragma once
#include "fp2.hip.h"
#include "pairing_consts.hip.h"

namespace zg {

struct Fp6 {
    Fp2 c0, c1, c2;  // c0 + c1 v + c2 v^2
};
struct Fp12 {
    Fp6 c0, c1;  // c0 + c1 w
    static constexpr int BYTES = 384, WORDS32 = 96;
};
static_assert(sizeof(Fp12) == Fp12::BYTES, "an Fp12 is 96 packed 32-bit limbs");

ZG_DEV Fp2 fp2_conj(const Fp2 &a) { return Fp2{a.c0, fe_neg(a.c1)}; }
// (a + bu)(9 + u) = (9a - b) + (a + 9b) u: additions only
ZG_DEV Fp2 fp2_mul_xi(const Fp2 &a) {
    const Fp2 a8 = fe_dbl(fe_dbl(fe_dbl(a)));
    return Fp2{fe_sub(fe_add(a8.c0, a.c0), a.c1), fe_add(fe_add(a8.c1, a.c1), a.c0)};
}
// an Fp2 value times an element of Fp (fp2ScalarMul), out of line like the Fp2 product
ZG_DEV_CALL Fp2 fp2_scale(Fp2 a, Fp s) { return fp2_mul_fp(a, s); }

ZG_DEV Fp6 fp6_zero() { return Fp6{Fp2::zero(), Fp2::zero(), Fp2::zero()}; }
ZG_DEV Fp6 fp6_one() { return Fp6{Fp2::one(), Fp2::zero(), Fp2::zero()}; }
ZG_DEV Fp6 fp6_add(const Fp6 &a, const Fp6 &b) { return Fp6{fe_add(a.c0, b.c0), fe_add(a.c1, b.c1), fe_add(a.c2, b.c2)}; }
ZG_DEV Fp6 fp6_sub(const Fp6 &a, const Fp6 &b) { return Fp6{fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1), fe_sub(a.c2, b.c2)}; }
ZG_DEV Fp6 fp6_neg(const Fp6 &a) { return Fp6{fe_neg(a.c0), fe_neg(a.c1), fe_neg(a.c2)}; }
ZG_DEV Fp6 fp6_mul_v(const Fp6 &a) { return Fp6{fp2_mul_xi(a.c2), a.c0, a.c1}; }  // v (c0 + c1 v + c2 v^2) = xi c2 + c0 v + c1 v^2
ZG_DEV bool fp6_is_zero(const Fp6 &a) { return a.c0.is_zero() && a.c1.is_zero() && a.c2.is_zero(); }

ZG_DEV Fp12 fp12_zero() { return Fp12{fp6_zero(), fp6_zero()}; }
ZG_DEV Fp12 fp12_one() { return Fp12{fp6_one(), fp6_zero()}; }
ZG_DEV bool fp12_is_zero(const Fp12 &a) { return fp6_is_zero(a.c0) && fp6_is_zero(a.c1); }
ZG_DEV Fp12 fp12_add(const Fp12 &a, const Fp12 &b) { return Fp12{fp6_add(a.c0, b.c0), fp6_add(a.c1, b.c1)}; }
ZG_DEV Fp12 fp12_sub(const Fp12 &a, const Fp12 &b) { return Fp12{fp6_sub(a.c0, b.c0), fp6_sub(a.c1, b.c1)}; }
ZG_DEV Fp12 fp12_neg(const Fp12 &a) { return Fp12{fp6_neg(a.c0), fp6_neg(a.c1)}; }
ZG_DEV Fp12 fp12_conj(const Fp12 &a) { return Fp12{a.c0, fp6_neg(a.c1)}; }  // = a^(p^6); the inverse of a cyclotomic element

ZG_DEV Fp12 fp12_load(const uint64_t *p) {
    Fp12 r;
    Fp2 *c[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
#pragma unroll
    for (int k = 0; k < 6; k++) *c[k] = Fp2::load(p + 8 * k);
    return r;
}
ZG_DEV void fp12_store(uint64_t *p, const Fp12 &v) {
    const Fp2 *c[6] = {&v.c0.c0, &v.c0.c1, &v.c0.c2, &v.c1.c0, &v.c1.c1, &v.c1.c2};
#pragma unroll
    for (int k = 0; k < 6; k++) fe_store(p + 8 * k, *c[k]);
}

// Karatsuba over v: six Fp2 products (the reference's schoolbook form spends nine, pairing.zig:331-358)
ZG_DEV_CALL void fp6_mul(Fp6 &r, const Fp6 &a, const Fp6 &b) {
    const Fp2 v0 = fe_mul(a.c0, b.c0), v1 = fe_mul(a.c1, b.c1), v2 = fe_mul(a.c2, b.c2);
    const Fp2 t0 = fe_sub(fe_sub(fe_mul(fe_add(a.c1, a.c2), fe_add(b.c1, b.c2)), v1), v2);
    const Fp2 t1 = fe_sub(fe_sub(fe_mul(fe_add(a.c0, a.c1), fe_add(b.c0, b.c1)), v0), v1);
    const Fp2 t2 = fe_sub(fe_sub(fe_mul(fe_add(a.c0, a.c2), fe_add(b.c0, b.c2)), v0), v2);
    r.c0 = fe_add(v0, fp2_mul_xi(t0));
    r.c1 = fe_add(t1, fp2_mul_xi(v2));
    r.c2 = fe_add(t2, v1);
}

// 1 / (c0 + c1 v + c2 v^2) = (A + B v + C v^2) / F with one Fp2 inversion, of the norm F; inverse(0) -> 0
ZG_DEV_CALL void fp6_inv(Fp6 &r, const Fp6 &a) {
    const Fp2 A = fe_sub(fe_sqr(a.c0), fp2_mul_xi(fe_mul(a.c1, a.c2)));
    const Fp2 B = fe_sub(fp2_mul_xi(fe_sqr(a.c2)), fe_mul(a.c0, a.c1));
    const Fp2 C = fe_sub(fe_sqr(a.c1), fe_mul(a.c0, a.c2));
    const Fp2 F = fe_add(fe_mul(a.c0, A), fp2_mul_xi(fe_add(fe_mul(a.c2, B), fe_mul(a.c1, C))));
    const Fp2 fi = fe_inv_safegcd(F);
    r.c0 = fe_mul(A, fi);
    r.c1 = fe_mul(B, fi);
    r.c2 = fe_mul(C, fi);
}

// Karatsuba over w: three Fp6 products
ZG_DEV_CALL void fp12_mul(Fp12 &r, const Fp12 &a, const Fp12 &b) {
    Fp6 aa, bb, m;
    fp6_mul(aa, a.c0, b.c0);
    fp6_mul(bb, a.c1, b.c1);
    const Fp6 sa = fp6_add(a.c0, a.c1), sb = fp6_add(b.c0, b.c1);
    fp6_mul(m, sa, sb);
    r.c1 = fp6_sub(fp6_sub(m, aa), bb);
    r.c0 = fp6_add(aa, fp6_mul_v(bb));
}

// (c0 + c1 w)^2 = (c0 + c1)(c0 + v c1) - c0 c1 - v c0 c1 + 2 c0 c1 w: two Fp6 products
ZG_DEV_CALL void fp12_sqr(Fp12 &r, const Fp12 &a) {
    Fp6 ab, m;
    fp6_mul(ab, a.c0, a.c1);
    const Fp6 s = fp6_add(a.c0, a.c1), t = fp6_add(a.c0, fp6_mul_v(a.c1));
    fp6_mul(m, s, t);
    r.c0 = fp6_sub(fp6_sub(m, ab), fp6_mul_v(ab));
    r.c1 = fp6_add(ab, ab);
}

// 1 / (c0 + c1 w) = (c0 - c1 w) / (c0^2 - v c1^2) (pairing.zig:586-614); inverse(0) -> 0 (null in the reference)
ZG_DEV_CALL void fp12_inv(Fp12 &r, const Fp12 &a) {
    Fp6 s0, s1, ni;
    fp6_mul(s0, a.c0, a.c0);
    fp6_mul(s1, a.c1, a.c1);
    const Fp6 norm = fp6_sub(s0, fp6_mul_v(s1));
    fp6_inv(ni, norm);
    const Fp6 n1 = fp6_neg(a.c1);
    fp6_mul(r.c0, a.c0, ni);
    fp6_mul(r.c1, n1, ni);
}

// a^(p^n), n = 1, 2, 3 (frobenius / frobenius2 / frobenius3): the coefficient of w^k, k = 2 i + j for c_j.c_i, is conjugated n times
// and multiplied by xi^(k (p^n - 1) / 6) (pairing_consts.hip.h, derived by tools/gen_pairing_consts.py)
ZG_DEV Fp2 pair_gamma(int n, int k) {
    Fp2 g;
#pragma unroll
    for (int i = 0; i < 8; i++) { g.c0.l[i] = PAIR_GAMMA[n - 1][k - 1][i]; g.c1.l[i] = PAIR_GAMMA[n - 1][k - 1][8 + i]; }
    return g;
}
ZG_DEV_CALL void fp12_frobenius(Fp12 &r, const Fp12 &a, int n) {
    const Fp2 *src[6] = {&a.c0.c0, &a.c1.c0, &a.c0.c1, &a.c1.c1, &a.c0.c2, &a.c1.c2};  // by the power of w
    Fp2 *dst[6] = {&r.c0.c0, &r.c1.c0, &r.c0.c1, &r.c1.c1, &r.c0.c2, &r.c1.c2};
    const bool odd = n & 1;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        Fp2 c = *src[k];
        if (odd) c = fp2_conj(c);
        if (k) c = fe_mul(c, pair_gamma(n, k));
        *dst[k] = c;
    }
}

// Fp6 times the sparse (c0, c1, 0): five Fp2 products (fp6MulBy01, pairing.zig:1107-1133)
ZG_DEV_CALL void fp6_mul_by_01(Fp6 &r, const Fp6 &f, Fp2 c0, Fp2 c1) {
    const Fp2 aa = fe_mul(f.c0, c0), bb = fe_mul(f.c1, c1);
    const Fp2 t1 = fe_add(fp2_mul_xi(fe_sub(fe_mul(c1, fe_add(f.c1, f.c2)), bb)), aa);
    const Fp2 t3 = fe_add(fe_sub(fe_mul(c0, fe_add(f.c0, f.c2)), aa), bb);
    const Fp2 t2 = fe_sub(fe_sub(fe_mul(fe_add(c0, c1), fe_add(f.c0, f.c1)), aa), bb);
    r.c0 = t1;
    r.c1 = t2;
    r.c2 = t3;
}

// f times the sparse c0 + c3 w + c4 v w — a line of the D-type twist — in 13 Fp2 products (fp12MulBy034, pairing.zig:1156-1189)
ZG_DEV_CALL void fp12_mul_by_034(Fp12 &f, const Fp2 &c0, const Fp2 &c3, const Fp2 &c4) {
    const Fp6 a = Fp6{fe_mul(f.c0.c0, c0), fe_mul(f.c0.c1, c0), fe_mul(f.c0.c2, c0)};
    Fp6 b, e;
    fp6_mul_by_01(b, f.c1, c3, c4);
    const Fp6 fs = fp6_add(f.c0, f.c1);
    fp6_mul_by_01(e, fs, fe_add(c0, c3), c4);
    f.c1 = fp6_sub(fp6_sub(e, a), b);
    f.c0 = fp6_add(a, fp6_mul_v(b));
}

// f^x, x = 4965661367192848881 (expByX, pairing.zig:1786-1800): square-and-multiply from the top bit, plain squarings — the input
// need not be cyclotomic
ZG_DEV_CALL void fp12_exp_by_x(Fp12 &r, const Fp12 &f) {
    const Fp12 base = f;
    Fp12 acc = f;  // bit 62, the top bit of x
#pragma unroll 1
    for (int bit = 61; bit >= 0; bit--) {
        fp12_sqr(acc, acc);
        if ((PAIR_BN_X >> bit) & 1ull) fp12_mul(acc, acc, base);
    }
    r = acc;
}

}  // namespace zg
