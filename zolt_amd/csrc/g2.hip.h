// g2.hip.h — BN254 G2 (the twist y^2 = x^3 + 3/(9+u) over Fp2) for gfx950 (device side).
//
// The reference's G2Point (src/field/pairing.zig:749-925) is affine: add / double are the chord-and-tangent formulas with one Fp2
// inversion each, scalarMul is double-and-add over them. Affine coordinates of a group element are unique canonical values, so any
// complete group law gives the same bytes: the device accumulates in extended-Jacobian "XYZZ" coordinates over Fp2 (the formulas of
// g1.hip.h, which never use the curve's b) and converts to affine once per output.
//
// Outcomes the reference distinguishes and every function here keeps (pairing.zig:839-875): an identity operand passes the other
// through; x1 == x2 with y1 == -y2 gives the identity; x1 == x2 otherwise doubles; doubling a point with y == 0 gives the identity.
#pragma once
#include "fp2.hip.h"

namespace zg {

struct G2Affine {  // 128 B in HBM: x.c0, x.c1, y.c0, y.c1 (Montgomery). Infinity is carried out of band.
    Fp2 x, y;
};

struct G2XYZZ {  // 256 B; identity <=> zz == 0
    Fp2 x, y, zz, zzz;

    ZG_DEV static G2XYZZ identity() { return G2XYZZ{Fp2::zero(), Fp2::zero(), Fp2::zero(), Fp2::zero()}; }
    ZG_DEV bool is_identity() const { return zz.is_zero(); }
    ZG_DEV static G2XYZZ from_affine(const G2Affine &p) { return G2XYZZ{p.x, p.y, Fp2::one(), Fp2::one()}; }
};

ZG_DEV G2Affine g2_affine_load(const void *p) {
    return G2Affine{fp2_load(p), fp2_load(reinterpret_cast<const char *>(p) + 64)};
}
ZG_DEV void g2_affine_store(void *p, const G2Affine &a) {
    fp2_store(p, a.x);
    fp2_store(reinterpret_cast<char *>(p) + 64, a.y);
}
ZG_DEV G2XYZZ g2_xyzz_load(const void *p) {
    const char *c = reinterpret_cast<const char *>(p);
    return G2XYZZ{fp2_load(c), fp2_load(c + 64), fp2_load(c + 128), fp2_load(c + 192)};
}
ZG_DEV void g2_xyzz_store(void *p, const G2XYZZ &v) {
    char *c = reinterpret_cast<char *>(p);
    fp2_store(c, v.x); fp2_store(c + 64, v.y); fp2_store(c + 128, v.zz); fp2_store(c + 192, v.zzz);
}
// G2Point.identity(): x = 0, y = (one, 0) (pairing.zig:754-760) — how an identity is WRITTEN; on input only the flag counts
ZG_DEV G2Affine g2_affine_identity() { return G2Affine{Fp2::zero(), Fp2::one()}; }

// the twist's b' = 3 / (9 + u) = (27 - 3u) / 82 (dory.zig getG2BTwist), Montgomery limbs
ZG_DEV Fp2 g2_b_twist() {
    const u32 c0[8] = {0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u};
    const u32 c1[8] = {0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu};
    Fp2 b;
#pragma unroll
    for (int i = 0; i < 8; i++) { b.c0.l[i] = c0[i]; b.c1.l[i] = c1[i]; }
    return b;
}
// y^2 == x^3 + b' (dory.zig computeG2YSquared)
ZG_DEV bool g2_is_on_curve(const G2Affine &p) {
    return fp2_sqr(p.y).eq(fp2_add(fp2_mul(fp2_sqr(p.x), p.x), g2_b_twist()));
}

// 2 * (x, y) for an affine point (mdbl-2008-s-1); y == 0 -> zz = 0 = identity, as G2Point.double (pairing.zig:863)
ZG_DEV G2XYZZ g2_dbl_affine(const G2Affine &p) {
    Fp2 U = fp2_dbl(p.y);
    Fp2 V = fp2_sqr(U);
    Fp2 W = fp2_mul(U, V);
    Fp2 S = fp2_mul(p.x, V);
    Fp2 M = fp2_mul3(fp2_sqr(p.x));
    G2XYZZ r;
    r.x = fp2_sub(fp2_sub(fp2_sqr(M), S), S);
    r.y = fp2_sub(fp2_mul(M, fp2_sub(S, r.x)), fp2_mul(W, p.y));
    r.zz = V;
    r.zzz = W;
    return r;
}

// 2 * P (dbl-2008-s-1); the identity stays the identity, y == 0 gives zz = 0
ZG_DEV G2XYZZ g2_dbl(const G2XYZZ &p) {
    if (p.is_identity()) return p;
    Fp2 U = fp2_dbl(p.y);
    Fp2 V = fp2_sqr(U);
    Fp2 W = fp2_mul(U, V);
    Fp2 S = fp2_mul(p.x, V);
    Fp2 M = fp2_mul3(fp2_sqr(p.x));
    G2XYZZ r;
    r.x = fp2_sub(fp2_sub(fp2_sqr(M), S), S);
    r.y = fp2_sub(fp2_mul(M, fp2_sub(S, r.x)), fp2_mul(W, p.y));
    r.zz = fp2_mul(V, p.zz);
    r.zzz = fp2_mul(W, p.zzz);
    return r;
}

// acc + P, P affine and not the identity (madd-2008-s)
ZG_DEV G2XYZZ g2_madd(const G2XYZZ &a, const G2Affine &p) {
    if (a.is_identity()) return G2XYZZ::from_affine(p);
    Fp2 Pp = fp2_sub(fp2_mul(p.x, a.zz), a.x);
    Fp2 R = fp2_sub(fp2_mul(p.y, a.zzz), a.y);
    if (Pp.is_zero()) {
        if (R.is_zero()) return g2_dbl_affine(p);  // same point
        return G2XYZZ::identity();                  // opposite points
    }
    Fp2 PP = fp2_sqr(Pp);
    Fp2 PPP = fp2_mul(Pp, PP);
    Fp2 Q = fp2_mul(a.x, PP);
    G2XYZZ r;
    r.x = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(R), PPP), Q), Q);
    r.y = fp2_sub(fp2_mul(R, fp2_sub(Q, r.x)), fp2_mul(a.y, PPP));
    r.zz = fp2_mul(a.zz, PP);
    r.zzz = fp2_mul(a.zzz, PPP);
    return r;
}

// a + b (add-2008-s), complete
ZG_DEV G2XYZZ g2_add(const G2XYZZ &a, const G2XYZZ &b) {
    if (a.is_identity()) return b;
    if (b.is_identity()) return a;
    Fp2 U1 = fp2_mul(a.x, b.zz);
    Fp2 S1 = fp2_mul(a.y, b.zzz);
    Fp2 Pp = fp2_sub(fp2_mul(b.x, a.zz), U1);
    Fp2 R = fp2_sub(fp2_mul(b.y, a.zzz), S1);
    if (Pp.is_zero()) {
        if (R.is_zero()) return g2_dbl(a);
        return G2XYZZ::identity();
    }
    Fp2 PP = fp2_sqr(Pp);
    Fp2 PPP = fp2_mul(Pp, PP);
    Fp2 Q = fp2_mul(U1, PP);
    G2XYZZ r;
    r.x = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(R), PPP), Q), Q);
    r.y = fp2_sub(fp2_mul(R, fp2_sub(Q, r.x)), fp2_mul(S1, PPP));
    r.zz = fp2_mul(fp2_mul(a.zz, b.zz), PP);
    r.zzz = fp2_mul(fp2_mul(a.zzz, b.zzz), PPP);
    return r;
}

// XYZZ -> affine, one inversion: 1/Z = ZZ/ZZZ, x = X/Z^2, y = Y/ZZZ. Returns the infinity flag; the identity is written as
// G2Point.identity() writes it.
ZG_DEV bool g2_to_affine(const G2XYZZ &p, G2Affine &out) {
    if (p.is_identity()) {
        out = g2_affine_identity();
        return true;
    }
    Fp2 izzz = fp2_inv(p.zzz);
    Fp2 iz = fp2_mul(izzz, p.zz);
    out.x = fp2_mul(p.x, fp2_sqr(iz));
    out.y = fp2_mul(p.y, izzz);
    return false;
}

// [s] P by double-and-add from the top bit, s a canonical integer (8 x 32-bit words) — G2Point.scalarMul's loop (pairing.zig:880-919)
// in projective form. p_inf or s == 0 -> identity. A wave whose lanes share s (the axpy kernels) runs it without divergence.
ZG_DEV G2XYZZ g2_scalar_mul(const G2Affine &p, bool p_inf, const Fr &s) {
    G2XYZZ acc = G2XYZZ::identity();
    if (p_inf) return acc;
    for (int limb = 7; limb >= 0; limb--) {
        u32 wv = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) wv = (k == limb) ? s.l[k] : wv;
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = g2_dbl(acc);
            if ((wv >> bit) & 1u) acc = g2_madd(acc, p);
        }
    }
    return acc;
}

}  // namespace zg
