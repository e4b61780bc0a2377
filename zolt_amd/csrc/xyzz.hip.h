// xyzz.hip.h — the short-Weierstrass group law with a = 0 in extended-Jacobian "XYZZ" coordinates, over any field (device side).
//
// One text for G1 (F = Fp, g1.hip.h) and for G2 (F = Fp2, g2.hip.h): the formulas never use the curve's b. The field is whatever type
// has the names field.hip.h gives Fp — fe_add, fe_sub, fe_dbl, fe_neg, fe_mul, fe_sqr, fe_inv_safegcd, fe_store, F::load, F::BYTES,
// zero, one, is_zero, eq — found by overload; fp2.hip.h gives them to Fp2 (product, square and inverse out of line).
//
// Coordinates: x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2 (EFD shortw/xyzz): a mixed add is 8M+2S (vs 7M+4S Jacobian) and needs no squaring
// trick, which suits a mul-only ALU. Affine coordinates of a group element are unique canonical field values, so any complete group
// law gives the bytes of the reference's Jacobian (G1, src/msm/mod.zig:145-329) and affine (G2, src/field/pairing.zig:839-919) ones.
//
// Completeness (the part a GPU shortcut must not drop, SURVEY §7 "hard parts"): every add handles acc = inf, P = acc (-> double),
// P = -acc (-> inf) exactly like the reference's addAffine/add edge cases (msm/mod.zig:229-232,258-267,311-320; pairing.zig:839-875);
// doubling a point with y = 0 gives zz = 0 = the identity (msm/mod.zig:122, pairing.zig:863).
#pragma once
#include "field.hip.h"

namespace zg {

template <class F>
struct AffineT {  // 2 * F::BYTES in HBM: x then y (Montgomery). Infinity is carried out of band.
    F x, y;
    // how the group's reference WRITES an identity result (on input only the flag counts): defined next to each group's alias
    ZG_DEV static AffineT identity();
};

template <class F>
struct XyzzT {  // 4 * F::BYTES; identity <=> zz == 0
    F x, y, zz, zzz;

    ZG_DEV static XyzzT identity() {
        XyzzT r;
        r.x = F::zero(); r.y = F::zero(); r.zz = F::zero(); r.zzz = F::zero();
        return r;
    }
    ZG_DEV bool is_identity() const { return zz.is_zero(); }
    ZG_DEV static XyzzT from_affine(const AffineT<F> &p) {
        XyzzT r;
        r.x = p.x; r.y = p.y; r.zz = F::one(); r.zzz = F::one();
        return r;
    }
};

template <class F>
ZG_DEV AffineT<F> affine_load(const void *p) {
    AffineT<F> a;
    a.x = F::load(p);
    a.y = F::load(reinterpret_cast<const char *>(p) + F::BYTES);
    return a;
}
template <class F>
ZG_DEV void affine_store(void *p, const AffineT<F> &a) {
    fe_store(p, a.x);
    fe_store(reinterpret_cast<char *>(p) + F::BYTES, a.y);
}
template <class F>
ZG_DEV XyzzT<F> xyzz_load(const void *p) {
    const char *c = reinterpret_cast<const char *>(p);
    XyzzT<F> r;
    r.x = F::load(c); r.y = F::load(c + F::BYTES);
    r.zz = F::load(c + 2 * F::BYTES); r.zzz = F::load(c + 3 * F::BYTES);
    return r;
}
template <class F>
ZG_DEV void xyzz_store(void *p, const XyzzT<F> &v) {
    char *c = reinterpret_cast<char *>(p);
    fe_store(c, v.x); fe_store(c + F::BYTES, v.y); fe_store(c + 2 * F::BYTES, v.zz); fe_store(c + 3 * F::BYTES, v.zzz);
}

// 2*(x,y) for an affine point (mdbl-2008-s-1). y = 0 (impossible on G1, odd prime order) yields zz = 0 = identity.
template <class F>
ZG_DEV XyzzT<F> xyzz_dbl_affine(const AffineT<F> &p) {
    F U = fe_dbl(p.y);
    F V = fe_sqr(U);
    F W = fe_mul(U, V);
    F S = fe_mul(p.x, V);
    F xx = fe_sqr(p.x);
    F M = fe_add(fe_dbl(xx), xx);
    XyzzT<F> r;
    r.x = fe_sub(fe_sub(fe_sqr(M), S), S);
    r.y = fe_sub(fe_mul(M, fe_sub(S, r.x)), fe_mul(W, p.y));
    r.zz = V;
    r.zzz = W;
    return r;
}

// 2*P (dbl-2008-s-1); identity stays identity (reference: msm/mod.zig:196)
template <class F>
ZG_DEV XyzzT<F> xyzz_dbl(const XyzzT<F> &p) {
    if (p.is_identity()) return p;
    F U = fe_dbl(p.y);
    F V = fe_sqr(U);
    F W = fe_mul(U, V);
    F S = fe_mul(p.x, V);
    F xx = fe_sqr(p.x);
    F M = fe_add(fe_dbl(xx), xx);
    XyzzT<F> r;
    r.x = fe_sub(fe_sub(fe_sqr(M), S), S);
    r.y = fe_sub(fe_mul(M, fe_sub(S, r.x)), fe_mul(W, p.y));
    r.zz = fe_mul(V, p.zz);
    r.zzz = fe_mul(W, p.zzz);
    return r;
}

// acc + P, P affine and not infinity (madd-2008-s) — the MSM inner-loop unit
// (reference: addAffine, msm/mod.zig:229-274).
template <class F>
ZG_DEV XyzzT<F> xyzz_madd(const XyzzT<F> &a, const AffineT<F> &p) {
    if (a.is_identity()) return XyzzT<F>::from_affine(p);
    F U2 = fe_mul(p.x, a.zz);
    F S2 = fe_mul(p.y, a.zzz);
    F Pp = fe_sub(U2, a.x);
    F R = fe_sub(S2, a.y);
    if (Pp.is_zero()) {
        if (R.is_zero()) return xyzz_dbl_affine(p);  // same point
        return XyzzT<F>::identity();                 // opposite points
    }
    F PP = fe_sqr(Pp);
    F PPP = fe_mul(Pp, PP);
    F Q = fe_mul(a.x, PP);
    XyzzT<F> r;
    r.x = fe_sub(fe_sub(fe_sub(fe_sqr(R), PPP), Q), Q);
    r.y = fe_sub(fe_mul(R, fe_sub(Q, r.x)), fe_mul(a.y, PPP));
    r.zz = fe_mul(a.zz, PP);
    r.zzz = fe_mul(a.zzz, PPP);
    return r;
}

// a + b (add-2008-s), complete (reference: add, msm/mod.zig:277-327)
template <class F>
ZG_DEV XyzzT<F> xyzz_add(const XyzzT<F> &a, const XyzzT<F> &b) {
    if (a.is_identity()) return b;
    if (b.is_identity()) return a;
    F U1 = fe_mul(a.x, b.zz);
    F U2 = fe_mul(b.x, a.zz);
    F S1 = fe_mul(a.y, b.zzz);
    F S2 = fe_mul(b.y, a.zzz);
    F Pp = fe_sub(U2, U1);
    F R = fe_sub(S2, S1);
    if (Pp.is_zero()) {
        if (R.is_zero()) return xyzz_dbl(a);
        return XyzzT<F>::identity();
    }
    F PP = fe_sqr(Pp);
    F PPP = fe_mul(Pp, PP);
    F Q = fe_mul(U1, PP);
    XyzzT<F> r;
    r.x = fe_sub(fe_sub(fe_sub(fe_sqr(R), PPP), Q), Q);
    r.y = fe_sub(fe_mul(R, fe_sub(Q, r.x)), fe_mul(S1, PPP));
    r.zz = fe_mul(fe_mul(a.zz, b.zz), PP);
    r.zzz = fe_mul(fe_mul(a.zzz, b.zzz), PPP);
    return r;
}

template <class F>
ZG_DEV XyzzT<F> xyzz_neg(const XyzzT<F> &a) {
    XyzzT<F> r = a;
    r.y = fe_neg(a.y);
    return r;
}

// XYZZ -> affine, one inversion (reference: toAffine, msm/mod.zig:178-189): 1/Z = ZZ/ZZZ, x = X/Z^2, y = Y/ZZZ. Returns the infinity
// flag; the identity is written as the group's reference writes it.
template <class F>
ZG_DEV bool xyzz_to_affine(const XyzzT<F> &p, AffineT<F> &out) {
    if (p.is_identity()) {
        out = AffineT<F>::identity();
        return true;  // infinity
    }
    F izzz = fe_inv_safegcd(p.zzz);
    F iz = fe_mul(izzz, p.zz);
    F izz = fe_sqr(iz);
    out.x = fe_mul(p.x, izz);
    out.y = fe_mul(p.y, izzz);
    return false;
}

// [s] P by double-and-add from the top bit, s a canonical integer (8 x 32-bit words) — the loop of MSM.scalarMul (msm/mod.zig:503-540)
// and G2Point.scalarMul (pairing.zig:880-919). p_inf or s == 0 -> identity. A wave whose lanes share s (the axpy kernels) runs it
// without divergence.
template <class F>
ZG_DEV XyzzT<F> xyzz_scalar_mul(const AffineT<F> &p, bool p_inf, const Fr &s) {
    XyzzT<F> acc = XyzzT<F>::identity();
    if (p_inf) return acc;
    for (int limb = 7; limb >= 0; limb--) {
        u32 wv = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) wv = (k == limb) ? s.l[k] : wv;
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = xyzz_dbl(acc);
            if ((wv >> bit) & 1u) acc = xyzz_madd(acc, p);
        }
    }
    return acc;
}

// out[i] = s * a[i] + b[i], s a canonical integer: scalarMul followed by the group's affine add, one inversion (the body of points.hip's
// axpy_kernel and of dory.hip's in-place updates). A lane reads index i of a and b and then writes index i of out, nothing else, and
// the inversion is the lane's own: out may be b (v[i] += s * g[i]) or a (v[i] = s * v[i] + v[i + n2] with b = v + n2), but never a
// range that another lane reads.
template <class F>
ZG_DEV void xyzz_axpy_at(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const Fr &s, size_t i, uint64_t *out_xy,
                         uint8_t *out_inf) {
    constexpr int WORDS = 2 * F::BYTES / 8;
    XyzzT<F> acc = xyzz_scalar_mul(affine_load<F>(a_xy + WORDS * i), a_inf && a_inf[i], s);
    if (!(b_inf && b_inf[i])) acc = xyzz_madd(acc, affine_load<F>(b_xy + WORDS * i));
    AffineT<F> r;
    const bool isinf = xyzz_to_affine(acc, r);
    affine_store(out_xy + WORDS * i, r);
    if (out_inf) out_inf[i] = isinf ? 1 : 0;
}

}  // namespace zg
