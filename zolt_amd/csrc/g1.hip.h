// g1.hip.h — BN254 G1 (y^2 = x^3 + 3 over Fp) for gfx950 (device side): the group law of xyzz.hip.h over Fp.
//
// The reference accumulates in Jacobian coordinates (src/msm/mod.zig:145-329:
// double = dbl-2009-l, addAffine = madd-2007-bl shape, add = add-2007-bl) and
// only ever exposes the final AFFINE point (toAffine :178-189). Affine coordinates of a
// group element are unique canonical field values, so the XYZZ law gives the same bytes.
#pragma once
#include "xyzz.hip.h"

namespace zg {

using Affine = AffineT<Fp>;  // 64 B in HBM
using XYZZ = XyzzT<Fp>;      // 128 B

// AffinePoint.identity(): x = y = 0 (msm/mod.zig:24-30; toAffine's identity -> {0,0,inf})
template <>
ZG_DEV Affine Affine::identity() {
    Affine r;
    r.x = Fp::zero(); r.y = Fp::zero();
    return r;
}

ZG_DEV Affine affine_load(const void *p) { return affine_load<Fp>(p); }
ZG_DEV XYZZ xyzz_load(const void *p) { return xyzz_load<Fp>(p); }

// AffinePoint.isOnCurve (msm/mod.zig:106-115): y^2 == x^3 + 3
ZG_DEV bool g1_is_on_curve(const Affine &p) {
    Fp three = fe_add(fe_dbl(Fp::one()), Fp::one());
    Fp rhs = fe_add(fe_mul(fe_sqr(p.x), p.x), three);
    return fe_sqr(p.y).eq(rhs);
}

// XYZZ -> the reference's Jacobian record (X, Y, Z) with the same affine image; identity
// is written as (1,1,0) like ProjectivePoint.identity (msm/mod.zig:154-160). Used for the
// per-GPU partial that crosses the RCCL all-gather.
//   Z := ZZZ/ZZ·ZZ^2... we simply take Z = ZZ, X' = X*ZZ, Y' = Y*ZZZ:  X'/Z^2 = X/ZZ, Y'/Z^3 = Y*ZZZ/ZZ^3 = Y/ZZZ.
ZG_DEV void xyzz_to_jacobian(const XYZZ &p, Fp &X, Fp &Y, Fp &Z) {
    if (p.is_identity()) {
        X = Fp::one(); Y = Fp::one(); Z = Fp::zero();
        return;
    }
    X = fe_mul(p.x, p.zz);
    Y = fe_mul(p.y, p.zzz);
    Z = p.zz;
}
// Jacobian (X,Y,Z) -> XYZZ: ZZ = Z^2, ZZZ = Z^3
ZG_DEV XYZZ xyzz_from_jacobian(const Fp &X, const Fp &Y, const Fp &Z) {
    XYZZ r;
    r.x = X; r.y = Y;
    r.zz = fe_sqr(Z);
    r.zzz = fe_mul(r.zz, Z);
    return r;
}

}  // namespace zg
