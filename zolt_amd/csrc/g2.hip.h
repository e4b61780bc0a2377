// g2.hip.h — BN254 G2 (the twist y^2 = x^3 + 3/(9+u) over Fp2) for gfx950 (device side): the group law of xyzz.hip.h over Fp2.
//
// The reference's G2Point (src/field/pairing.zig:749-925) is affine: add / double are the chord-and-tangent formulas with one Fp2
// inversion each, scalarMul is double-and-add over them. Affine coordinates of a group element are unique canonical values, so any
// complete group law gives the same bytes: the device accumulates in extended-Jacobian "XYZZ" coordinates over Fp2 and converts to
// affine once per output.
//
// Outcomes the reference distinguishes and the law keeps (pairing.zig:839-875): an identity operand passes the other
// through; x1 == x2 with y1 == -y2 gives the identity; x1 == x2 otherwise doubles; doubling a point with y == 0 gives the identity.
#pragma once
#include "fp2.hip.h"
#include "xyzz.hip.h"

namespace zg {

using G2Affine = AffineT<Fp2>;  // 128 B in HBM: x.c0, x.c1, y.c0, y.c1
using G2XYZZ = XyzzT<Fp2>;      // 256 B

// G2Point.identity(): x = 0, y = (one, 0) (pairing.zig:754-760) — how an identity is WRITTEN; on input only the flag counts
template <>
ZG_DEV G2Affine G2Affine::identity() { return G2Affine{Fp2::zero(), Fp2::one()}; }

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
    return fe_sqr(p.y).eq(fe_add(fe_mul(fe_sqr(p.x), p.x), g2_b_twist()));
}

}  // namespace zg
