// fp2.hip.h — Fp2 = Fp[u] / (u^2 + 1) over the BN254 base field, for gfx950 (device side).
//
// The reference's Fp2 (src/field/pairing.zig:182-272) on the canonical 8 x 32-bit Montgomery form of field.hip.h: every component
// of every result is canonical (< p), so a value computed here has the bytes the reference's schoolbook formulas give — the
// element (ac - bd) + (ad + bc) u is unique whatever sequence of Fp operations reaches it. The lazy 9 x 29 form of fp29.hip.h is
// NOT used: its bounds are stated for the G1 formulas only, and G2 work is latency-bound (short vectors), not multiplier-bound.
#pragma once
#include "field.hip.h"

namespace zg {

// The three heavy operations are real functions, not inlined: a G2 kernel holds 50-150 Fp2 products, and with every one expanded to its
// ~900 instructions the translation unit took ten minutes to compile. Arguments and results travel in registers (48 VGPRs a call).
#ifndef ZG_DEV_CALL  // tests/cpp/pairing_host.cpp compiles the tower for the host
#define ZG_DEV_CALL static __device__ __noinline__
#endif

struct Fp2 {
    Fp c0, c1;  // c0 + c1 u
    static constexpr int BYTES = 64;  // in HBM: c0 then c1

    ZG_DEV static Fp2 zero() { return Fp2{Fp::zero(), Fp::zero()}; }
    ZG_DEV static Fp2 one() { return Fp2{Fp::one(), Fp::zero()}; }
    ZG_DEV static Fp2 load(const void *p) { return Fp2{Fp::load(p), Fp::load(reinterpret_cast<const char *>(p) + 32)}; }
    ZG_DEV bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    ZG_DEV bool eq(const Fp2 &b) const { return c0.eq(b.c0) && c1.eq(b.c1); }
};

// Fp2 carries the names field.hip.h gives Fp, as overloads: they are the field interface the group law of xyzz.hip.h is written in.
ZG_DEV void fe_store(void *p, const Fp2 &v) {
    fe_store(p, v.c0);
    fe_store(reinterpret_cast<char *>(p) + 32, v.c1);
}
ZG_DEV Fp2 fe_add(const Fp2 &a, const Fp2 &b) { return Fp2{fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
ZG_DEV Fp2 fe_sub(const Fp2 &a, const Fp2 &b) { return Fp2{fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
ZG_DEV Fp2 fe_neg(const Fp2 &a) { return Fp2{fe_neg(a.c0), fe_neg(a.c1)}; }
ZG_DEV Fp2 fe_dbl(const Fp2 &a) { return Fp2{fe_dbl(a.c0), fe_dbl(a.c1)}; }
ZG_DEV Fp2 fp2_mul3(const Fp2 &a) { return fe_add(fe_dbl(a), a); }  // multiplication by a small constant: additions only

// (a + bu)(c + du) = (ac - bd) + ((a + b)(c + d) - ac - bd) u — three Fp products (pairing.zig:212-223 spends four)
ZG_DEV_CALL Fp2 fe_mul(Fp2 x, Fp2 y) {
    Fp ac = fe_mul(x.c0, y.c0);
    Fp bd = fe_mul(x.c1, y.c1);
    Fp k = fe_mul(fe_add(x.c0, x.c1), fe_add(y.c0, y.c1));
    return Fp2{fe_sub(ac, bd), fe_sub(fe_sub(k, ac), bd)};
}

// (a + bu)^2 = (a + b)(a - b) + 2ab u — two Fp products (pairing.zig:225-237)
ZG_DEV_CALL Fp2 fe_sqr(Fp2 x) {
    Fp t = fe_mul(fe_add(x.c0, x.c1), fe_sub(x.c0, x.c1));
    return Fp2{t, fe_dbl(fe_mul(x.c0, x.c1))};
}

ZG_DEV Fp2 fp2_mul_fp(const Fp2 &x, const Fp &s) { return Fp2{fe_mul(x.c0, s), fe_mul(x.c1, s)}; }

// 1 / (a + bu) = (a - bu) / (a^2 + b^2): ONE Fp inversion, of the norm (pairing.zig:255-263). inverse(0) -> 0 (the reference
// returns null; callers test is_zero first). -1 is not a square mod p, so the norm of a non-zero element is never zero.
ZG_DEV_CALL Fp2 fe_inv_safegcd(Fp2 x) {
    Fp ninv = fe_inv_safegcd(fe_add(fe_sqr(x.c0), fe_sqr(x.c1)));
    return Fp2{fe_mul(x.c0, ninv), fe_mul(fe_neg(x.c1), ninv)};
}

}  // namespace zg
