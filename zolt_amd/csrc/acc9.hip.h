// acc9.hip.h — the lazy 288-bit sums of the sumcheck kernels (sc_common.hip.h includes this): the scalar part, without a lane movement,
// so that the host harness of tests/test_lazy_fr_host.py (tests/cpp/lazy_fr_host.cpp) compiles the same code for the CPU.
#pragma once
#include "field.hip.h"

namespace zg {

// ---- lazy sums. A sum of canonical scalars is kept as a plain 288-bit integer (nine 32-bit limbs, no modular reduction: 9
// add-with-carry instructions per term instead of ~45 for fe_add) and reduced to the canonical element ONCE, where the value leaves
// the kernel. Integer addition is exact, so the canonical result is the reference's whatever the order and grouping. Bound: at most
// 2^30 terms (< 2^284) between two reductions — every table this library accepts is shorter.
struct Acc9 {
    u32 l[9];
};
ZG_DEV Acc9 acc9_zero() {
    Acc9 a;
#pragma unroll
    for (int i = 0; i < 9; i++) a.l[i] = 0;
    return a;
}
ZG_DEV void acc9_add(Acc9 &a, const Fr &v) {
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) a.l[i] = __builtin_addc(a.l[i], v.l[i], c, &c);
    a.l[8] += c;
}
ZG_DEV void acc9_add_if(Acc9 &a, const Fr &v, bool take) {  // a += take ? v : 0
    const u32 m = take ? 0xffffffffu : 0u;
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) a.l[i] = __builtin_addc(a.l[i], v.l[i] & m, c, &c);
    a.l[8] += c;
}
ZG_DEV void acc9_add_acc(Acc9 &a, const Acc9 &b) {
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) a.l[i] = __builtin_addc(a.l[i], b.l[i], c, &c);
    a.l[8] += b.l[8] + c;
}
// S mod r for S < 2^284. Quotient estimate from the top 64 bits: q = floor(floor(S / 2^224) * floor(2^64 / d) / 2^64) with
// d = ceil(r / 2^224) never exceeds floor(S / r) and falls short of it by less than 3.8 for S / r < 2^30.4 (relative error of d:
// 1.24e-9), by at most 2 for S / r < 2^20 — two estimate-and-subtract passes leave a value < 3 r, two conditional subtractions
// finish. ~80 instructions, executed by the one or two lanes that hold a total.
ZG_DEV Fr acc9_reduce(const Acc9 &s) {
    constexpr u64 MAGIC = 0x54a474622ull;  // floor(2^64 / 811880051), 811880051 = ceil(r / 2^224)
    u32 x[9];
#pragma unroll
    for (int i = 0; i < 9; i++) x[i] = s.l[i];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const u64 hi = ((u64)x[8] << 32) | x[7];
        const u32 q = (u32)__umul64hi(hi, MAGIC);  // < 2^31 for S < 2^284
        u64 carry = 0;
        u32 borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            carry += (u64)q * FrParams::MOD[i];
            x[i] = __builtin_subc(x[i], (u32)carry, borrow, &borrow);
            carry >>= 32;
        }
        x[8] = x[8] - (u32)carry - borrow;
    }
    Fr v;  // < 3 r < 2^256: x[8] == 0
#pragma unroll
    for (int i = 0; i < 8; i++) v.l[i] = x[i];
    return fe_reduce_once(fe_reduce_once(v));
}

}  // namespace zg
