// lazy_selftest.hip.h — one record of zg_selftest_lazy_g1 (include/zolt_gpu_internal.h): the MSM's lazy-limb field forms
// (fp29.hip.h) and group law (g1_29.hip.h, g1_29x4.hip.h) on RAW limbs, so that a test can choose the representative and the limb
// encoding of every operand. The functions called here are the ones msm.hip calls, not restatements of them.
//
// Shared by the device kernel (selftest.hip) and the host harness (tests/cpp/lazy_g1_host.cpp, which compiles the same headers for the
// CPU with ZG_F29_SERIAL and without ZG_LAZY_DEVICE_FORMS: no inline-assembly product forms, no quad ops).
//
// Record in  (ZG_LAZY_IN_WORDS u32):  ten F29 operands s0..s9 as 9 raw limbs each, then one flags word.
// Record out (ZG_LAZY_OUT_WORDS u32): sixteen F29 results r0..r15, then a status word and an aux word. Results not written are zero.
//
//   op      operands                                flags                              results
//   MADD    s0..s3 acc (x, y, zz, zzz), s4 s5 (px, py)  bit 0: neg                     r0..r3 acc, status = exc code, aux = inf
//           bit 3 (MADD and START): the addition with P, R and 4p - Y1 carried (xyzz29_madd_nz_t<true>), the reference form of the
//           un-carried one the kernels run — one binary compares the two
//   START   s4 s5 first point, s6 s7 second point   bit 0: neg of the first, bit 1: of the second   as MADD
//   ADD     s0..s3 a, s4..s7 b                      -                                  r0..r3, aux = the result is the identity
//   DBL     s0..s3 a                                -                                  r0..r3, aux as ADD
//   JDBL    s0..s2 (x, y, z)                        -                                  r0..r2
//   PROD    s0..s5 = A B C D E F                    -                                  compiler forms: r9 = A*B, r10 = C*D, r11 = E*F,
//           r12 = A^2, r13 = C^2, r14 = A*B + C*D; device only (status bit 0 set): r0 r1 = f29_mul_x2(A*B, C*D), r2 r3 r4 =
//           f29_mul_x3(A*B, C*D, E*F), r5 r6 = f29_sqr_x2(A^2, C^2), r7 r8 = f29_mul2_mul(A*B + C*D, E*F)
//   LIN     s0 s1 s2 = a b c                        bit k: run function k (ZG_LAZY_LIN_*)   r[k], f29_to_fp as 8 words of r12;
//           status bit 0 = f29_is_zero_modp(a). Bit 16: the SUB7 / PMSUB_POS / PMSUB_NEG / NEG4 slots run the un-carried forms
//           (f29_sub7_raw, f29_pmsub45_raw, f29_neg4_raw): the same integers, limbs up to 3 * 2^29
//   MADD4 ADD4 DBL4 (device only): the operands of MADD (flags bit 2: the accumulator is the identity; neg is not an input of
//           xyzz29_madd4) / ADD / DBL, one record per QUAD; lane q of the quad writes r[4q..4q+3], status bit q = that lane's inf
#pragma once
#include "g1_29.hip.h"
#ifdef ZG_LAZY_DEVICE_FORMS
#include "g1_29x4.hip.h"
#endif

#define ZG_LAZY_IN_WORDS 91
#define ZG_LAZY_OUT_WORDS 146

namespace zg {

enum LazyOp { LAZY_MADD = 0, LAZY_START = 1, LAZY_ADD = 2, LAZY_DBL = 3, LAZY_JDBL = 4, LAZY_PROD = 5, LAZY_LIN = 6, LAZY_MADD4 = 7, LAZY_ADD4 = 8, LAZY_DBL4 = 9,
              LAZY_NOPS = 10 };
enum LazyLin { LIN_SUB2 = 0, LIN_SUB4 = 1, LIN_SUB7 = 2, LIN_PMSUB_POS = 3, LIN_PMSUB_NEG = 4, LIN_NEG2 = 5, LIN_NEG4 = 6, LIN_X3 = 7, LIN_SUB4_2C = 8,
               LIN_TIMES2 = 9, LIN_TIMES3 = 10, LIN_TIMES4 = 11, LIN_TO_FP = 12, LIN_IS_ZERO = 13 };
constexpr u32 LAZY_MADD_CARRY_ALL = 1u << 3;  // flags of MADD / START
constexpr u32 LAZY_LIN_RAW = 1u << 16;        // flags of LIN

ZG_DEV F29 lazy_get(const u32 *in, int slot) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = in[9 * slot + i];
    return r;
}
ZG_DEV void lazy_put(u32 *out, int slot, const F29 &v) {
#pragma unroll
    for (int i = 0; i < 9; i++) out[9 * slot + i] = v.l[i];
}
ZG_DEV XYZZ29 lazy_get_point(const u32 *in, int slot) {
    XYZZ29 a;
    a.x = lazy_get(in, slot); a.y = lazy_get(in, slot + 1); a.zz = lazy_get(in, slot + 2); a.zzz = lazy_get(in, slot + 3);
    return a;
}
ZG_DEV void lazy_put_point(u32 *out, int slot, const XYZZ29 &a) {
    lazy_put(out, slot, a.x); lazy_put(out, slot + 1, a.y); lazy_put(out, slot + 2, a.zz); lazy_put(out, slot + 3, a.zzz);
}

// the single-lane ops: `out` is the record's own, zeroed by the caller
ZG_DEV void lazy_record(int op, const u32 *in, u32 *out) {
    const u32 flags = in[90];
    u32 status = 0, aux = 0;
    if (op == LAZY_MADD || op == LAZY_START) {
        XYZZ29 acc;
        F29 px, py;
        u32 neg;
        if (op == LAZY_MADD) {
            acc = lazy_get_point(in, 0);
            px = lazy_get(in, 4); py = lazy_get(in, 5);
            neg = (flags & 1u) ? ~0u : 0u;
        } else {
            const F29 sx = lazy_get(in, 4), sy = lazy_get(in, 5);
            xyzz29_start(acc, sx, (flags & 1u) ? f29_neg2(sy) : sy);
            px = lazy_get(in, 6); py = lazy_get(in, 7);
            neg = (flags & 2u) ? ~0u : 0u;
        }
        bool inf = false;
        const u32 exc = (flags & LAZY_MADD_CARRY_ALL) ? xyzz29_madd_nz_t<true>(acc, px, py, neg) : xyzz29_madd_nz(acc, px, py, neg);
        if (exc != 0) xyzz29_madd_except(acc, inf, px, py, neg, exc);
        lazy_put_point(out, 0, acc);
        status = exc;
        aux = inf ? 1u : 0u;
    } else if (op == LAZY_ADD) {
        const XYZZ29 r = xyzz29_add(lazy_get_point(in, 0), lazy_get_point(in, 4));
        lazy_put_point(out, 0, r);
        aux = xyzz29_is_identity(r) ? 1u : 0u;
    } else if (op == LAZY_DBL) {
        const XYZZ29 r = xyzz29_dbl(lazy_get_point(in, 0));
        lazy_put_point(out, 0, r);
        aux = xyzz29_is_identity(r) ? 1u : 0u;
    } else if (op == LAZY_JDBL) {
        Jac29 p;
        p.x = lazy_get(in, 0); p.y = lazy_get(in, 1); p.z = lazy_get(in, 2);
        const Jac29 r = jac29_dbl(p);
        lazy_put(out, 0, r.x); lazy_put(out, 1, r.y); lazy_put(out, 2, r.z);
    } else if (op == LAZY_PROD) {
        const F29 A = lazy_get(in, 0), B = lazy_get(in, 1), C = lazy_get(in, 2), D = lazy_get(in, 3), E = lazy_get(in, 4), F = lazy_get(in, 5);
#ifdef ZG_LAZY_DEVICE_FORMS
        F29 r0, r1, r2, r3, r4, r5, r6, r7, r8;
        f29_mul_x2(r0, A, B, r1, C, D);
        f29_mul_x3(r2, A, B, r3, C, D, r4, E, F);
        f29_sqr_x2(r5, A, r6, C);
        f29_mul2_mul(r7, A, B, C, D, r8, E, F);
        lazy_put(out, 0, r0); lazy_put(out, 1, r1); lazy_put(out, 2, r2); lazy_put(out, 3, r3); lazy_put(out, 4, r4);
        lazy_put(out, 5, r5); lazy_put(out, 6, r6); lazy_put(out, 7, r7); lazy_put(out, 8, r8);
        status = 1u;
#endif
        lazy_put(out, 9, f29_mul(A, B));
        lazy_put(out, 10, f29_mul(C, D));
        lazy_put(out, 11, f29_mul(E, F));
        lazy_put(out, 12, f29_sqr(A));
        lazy_put(out, 13, f29_sqr(C));
        lazy_put(out, 14, f29_mul2(A, B, C, D));
    } else if (op == LAZY_LIN) {
        const F29 a = lazy_get(in, 0), b = lazy_get(in, 1), c = lazy_get(in, 2);
        if (flags >> LIN_SUB2 & 1u) lazy_put(out, LIN_SUB2, f29_sub2(a, b));
        if (flags >> LIN_SUB4 & 1u) lazy_put(out, LIN_SUB4, f29_sub4(a, b));
        const bool raw = (flags & LAZY_LIN_RAW) != 0;
        if (flags >> LIN_SUB7 & 1u) lazy_put(out, LIN_SUB7, raw ? f29_sub7_raw(a, b) : f29_sub7(a, b));
        if (flags >> LIN_PMSUB_POS & 1u) lazy_put(out, LIN_PMSUB_POS, raw ? f29_pmsub45_raw(a, b, 0u) : f29_pmsub45(a, b, 0u));
        if (flags >> LIN_PMSUB_NEG & 1u) lazy_put(out, LIN_PMSUB_NEG, raw ? f29_pmsub45_raw(a, b, ~0u) : f29_pmsub45(a, b, ~0u));
        if (flags >> LIN_NEG2 & 1u) lazy_put(out, LIN_NEG2, f29_neg2(b));
        if (flags >> LIN_NEG4 & 1u) lazy_put(out, LIN_NEG4, raw ? f29_neg4_raw(b) : f29_neg4(b));
        if (flags >> LIN_X3 & 1u) lazy_put(out, LIN_X3, f29_x3(a, b, c));
        if (flags >> LIN_SUB4_2C & 1u) lazy_put(out, LIN_SUB4_2C, f29_sub4_2c(a, c));
        if (flags >> LIN_TIMES2 & 1u) lazy_put(out, LIN_TIMES2, f29_times2(a));
        if (flags >> LIN_TIMES3 & 1u) lazy_put(out, LIN_TIMES3, f29_times3(a));
        if (flags >> LIN_TIMES4 & 1u) lazy_put(out, LIN_TIMES4, f29_times4(a));
        if (flags >> LIN_TO_FP & 1u) {
            const Fp t = f29_to_fp(a);
#pragma unroll
            for (int i = 0; i < 8; i++) out[9 * LIN_TO_FP + i] = t.l[i];
        }
        if (flags >> LIN_IS_ZERO & 1u) status = f29_is_zero_modp(a) ? 1u : 0u;
    }
    out[144] = status;
    out[145] = aux;
}

#ifdef ZG_LAZY_DEVICE_FORMS
// the quad ops: called by the four lanes of a quad with the same record; lane q writes its own copy of the result.
// Words 144 and 145 are lane 0's to write (the caller ors the lanes' inf bits together).
ZG_DEV u32 lazy_record4(int op, const u32 *in, u32 *out, u32 q) {
    const u32 flags = in[90];
    XYZZ29 r;
    bool inf = false;
    if (op == LAZY_MADD4) {
        r = lazy_get_point(in, 0);
        inf = (flags & 4u) != 0;
        xyzz29_madd4(r, inf, lazy_get(in, 4), lazy_get(in, 5), q);
    } else if (op == LAZY_ADD4) {
        r = xyzz29_add4(lazy_get_point(in, 0), lazy_get_point(in, 4), q);
        inf = xyzz29_is_identity(r);
    } else {
        r = xyzz29_dbl4(lazy_get_point(in, 0), q);
        inf = xyzz29_is_identity(r);
    }
    lazy_put_point(out, 4 * (int)q, r);
    return inf ? 1u << q : 0u;
}
#endif

}  // namespace zg
