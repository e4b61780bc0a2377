// lazy_fr_selftest.hip.h — one record of zg_selftest_lazy_fr (include/zolt_gpu_internal.h): the sumcheck kernels' lazy Fr arithmetic
// (the Fr side of fp29.hip.h) and their lazy 288-bit sums (acc9.hip.h) on RAW limbs, so that a test can choose the representative and
// the limb encoding of every operand and place it where the headers' comments say the edge of a function's operand class is. The
// functions called here are the ones poly.hip, psc.hip, rrw.hip, rwc.hip and ingest.hip call, not restatements of them.
//
// Shared by the device kernel (selftest.hip) and the host harness (tests/cpp/lazy_fr_host.cpp, which compiles the same headers for the
// CPU with ZG_F29_SERIAL). The block reduction (FR_BLOCKSUM: the DPP additions, wave_sum_pair9, block_sum_pair9 of sc_common.hip.h) moves
// data across lanes and exists in selftest.hip only.
//
// Record in  (ZG_LAZY_FR_IN_WORDS u32):  sixteen slots s0..s15 of 9 words, then a flags word (144) and a length word (145).
// Record out (ZG_LAZY_FR_OUT_WORDS u32): sixteen slots r0..r15 of 9 words, then a status word (144) and an aux word (145). Slots not
// written are zero. "F29": nine raw limbs. "Fr": eight 32-bit words of a Montgomery-2^256 element in words 0..7 of the slot.
//
//   op          operands                                      results
//   MUL         s0 s1 = F29 a, b                              r0 = f29t_mul<Fr29>(a, b) raw, r1 = fr29_out(r0)
//   MUL_SHORT5  s0 s1 = F29 a, b (five limbs of b used)       r0 = f29t_mul_short<Fr29, 5>(a, b) raw, r1 = fr29_out(r0)
//   MUL_SHORT3  the same with three limbs                     the same with f29t_mul_short<Fr29, 3>
//   CANON       s0 s1 = Fr x, y; s2 words 0 1 = u64 u (low,   bit k of flags runs function k (enum LazyFrCanon) into r[k]:    
//               high); flags = the functions to run           0 fr_mul29(x, fr29_prescale(y))   1 fr_mul29v(x, y)
//                                                             2 frmul_apply(x, frmul_prepare(y)), aux bit 0 = narrow, r8 = the prepared factor raw
//                                                             3 fr29_in_shift(y) raw   4 fr_from_u64_29(u)   5 fr_from_mont29(x)
//                                                             6 fe_mul(x, y)           7 fr_mul29(x, Fr29::R2PRE)
//   SUM64       s0 .. s[len-1] = F29 values, flags = count    r0 = acc29_reduce of acc29_add(s[j mod len]) for j < count; aux = FR29_ACC_MAX
//   SUM32       s[4 j + t], j < len <= 4, t < 4 = F29 values  ChainAcc4: init, add({s[4 (j mod len) + t]}, e) for j < count, flush, from
//               flags = count                                 e = 0: r0..r3 = e[0..3]; status = cnt before the last flush, aux = FR29_ACC_MAX
//   CARRY       s0 = F29 with limbs up to 2^32 - 1            r0 = f29_carry(s0)
//   ACC9        s0 = Acc9 S (nine words), s1 s2 = Fr v, w,    r0 = acc9_reduce(S), r1 = S after acc9_add(S, v), r2 = after acc9_add_if(S, w, true),
//               s3 = Acc9 T                                   r3 = after acc9_add_if(S, w, false), r4 = after acc9_add_acc(S, T)
//   BLOCKSUM    (device only, its own layout: selftest.hip)
#pragma once
#include "fp29.hip.h"
#include "acc9.hip.h"

#define ZG_LAZY_FR_IN_WORDS 146
#define ZG_LAZY_FR_OUT_WORDS 146
#define ZG_LAZY_FR_PAIR_WORDS 18 /* BLOCKSUM: one thread's (g0, g1) */
#define ZG_LAZY_FR_MAX_COUNT 1024u /* SUM64, SUM32: the longest loop a record may ask for */

namespace zg {

enum LazyFrOp { FR_MUL = 0, FR_MUL_SHORT5 = 1, FR_MUL_SHORT3 = 2, FR_CANON = 3, FR_SUM64 = 4, FR_SUM32 = 5, FR_CARRY = 6, FR_ACC9 = 7, FR_BLOCKSUM = 8,
                FR_NOPS = 9 };
enum LazyFrCanon { CANON_MUL29 = 0, CANON_MUL29V = 1, CANON_FRMUL = 2, CANON_IN_SHIFT = 3, CANON_FROM_U64 = 4, CANON_FROM_MONT = 5, CANON_FE_MUL = 6,
                   CANON_TO_MONT = 7 };

ZG_DEV F29 lazy_fr_get(const u32 *in, int slot) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = in[9 * slot + i];
    return r;
}
ZG_DEV void lazy_fr_put(u32 *out, int slot, const F29 &v) {
#pragma unroll
    for (int i = 0; i < 9; i++) out[9 * slot + i] = v.l[i];
}
ZG_DEV Fr lazy_fr_get_fr(const u32 *in, int slot) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = in[9 * slot + i];
    return r;
}
ZG_DEV void lazy_fr_put_fr(u32 *out, int slot, const Fr &v) {
#pragma unroll
    for (int i = 0; i < 8; i++) out[9 * slot + i] = v.l[i];
}
ZG_DEV Acc9 lazy_fr_get_acc(const u32 *in, int slot) {
    Acc9 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = in[9 * slot + i];
    return r;
}
ZG_DEV void lazy_fr_put_acc(u32 *out, int slot, const Acc9 &v) {
#pragma unroll
    for (int i = 0; i < 9; i++) out[9 * slot + i] = v.l[i];
}

// `out` is the record's own, zeroed by the caller. A length word outside its range, or a count above ZG_LAZY_FR_MAX_COUNT, leaves the
// record zero with status = ~0.
ZG_DEV void lazy_fr_record(int op, const u32 *in, u32 *out) {
    const u32 flags = in[144], len = in[145];
    u32 status = 0, aux = 0;
    if (op == FR_MUL || op == FR_MUL_SHORT5 || op == FR_MUL_SHORT3) {
        const F29 a = lazy_fr_get(in, 0), b = lazy_fr_get(in, 1);
        const F29 t = op == FR_MUL ? f29t_mul<Fr29>(a, b) : op == FR_MUL_SHORT5 ? f29t_mul_short<Fr29, 5>(a, b) : f29t_mul_short<Fr29, 3>(a, b);
        lazy_fr_put(out, 0, t);
        lazy_fr_put_fr(out, 1, fr29_out(t));
    } else if (op == FR_CANON) {
        const Fr x = lazy_fr_get_fr(in, 0), y = lazy_fr_get_fr(in, 1);
        const u64 u = (u64)in[18] | ((u64)in[19] << 32);
        if (flags >> CANON_MUL29 & 1u) lazy_fr_put_fr(out, CANON_MUL29, fr_mul29(x, fr29_prescale(y)));
        if (flags >> CANON_MUL29V & 1u) lazy_fr_put_fr(out, CANON_MUL29V, fr_mul29v(x, y));
        if (flags >> CANON_FRMUL & 1u) {
            const FrMul m = frmul_prepare(y);
            lazy_fr_put_fr(out, CANON_FRMUL, frmul_apply(x, m));
            lazy_fr_put(out, 8, m.p);
            aux = m.narrow ? 1u : 0u;
        }
        if (flags >> CANON_IN_SHIFT & 1u) lazy_fr_put(out, CANON_IN_SHIFT, fr29_in_shift(y));
        if (flags >> CANON_FROM_U64 & 1u) lazy_fr_put_fr(out, CANON_FROM_U64, fr_from_u64_29(u));
        if (flags >> CANON_FROM_MONT & 1u) lazy_fr_put_fr(out, CANON_FROM_MONT, fr_from_mont29(x));
        if (flags >> CANON_FE_MUL & 1u) lazy_fr_put_fr(out, CANON_FE_MUL, fe_mul(x, y));
        if (flags >> CANON_TO_MONT & 1u) {
            F29 r2p;
#pragma unroll
            for (int i = 0; i < 9; i++) r2p.l[i] = Fr29::R2PRE[i];
            lazy_fr_put_fr(out, CANON_TO_MONT, fr_mul29(x, r2p));
        }
    } else if (op == FR_SUM64) {
        if (len < 1 || len > 16 || flags > ZG_LAZY_FR_MAX_COUNT) {
            status = ~0u;
        } else {
            Acc29 a = acc29_zero();
            u32 slot = 0;
            for (u32 j = 0; j < flags; j++) {
                acc29_add(a, lazy_fr_get(in, (int)slot));
                if (++slot == len) slot = 0;
            }
            lazy_fr_put_fr(out, 0, acc29_reduce(a));
            aux = FR29_ACC_MAX;
        }
    } else if (op == FR_SUM32) {
        if (len < 1 || len > 4 || flags > ZG_LAZY_FR_MAX_COUNT) {
            status = ~0u;
        } else {
            Fr e[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
            ChainAcc4 acc;
            acc.init();
            u32 slot = 0;
            for (u32 j = 0; j < flags; j++) {
                F29 w[4];
#pragma unroll
                for (int t = 0; t < 4; t++) w[t] = lazy_fr_get(in, (int)(4 * slot) + t);
                acc.add(w, e);
                if (++slot == len) slot = 0;
            }
            status = acc.cnt;
            acc.flush(e);
#pragma unroll
            for (int t = 0; t < 4; t++) lazy_fr_put_fr(out, t, e[t]);
            aux = FR29_ACC_MAX;
        }
    } else if (op == FR_CARRY) {
        lazy_fr_put(out, 0, f29_carry(lazy_fr_get(in, 0)));
    } else if (op == FR_ACC9) {
        const Acc9 s = lazy_fr_get_acc(in, 0), t = lazy_fr_get_acc(in, 3);
        const Fr v = lazy_fr_get_fr(in, 1), w = lazy_fr_get_fr(in, 2);
        lazy_fr_put_fr(out, 0, acc9_reduce(s));
        Acc9 a = s;
        acc9_add(a, v);
        lazy_fr_put_acc(out, 1, a);
        a = s;
        acc9_add_if(a, w, true);
        lazy_fr_put_acc(out, 2, a);
        a = s;
        acc9_add_if(a, w, false);
        lazy_fr_put_acc(out, 3, a);
        a = s;
        acc9_add_acc(a, t);
        lazy_fr_put_acc(out, 4, a);
    }
    out[144] = status;
    out[145] = aux;
}

}  // namespace zg
