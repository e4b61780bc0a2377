// xyzz_selftest.hip.h — one record of zg_selftest_xyzz (include/zolt_gpu_internal.h): the canonical XYZZ group law of xyzz.hip.h on RAW
// coordinates, over Fp (G1, group 0) and over Fp2 (G2, group 1), so that a test can choose the representative (l^2 x, l^3 y, l^2, l^3) of
// every XYZZ operand — which no entry point that takes affine points can. The functions called here are the ones small_msm.hip.h, g2.hip,
// points.hip and dory.hip call, not restatements of them.
//
// Shared by the device kernel (selftest.hip) and the host harness (tests/cpp/xyzz_host.cpp, which compiles the same headers for the CPU).
//
// W = F::BYTES / 8 (4: Fp, 8: Fp2) u64 words per coordinate, the ABI's canonical Montgomery form.
// Record in  (8 W + 6 u64): a.x a.y a.zz a.zzz b.x b.y b.zz b.zzz, a scalar (four words, a canonical integer < 2^256), a flags word, a pad.
// Record out (4 W + 2 u64): r.x r.y r.zz r.zzz (words not written are zero), a status word, a pad.
//
//   op          operands                              flags                                   results
//   DBL_AFFINE  a.x a.y                               -                                       r, status = r is the identity
//   DBL         a                                     -                                       r, status as above
//   MADD        a (acc), b.x b.y (P)                  -                                       r, status as above
//   ADD         a, b                                  bit 8: chained, r = (a + b) + b         r, status as above
//   NEG         a                                     -                                       r, status as above
//   TO_AFFINE   a                                     -                                       r.x r.y affine, status = the returned flag
//   SCALAR_MUL  a.x a.y (P), scalar                   bit 0: p_inf                            r, status = r is the identity
//   AXPY        a.x a.y, b.x b.y, scalar              bit 0: a_inf[i], bit 1: b_inf[i]        r.x r.y = out[i], status = out_inf[i] (0xAA when
//               (index 1 of two-element arrays)       bits 4..5: 0 out is its own range,      out_inf is null: the byte is the harness's own),
//                                                     1 out is b, 2 out is a;                 bit 8 set if index 0 of any array changed
//                                                     bit 6: out_inf == nullptr
//   INV         a.x                                   -                                       r.x = fe_inv_safegcd(a.x) (Fp2: through the norm)
#pragma once
#include "g1.hip.h"
#include "g2.hip.h"

namespace zg {

enum XyzzOp { XS_DBL_AFFINE = 0, XS_DBL = 1, XS_MADD = 2, XS_ADD = 3, XS_NEG = 4, XS_TO_AFFINE = 5, XS_SCALAR_MUL = 6, XS_AXPY = 7, XS_INV = 8, XS_NOPS = 9 };
constexpr u64 XS_P_INF = 1, XS_A_INF = 1, XS_B_INF = 2, XS_OUT_IS_B = 1 << 4, XS_OUT_IS_A = 2 << 4, XS_NO_OUT_INF = 1 << 6, XS_CHAINED = 1 << 8;
constexpr u64 XS_TOUCHED = 1 << 8;  // status of AXPY

template <class F>
struct XyzzRec {
    static constexpr int W = F::BYTES / 8, IN_WORDS = 8 * W + 6, OUT_WORDS = 4 * W + 2;
};

ZG_DEV void xs_get(const u64 *w, Fp &f) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f.l[2 * i] = (u32)w[i];
        f.l[2 * i + 1] = (u32)(w[i] >> 32);
    }
}
ZG_DEV void xs_get(const u64 *w, Fp2 &f) {
    xs_get(w, f.c0);
    xs_get(w + 4, f.c1);
}
ZG_DEV void xs_put(u64 *w, const Fp &f) {
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (u64)f.l[2 * i] | ((u64)f.l[2 * i + 1] << 32);
}
ZG_DEV void xs_put(u64 *w, const Fp2 &f) {
    xs_put(w, f.c0);
    xs_put(w + 4, f.c1);
}
template <class F>
ZG_DEV XyzzT<F> xs_get_point(const u64 *in, int slot) {
    constexpr int W = XyzzRec<F>::W;
    XyzzT<F> a;
    xs_get(in + W * slot, a.x); xs_get(in + W * (slot + 1), a.y); xs_get(in + W * (slot + 2), a.zz); xs_get(in + W * (slot + 3), a.zzz);
    return a;
}
template <class F>
ZG_DEV AffineT<F> xs_get_affine(const u64 *in, int slot) {
    constexpr int W = XyzzRec<F>::W;
    AffineT<F> a;
    xs_get(in + W * slot, a.x); xs_get(in + W * (slot + 1), a.y);
    return a;
}
template <class F>
ZG_DEV void xs_put_point(u64 *out, const XyzzT<F> &a) {
    constexpr int W = XyzzRec<F>::W;
    xs_put(out, a.x); xs_put(out + W, a.y); xs_put(out + 2 * W, a.zz); xs_put(out + 3 * W, a.zzz);
}

// `out` is the record's own, zeroed by the caller
template <class F>
ZG_DEV void xyzz_record(int op, const u64 *in, u64 *out) {
    constexpr int W = XyzzRec<F>::W;
    const u64 flags = in[8 * W + 4];
    Fr s;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s.l[2 * i] = (u32)in[8 * W + i];
        s.l[2 * i + 1] = (u32)(in[8 * W + i] >> 32);
    }
    u64 status = 0;
    if (op == XS_TO_AFFINE) {
        AffineT<F> r;
        status = xyzz_to_affine(xs_get_point<F>(in, 0), r) ? 1 : 0;
        xs_put(out, r.x); xs_put(out + W, r.y);
    } else if (op == XS_AXPY) {
        // index 1 of two-element arrays; index 0 holds a pattern that must come back unchanged
        constexpr int AW = 2 * W;
        alignas(16) u64 av[2 * AW], bv[2 * AW], ov[2 * AW];
        uint8_t ainf[2], binf[2], oinf[2];
        for (int k = 0; k < AW; k++) {
            av[k] = 0xa0a0a0a0a0a0a0a0ull + k; bv[k] = 0xb0b0b0b0b0b0b0b0ull + k; ov[k] = 0xc0c0c0c0c0c0c0c0ull + k;
            av[AW + k] = in[k];
            bv[AW + k] = in[4 * W + k];
            ov[AW + k] = 0;
        }
        ainf[0] = 1; binf[0] = 1; oinf[0] = 0x55;
        ainf[1] = (flags & XS_A_INF) ? 1 : 0;
        binf[1] = (flags & XS_B_INF) ? 1 : 0;
        oinf[1] = 0xAA;
        const u64 alias = flags & (3 << 4);
        u64 *o = alias == XS_OUT_IS_B ? bv : alias == XS_OUT_IS_A ? av : ov;
        xyzz_axpy_at<F>(av, ainf, bv, binf, s, 1, o, (flags & XS_NO_OUT_INF) ? nullptr : oinf);
        for (int k = 0; k < AW; k++) out[k] = o[AW + k];
        status = oinf[1];
        bool touched = ainf[0] != 1 || binf[0] != 1 || oinf[0] != 0x55;
        for (int k = 0; k < AW; k++)
            touched = touched || av[k] != 0xa0a0a0a0a0a0a0a0ull + k || bv[k] != 0xb0b0b0b0b0b0b0b0ull + k || ov[k] != 0xc0c0c0c0c0c0c0c0ull + k;
        if (touched) status |= XS_TOUCHED;
    } else if (op == XS_INV) {
        F a;
        xs_get(in, a);
        xs_put(out, fe_inv_safegcd(a));
    } else {
        XyzzT<F> r = XyzzT<F>::identity();
        if (op == XS_DBL_AFFINE) r = xyzz_dbl_affine(xs_get_affine<F>(in, 0));
        else if (op == XS_DBL) r = xyzz_dbl(xs_get_point<F>(in, 0));
        else if (op == XS_MADD) r = xyzz_madd(xs_get_point<F>(in, 0), xs_get_affine<F>(in, 4));
        else if (op == XS_ADD) {
            const XyzzT<F> b = xs_get_point<F>(in, 4);
            r = xyzz_add(xs_get_point<F>(in, 0), b);
            if (flags & XS_CHAINED) r = xyzz_add(r, b);
        } else if (op == XS_NEG) r = xyzz_neg(xs_get_point<F>(in, 0));
        else if (op == XS_SCALAR_MUL) r = xyzz_scalar_mul(xs_get_affine<F>(in, 0), (flags & XS_P_INF) != 0, s);
        xs_put_point(out, r);
        status = r.is_identity() ? 1 : 0;
    }
    out[4 * W] = status;
}

}  // namespace zg
