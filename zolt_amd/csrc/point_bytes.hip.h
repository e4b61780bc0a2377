// point_bytes.hip.h — curve points out of the byte formats of key, proof and preprocessing files, one lane per record (device side; the
// lane functions also compile for the host: tests/cpp/point_bytes_host.cpp).
//
// The encodings (include/zolt_gpu.h, "Points from bytes"; record sizes G1 / G2):
//   ZG_POINT_BYTES_BE              64 / 128   parseG1Uncompressed / parseG2Uncompressed (src/poly/commitment/srs.zig:65-99, :165-203):
//                                             G1 x, y big-endian; G2 x.c1, x.c0, y.c1, y.c0 big-endian; identity = every byte zero
//   ZG_POINT_BYTES_LE              64 / 128   parseG1LE / parseG2LE (srs.zig:616-712): G1 x, y little-endian; G2 x.c0, x.c1, y.c0, y.c1
//                                             little-endian; identity = every byte zero
//   ZG_POINT_BYTES_ARK             64 / 128   the Jolt Dory SRS records (src/poly/commitment/dory.zig:828-924): as LE with the two top bits of
//                                             the record's last byte cleared first; identity = every byte zero after that
//   ZG_POINT_BYTES_ARK_COMPRESSED  32 / 64    decompressG1 / decompressG2 (dory.zig:81-120, :214-261): x little-endian (G2 x.c0, x.c1),
//                                             flag = last byte & 0xC0: 0x40 exactly = identity, the stored sign is positive iff flag == 0,
//                                             x is taken with the two bits cleared; y = sqrt(x^3 + b) with the sign the flag names
// A coordinate is reduced and brought to Montgomery form as ZG_OP_TO_MONT does it (one product by R^2: fromBytesBE's reduction,
// src/field/mod.zig:171-184), so a coordinate >= p gives the words zg_field_op gives. With ZG_POINT_BYTES_CHECK a non-identity
// uncompressed point that is not on its curve is a bad record (the reference checks G1 in BE and LE, never G2, never ARK: the mirrors
// pass the flag accordingly). Compressed records are on the curve by construction; one whose x has no y is a bad record.
//
// Two deviations from the reference:
//   - its ARK G2 parser (dory.zig:892-924) has no identity rule: an all-zero record becomes the point (0, 0), which is on no curve.
//     Here it is the identity, written as G2Point.identity().
//   - parseG1Compressed (srs.zig:102-162) is left out. Its 48-byte layout is another curve's; the top limb of its sqrtFp exponent
//     (:227-232) is p's own top limb, so the exponent is not (p + 1) / 4 and the function refuses almost every input; nothing calls it.
// Subgroup membership of G2 is not checked: the reference has no such check.
//
// Square roots: p = 3 mod 4 (dory.zig:124-158), so sqrt(a) = a^((p+1)/4) where it exists — a 4-bit window over the fixed exponent,
// 252 squarings and 76 products, accepted only if its square is a. In Fp2 = Fp[u]/(u^2 + 1) for a = a0 + a1 u:
//   alpha = sqrt(a0^2 + a1^2) (no root: a is no square), delta = (a0 + alpha) / 2 (delta = a0 for a1 = 0, dory.zig:273-286),
//   c = delta^((p+1)/4): c^2 = delta gives (c, a1 / 2c), otherwise c^2 = -delta and the root is (a1 / 2c, c)
// — two exponentiations and one inversion, no second attempt that only half the lanes would need. The reference's fp2Sqrt (:265-316)
// may return the other root; the y that leaves here is normalised by the sign flag, so it is the same point. fp2Sqrt also returns null
// for the squares whose (a0 + alpha) / 2 and (alpha - a0) / 2 are both non-squares (they are squares together or not at all) — half of
// the G2 points of the reference's own captured proof; here every square has its root.
#pragma once
#include "../../include/zolt_gpu.h"
#include "g1.hip.h"
#include "g2.hip.h"

namespace zg {

// what a lane reports for its record
static constexpr int PB_OK = 0, PB_NOT_ON_CURVE = 1, PB_NO_ROOT = 2;

struct PbG1 {
    using F = Fp;
    static constexpr int BLOCK = 256, WORDS = 8, COORDS = 2;  // 64-bit words and Fp coordinates of an affine point
    ZG_DEV static bool on_curve(const Affine &p) { return g1_is_on_curve(p); }
};
struct PbG2 {
    using F = Fp2;
    static constexpr int BLOCK = 64, WORDS = 16, COORDS = 4;
    ZG_DEV static bool on_curve(const G2Affine &p) { return g2_is_on_curve(p); }
};

constexpr size_t pb_record_bytes(int coords, uint32_t encoding) { return (size_t)coords * (encoding == ZG_POINT_BYTES_ARK_COMPRESSED ? 16 : 32); }

ZG_DEV u32 pb_bswap(u32 v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// coordinate k of a point (x.c0, x.c1, y.c0, y.c1 order; x, y for G1) out of the record's words: the raw 256-bit integer, then TO_MONT
template <int COORDS>
ZG_DEV Fp pb_coord(const u32 *w, int k, bool big_endian) {
    Fp raw;
    if (big_endian) {
        const int at = COORDS == 4 ? (k ^ 1) : k;  // G2 stores c1 before c0
#pragma unroll
        for (int i = 0; i < 8; i++) raw.l[i] = pb_bswap(w[8 * at + 7 - i]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) raw.l[i] = w[8 * k + i];
    }
    return fe_to_mont(raw);
}

ZG_DEV AffineT<Fp> pb_point(const Fp *c, const Affine *) { return Affine{c[0], c[1]}; }
ZG_DEV AffineT<Fp2> pb_point(const Fp *c, const G2Affine *) { return G2Affine{Fp2{c[0], c[1]}, Fp2{c[2], c[3]}}; }

// one uncompressed record (16-byte aligned) -> point and identity flag
template <class G>
ZG_DEV int pb_decode(const uint4 *rec, uint32_t encoding, bool check, AffineT<typename G::F> &out, bool &inf) {
    constexpr int NW = G::COORDS * 8;
    u32 w[NW];
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
        const uint4 v = rec[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    if (encoding == ZG_POINT_BYTES_ARK) w[NW - 1] &= 0x3fffffffu;  // the flag bits of the record's last byte
    u32 any = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) any |= w[i];
    inf = any == 0;
    if (inf) {
        out = AffineT<typename G::F>::identity();
        return PB_OK;
    }
    Fp c[G::COORDS];
#pragma unroll
    for (int k = 0; k < G::COORDS; k++) c[k] = pb_coord<G::COORDS>(w, k, encoding == ZG_POINT_BYTES_BE);
    out = pb_point(c, (const AffineT<typename G::F> *)nullptr);
    return (check && !G::on_curve(out)) ? PB_NOT_ON_CURVE : PB_OK;
}

// a^((p+1)/4): the exponent's limbs are dory.zig:131-136's, its top nibble is zero
ZG_DEV_CALL Fp pb_fp_pow_sqrt(Fp a) {
    const u64 E0 = 0x4f082305b61f3f52ull, E1 = 0x65e05aa45a1c72a3ull, E2 = 0x6e14116da0605617ull, E3 = 0x0c19139cb84c680aull;
    Fp tbl[16];  // tbl[j] = a^j, 512 bytes of private segment (profiles/point_bytes_resources.txt); one entry is read per window
    tbl[0] = Fp::one();
    tbl[1] = a;
#pragma unroll
    for (int j = 2; j < 16; j++) tbl[j] = (j & 1) ? fe_mul(tbl[j - 1], a) : fe_sqr(tbl[j / 2]);
    Fp acc = tbl[(E3 >> 56) & 15];  // nibble 62
#pragma unroll 1
    for (int k = 61; k >= 0; k--) {
        acc = fe_sqr(fe_sqr(fe_sqr(fe_sqr(acc))));
        const u64 e = k >= 48 ? E3 : k >= 32 ? E2 : k >= 16 ? E1 : E0;
        const u32 nib = (u32)(e >> (4 * (k & 15))) & 15u;
        if (nib) {
            Fp t = tbl[1];
#pragma unroll
            for (u32 j = 2; j < 16; j++)
                if (nib == j) t = tbl[j];
            acc = fe_mul(acc, t);
        }
    }
    return acc;
}

// tonelliShanks (dory.zig:124-158): sqrt(0) = 0; false when a is no square
ZG_DEV bool pb_fp_sqrt(const Fp &a, Fp &r) {
    r = pb_fp_pow_sqrt(a);
    return fe_sqr(r).eq(a);
}

ZG_DEV bool pb_fp2_sqrt(const Fp2 &a, Fp2 &r) {
    r = Fp2::zero();
    if (a.is_zero()) return true;
    Fp alpha;
    if (!pb_fp_sqrt(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)), alpha)) return false;
    Fp delta = a.c0;
    if (!a.c1.is_zero()) {
        delta = fe_add(a.c0, alpha);
        limbs_half_mod<FpParams>(delta.l);  // x / 2 mod p is linear: it halves the Montgomery residue's value
    }
    const Fp c = pb_fp_pow_sqrt(delta);
    const Fp t = fe_mul(a.c1, fe_inv_safegcd(fe_dbl(c)));
    r = fe_sqr(c).eq(delta) ? Fp2{c, t} : Fp2{t, c};
    return fe_sqr(r).eq(a);
}

// yIsPositive / fp2IsPositive (dory.zig:162-175, :320-344): y <= -y as canonical integers; Fp2 compares c1 first, then c0
ZG_DEV bool pb_is_positive(const Fp &y) {
    const Fp ys = fe_from_mont(y), ns = fe_from_mont(fe_neg(y));
    return limbs_ge<FpParams>(ns.l, ys.l);
}
ZG_DEV bool pb_is_positive(const Fp2 &y) { return y.c1.is_zero() ? pb_is_positive(y.c0) : pb_is_positive(y.c1); }

ZG_DEV bool pb_sqrt(const Fp &a, Fp &r) { return pb_fp_sqrt(a, r); }
ZG_DEV bool pb_sqrt(const Fp2 &a, Fp2 &r) { return pb_fp2_sqrt(a, r); }
ZG_DEV Fp pb_curve_b(const Fp *) { return fe_add(fe_dbl(Fp::one()), Fp::one()); }
ZG_DEV Fp2 pb_curve_b(const Fp2 *) { return g2_b_twist(); }
ZG_DEV Fp pb_x(const Fp *c, const Fp *) { return c[0]; }
ZG_DEV Fp2 pb_x(const Fp *c, const Fp2 *) { return Fp2{c[0], c[1]}; }

// one compressed record (16-byte aligned) -> point and identity flag
template <class G>
ZG_DEV int pb_decompress(const uint4 *rec, AffineT<typename G::F> &out, bool &inf) {
    using F = typename G::F;
    constexpr int NW = G::COORDS * 4, NX = G::COORDS / 2;
    u32 w[NW];
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
        const uint4 v = rec[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    const u32 flag = w[NW - 1] >> 30;  // bit 7 and bit 6 of the last byte: 1 = identity, 0 = y is positive
    w[NW - 1] &= 0x3fffffffu;
    inf = flag == 1u;
    out = AffineT<F>::identity();
    if (inf) return PB_OK;
    Fp c[NX];
#pragma unroll
    for (int k = 0; k < NX; k++) c[k] = pb_coord<NX>(w, k, false);
    const F x = pb_x(c, (const F *)nullptr);
    F y;
    if (!pb_sqrt(fe_add(fe_mul(fe_sqr(x), x), pb_curve_b((const F *)nullptr)), y)) return PB_NO_ROOT;
    if ((flag == 0u) != pb_is_positive(y)) y = fe_neg(y);
    out.x = x;
    out.y = y;
    return PB_OK;
}

}  // namespace zg
