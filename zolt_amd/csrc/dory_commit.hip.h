// dory_commit.hip.h — what a lane of the Dory commitment kernels computes (dory_commit.hip), free of launch geometry so that the same
// text compiles for the host (tests/cpp/dory_commit_host.cpp): the digit decode, the key's digit table, a lane's share of a row sum,
// the tree step over the lanes of a row, and the Horner combine of a 64-bit polynomial's eight byte sums.
//
// The key holds T[c][d] = d * g1_vec[c], d = 1..255, as affine rows in the packed lazy form msm_accumulate gathers (64 bytes: x, y as
// 256-bit words of Montgomery-2^261 values, fp29.hip.h); row (c, d) sits at 64 * (255 c + d - 1). A polynomial whose entries are
// digits < 256 then has the row commitment sum_c T[c][digit(c)] — mixed additions only, no buckets, no sort. The sum is COMPLETE:
// generators may be related (a degenerate key, or d1 g = d2 g' by construction), so a lane's partial sum can equal the next table
// entry or its negative; xyzz29_madd_nz reports that case exactly and xyzz29_madd_except finishes it, and the tree is xyzz29_add.
#pragma once
#include "g1_29.hip.h"

namespace zg {

static constexpr uint32_t DC_DIGITS = 255;  // table rows per column

// A virtual polynomial: one digit of at most 8 bits of a column of 64- or 128-bit integers, with an optional sign byte per entry.
// ZG_DORY_POLY_CHUNK* is one of them, ZG_DORY_POLY_U64 eight (shift = 8 w).
struct DcVirt {
    const uint64_t *data;  // words u64 per entry, little-endian
    const uint8_t *aux;    // 1 = the entry is negated; may be null
    uint64_t len;          // entries that are read: 2^num_vars (1 for a one-entry polynomial)
    uint32_t words;        // 1 or 2
    uint32_t shift, mask;  // digit = (entry >> shift) & mask, mask <= 255, shift + bits <= 64 * words
    uint32_t sigma;        // 2^sigma columns
    uint32_t rows;         // 2^nu
    uint32_t lanes_log2;   // lanes that share a row (a power of two <= 64)
    uint32_t first_wave;   // the first wave of this polynomial in the launch
    uint32_t out;          // index of row 0's sum in the array of sums
};

// (entry i >> shift) & mask; a field of a 128-bit entry may straddle its two words
ZG_DEV u32 dc_digit(const uint64_t *data, uint32_t words, uint64_t i, uint32_t shift, uint32_t mask) {
    if (words == 1) return (u32)(data[i] >> shift) & mask;
    const uint64_t lo = data[2 * i], hi = data[2 * i + 1];
    const uint64_t v = shift >= 64 ? hi >> (shift - 64) : shift ? (lo >> shift) | (hi << (64 - shift)) : lo;
    return (u32)v & mask;
}

ZG_DEV F29 dc_one29() {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = Fp29::ONE[i];
    return r;
}

// F29 values in scratch: 48-byte slots, three 16-byte words (limbs 0..8, three unused)
ZG_DEV void dc_f29_store(void *p, const F29 &v) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    q[2] = make_uint4(v.l[8], 0u, 0u, 0u);
}
ZG_DEV F29 dc_f29_load(const void *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 a = q[0], b = q[1], c = q[2];
    F29 r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    r.l[8] = c.x;
    return r;
}

// One column of the table: rows d = 1..255 of g at col (64 bytes apart). 254 mixed additions of the one point (d = 2 is the doubling,
// through the exceptional finish), every multiple kept in XYZZ with the running product of the ZZZ before it, then ONE inversion and a
// backward pass to affine: 1/ZZZ_d = t * prefix_d, 1/Z = ZZ / ZZZ, x = X / Z^2, y = Y / ZZZ. rec / pref: this lane's 255 records of 144 /
// 48 bytes, rec_stride / pref_stride bytes apart. An identity generator leaves zero rows (never gathered: the row sum skips the column).
// d g is never the identity for d <= 255: the group has odd prime order.
ZG_DEV void dc_table_column(const Affine &g, bool g_inf, char *col, char *rec, size_t rec_stride, char *pref, size_t pref_stride) {
    if (g_inf) {
        F29 z;
#pragma unroll
        for (int i = 0; i < 9; i++) z.l[i] = 0;
        for (uint32_t d = 0; d < DC_DIGITS; d++) {
            f29_store_packed(col + 64 * (size_t)d, z);
            f29_store_packed(col + 64 * (size_t)d + 32, z);
        }
        return;
    }
    const F29 gx = f29_from_fp(g.x), gy = f29_from_fp(g.y);
    XYZZ29 acc;
    bool inf = true;
    F29 run = dc_one29();
    for (uint32_t d = 0; d < DC_DIGITS; d++) {
        xyzz29_madd(acc, inf, gx, gy);
        xyzz29_store(rec + rec_stride * d, acc);
        dc_f29_store(pref + pref_stride * d, run);
        run = f29_mul(run, acc.zzz);
    }
    F29 t = f29_from_fp(fe_inv_safegcd(f29_to_fp(run)));  // 1 / (ZZZ_1 ... ZZZ_255)
    for (uint32_t d = DC_DIGITS; d-- > 0;) {
        const XYZZ29 r = xyzz29_load(rec + rec_stride * d);
        const F29 izzz = f29_mul(t, dc_f29_load(pref + pref_stride * d));
        t = f29_mul(t, r.zzz);
        const F29 iz = f29_mul(izzz, r.zz);
        f29_store_packed(col + 64 * (size_t)d, f29_mul(r.x, f29_sqr(iz)));
        f29_store_packed(col + 64 * (size_t)d + 32, f29_mul(r.y, izzz));
    }
}

// table row (c, d), d = 1..255, as the lazy coordinates of d * g1_vec[c]
ZG_DEV void dc_row(const char *table, uint32_t c, u32 d, F29 &px, F29 &py) {
    const uint4 *q = reinterpret_cast<const uint4 *>(table + 64 * ((size_t)c * DC_DIGITS + d - 1));
    const uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    const u32 x[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const u32 y[8] = {w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
    px = f29_unpack(x);
    py = f29_unpack(y);
}

// A lane's share of row `row` of v: sum of +-T[c][digit(row, c)] over the columns c = lane, lane + stride, ... of the row that lie inside
// the polynomial, non-zero digits and non-identity generators only. Returns the identity (zz = 0) for an empty share.
ZG_DEV XYZZ29 dc_lane_sum(const char *table, const uint8_t *g1_inf, const DcVirt &v, uint32_t row, uint32_t lane, uint32_t stride) {
    const uint32_t cols = 1u << v.sigma;
    const uint64_t base = (uint64_t)row << v.sigma;
    XYZZ29 acc = xyzz29_identity();  // the accumulator is the identity whenever `inf` says so: nothing is selected at the end
    bool inf = true;
    for (uint32_t c = lane; c < cols && base + c < v.len; c += stride) {
        const u32 d = dc_digit(v.data, v.words, base + c, v.shift, v.mask);
        if (d == 0 || (g1_inf && g1_inf[c])) continue;
        const u32 neg = v.aux && v.aux[base + c] ? ~0u : 0u;
        F29 px, py;
        dc_row(table, c, d, px, py);
        if (inf) {
            xyzz29_start(acc, px, neg ? f29_neg2(py) : py);
            inf = false;
        } else {
            const u32 exc = xyzz29_madd_nz(acc, px, py, neg);
            if (exc) {  // acc was +-T[c][d]: the double, or the identity
                xyzz29_madd_except(acc, inf, px, py, neg, exc);
                if (inf) acc = xyzz29_identity();
            }
        }
    }
    return acc;
}

// R = sum_w 2^(8 w) S_w from the top byte down: 56 doublings and 7 complete additions. sums: the eight records, stride bytes apart.
ZG_DEV XYZZ29 dc_horner(const char *sums, size_t stride) {
    XYZZ29 r = xyzz29_load(sums + 7 * stride);
    for (int w = 6; w >= 0; w--) {
        for (int k = 0; k < 8; k++) r = xyzz29_dbl(r);
        r = xyzz29_add(r, xyzz29_load(sums + (size_t)w * stride));
    }
    return r;
}

// a sum as the 9-word record of zg_msm_g1_batch_dev: canonical affine xy[8] and the flag word; the identity is written x = y = 0
ZG_DEV void dc_store_record(uint64_t *rec, const XYZZ29 &s) {
    Affine a;
    const bool inf = xyzz_to_affine(xyzz29_to_std_val(s), a);
    fe_store(rec, a.x);
    fe_store(rec + 4, a.y);
    rec[8] = inf ? 1 : 0;
}

}  // namespace zg
