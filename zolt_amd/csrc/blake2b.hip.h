// blake2b.hip.h — Fiat-Shamir lane functions: Blake2b-256 as a stream over bytes, the operations of the Jolt-compatible transcript
// (src/transcripts/blake2b.zig:25-398) on a state of 32 bytes and a round counter, and the step that ends a round of a batched sumcheck
// (src/zkvm/batched_sumcheck.zig:127-262, 306-430). One lane does all of it: a round is six dependent compressions, and nothing in them
// is wider than the four independent G steps of a half round. Verified on the host only (tests/cpp/blake2b_host.cpp runs them on the
// CPU, tests/cpp/blake2b_device_compile.hip only compiles them for gfx950): no unit of the library includes this header. Like
// field_vec.hip.h and point_bytes.hip.h, the function qualifiers are the only things a host build replaces.
#pragma once
#include "field.hip.h"

#ifndef ZG_DEV_CALL
#define ZG_DEV_CALL static __device__ __noinline__
#endif

namespace zg {

typedef FrParams FsFrP;
typedef Fe<FrParams> FsFr;

// ---- Blake2b-256, unkeyed (RFC 7693). The 128-byte block buffer is the caller's (LDS on the device, the stack on the host): sixteen
// words, filled byte by byte. A full buffer is compressed only when another byte arrives — the last block, full or not, is compressed
// by b2b_final with the finalisation flag (the "last-block rule": a message of exactly 128 bytes is ONE final block).
struct B2b {
    u64 h[8];
    u64 t;     // bytes compressed so far, the buffered ones included at the time of a compression
    u32 fill;  // bytes in m
    u64 *m;    // sixteen words
};
ZG_DEV u64 b2b_iv(int i) {
    switch (i) {
        case 0: return 0x6a09e667f3bcc908ull;
        case 1: return 0xbb67ae8584caa73bull;
        case 2: return 0x3c6ef372fe94f82bull;
        case 3: return 0xa54ff53a5f1d36f1ull;
        case 4: return 0x510e527fade682d1ull;
        case 5: return 0x9b05688c2b3e6c1full;
        case 6: return 0x1f83d9abfb41bd6bull;
        default: return 0x5be0cd19137e2179ull;
    }
}
ZG_DEV u64 b2b_rotr(u64 x, int n) { return (x >> n) | (x << (64 - n)); }
#define ZG_B2B_G(a, b, c, d, x, y) \
    do {                           \
        a = a + b + (x);           \
        d = b2b_rotr(d ^ a, 32);   \
        c = c + d;                 \
        b = b2b_rotr(b ^ c, 24);   \
        a = a + b + (y);           \
        d = b2b_rotr(d ^ a, 16);   \
        c = c + d;                 \
        b = b2b_rotr(b ^ c, 63);   \
    } while (0)
// one round with the message schedule s0..s15 as constants: the words are named, never indexed at run time
#define ZG_B2B_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                                 \
        ZG_B2B_G(v0, v4, v8, v12, m[s0], m[s1]);                                         \
        ZG_B2B_G(v1, v5, v9, v13, m[s2], m[s3]);                                         \
        ZG_B2B_G(v2, v6, v10, v14, m[s4], m[s5]);                                        \
        ZG_B2B_G(v3, v7, v11, v15, m[s6], m[s7]);                                        \
        ZG_B2B_G(v0, v5, v10, v15, m[s8], m[s9]);                                        \
        ZG_B2B_G(v1, v6, v11, v12, m[s10], m[s11]);                                      \
        ZG_B2B_G(v2, v7, v8, v13, m[s12], m[s13]);                                       \
        ZG_B2B_G(v3, v4, v9, v14, m[s14], m[s15]);                                       \
    } while (0)
ZG_DEV_CALL void b2b_compress(u64 *h, const u64 *mw, u64 t, bool last) {
    u64 m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = mw[i];
    u64 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    u64 v8 = b2b_iv(0), v9 = b2b_iv(1), v10 = b2b_iv(2), v11 = b2b_iv(3), v12 = b2b_iv(4) ^ t, v13 = b2b_iv(5);  // t < 2^64: the high word is 0
    u64 v14 = last ? ~b2b_iv(6) : b2b_iv(6), v15 = b2b_iv(7);
    ZG_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    ZG_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    ZG_B2B_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    ZG_B2B_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    ZG_B2B_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    ZG_B2B_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    ZG_B2B_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    ZG_B2B_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    ZG_B2B_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    ZG_B2B_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    ZG_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    ZG_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    h[0] ^= v0 ^ v8;
    h[1] ^= v1 ^ v9;
    h[2] ^= v2 ^ v10;
    h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12;
    h[5] ^= v5 ^ v13;
    h[6] ^= v6 ^ v14;
    h[7] ^= v7 ^ v15;
}
#undef ZG_B2B_ROUND
#undef ZG_B2B_G

ZG_DEV void b2b_init(B2b &b, u64 *m16) {
#pragma unroll
    for (int i = 0; i < 8; i++) b.h[i] = b2b_iv(i);
    b.h[0] ^= 0x01010020ull;  // digest_size 32, no key, fanout 1, depth 1
    b.t = 0;
    b.fill = 0;
    b.m = m16;
    for (int i = 0; i < 16; i++) m16[i] = 0;
}
ZG_DEV void b2b_byte(B2b &b, u32 byte) {
    if (b.fill == 128) {  // more input behind a full block: it was not the last one
        b.t += 128;
        b2b_compress(b.h, b.m, b.t, false);
        for (int i = 0; i < 16; i++) b.m[i] = 0;
        b.fill = 0;
    }
    b.m[b.fill >> 3] |= (u64)(byte & 0xffu) << (8 * (b.fill & 7u));
    b.fill++;
}
ZG_DEV void b2b_zeros(B2b &b, u32 n) {
    for (u32 i = 0; i < n; i++) b2b_byte(b, 0);
}
ZG_DEV void b2b_bytes(B2b &b, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) b2b_byte(b, p[i]);
}
ZG_DEV void b2b_be32(B2b &b, u32 x) {
    for (int i = 3; i >= 0; i--) b2b_byte(b, x >> (8 * i));
}
ZG_DEV void b2b_be64(B2b &b, u64 x) {
    for (int i = 7; i >= 0; i--) b2b_byte(b, (u32)(x >> (8 * i)));
}
// the digest as four little-endian words (word i = digest bytes 8 i .. 8 i + 7)
ZG_DEV void b2b_final(B2b &b, u64 out[4]) {
    b.t += b.fill;
    b2b_compress(b.h, b.m, b.t, true);  // the buffer's tail is zero: it is cleared after every compression
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = b.h[i];
}

// ---- the transcript. Its state in memory: four words = the 32 state bytes (byte j of the state is byte j % 8 of word j / 8), then
// the round counter in the low half of word 4. FS_STATE_WORDS words in HBM (or anywhere).
constexpr int FS_STATE_WORDS = 5;
struct FsT {
    u64 s[4];
    u32 n_rounds;
    u64 *m;  // the block buffer every hash of this transcript uses
};
ZG_DEV FsT fs_load(const u64 *st, u64 *m16) {
    FsT t;
    for (int i = 0; i < 4; i++) t.s[i] = st[i];
    t.n_rounds = (u32)st[4];
    t.m = m16;
    return t;
}
ZG_DEV void fs_store(const FsT &t, u64 *st) {
    for (int i = 0; i < 4; i++) st[i] = t.s[i];
    st[4] = t.n_rounds;
}
ZG_DEV void b2b_words_le(B2b &b, const u64 *w, int n) {  // n words as their bytes in memory order
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 8; j++) b2b_byte(b, (u32)(w[i] >> (8 * j)));
}
// hasher() (:76-87): state || 0^28 || n_rounds_be32, the payload follows; fs_end (:90-93): the digest is the new state
ZG_DEV B2b fs_begin(const FsT &t) {
    B2b b;
    b2b_init(b, t.m);
    b2b_words_le(b, t.s, 4);
    b2b_zeros(b, 28);
    b2b_be32(b, t.n_rounds);
    return b;
}
ZG_DEV void fs_end(FsT &t, B2b &b) {
    b2b_final(b, t.s);
    t.n_rounds += 1;
}
// init (:39-69): the label, zero-padded to 32 bytes, hashed; a longer label is cut to 32 (the reference refuses it)
ZG_DEV void fs_init(FsT &t, const uint8_t *label, u32 len) {
    if (len > 32) len = 32;
    B2b b;
    b2b_init(b, t.m);
    b2b_bytes(b, label, len);
    b2b_zeros(b, 32 - len);
    b2b_final(b, t.s);
    t.n_rounds = 0;
}
ZG_DEV void fs_append_bytes(FsT &t, const uint8_t *p, size_t n) {  // :123-156
    B2b b = fs_begin(t);
    b2b_bytes(b, p, n);
    fs_end(t, b);
}
ZG_DEV void fs_append_message(FsT &t, const char *msg, u32 len) {  // :96-120: right-padded to 32; a longer message is cut to 32
    if (len > 32) len = 32;
    B2b b = fs_begin(t);
    for (u32 i = 0; i < len; i++) b2b_byte(b, (u32)(uint8_t)msg[i]);
    b2b_zeros(b, 32 - len);
    fs_end(t, b);
}
ZG_DEV void fs_append_u64(FsT &t, u64 x) {  // :160-176
    B2b b = fs_begin(t);
    b2b_zeros(b, 24);
    b2b_be64(b, x);
    fs_end(t, b);
}
ZG_DEV void fs_append_scalar(FsT &t, const FsFr &mont) {  // :182-200: the canonical value, 32 big-endian bytes
    const FsFr v = fe_from_mont(mont);
    B2b b = fs_begin(t);
    for (int i = 7; i >= 0; i--) b2b_be32(b, v.l[i]);
    fs_end(t, b);
}
// the first 16 digest bytes of hash_with(empty) as a little-endian u128 (challengeBytes(16) reversed, read big-endian: :215-254)
ZG_DEV void fs_challenge_u128(FsT &t, u64 &lo, u64 &hi) {
    B2b b = fs_begin(t);
    fs_end(t, b);
    lo = t.s[0];
    hi = t.s[1];
}
// challengeScalar (:332-388): 125 bits, kept as the RAW limbs [0, 0, lo, hi] — no Montgomery conversion
ZG_DEV FsFr fs_challenge_scalar(FsT &t) {
    u64 lo, hi;
    fs_challenge_u128(t, lo, hi);
    hi &= (1ull << 61) - 1;
    FsFr r = FsFr::zero();
    r.l[4] = (u32)lo;
    r.l[5] = (u32)(lo >> 32);
    r.l[6] = (u32)hi;
    r.l[7] = (u32)(hi >> 32);
    return r;
}
// challengeScalarFull (:279-309): the same 16 digest bytes, unmasked, REVERSED and then read little-endian — the big-endian reading of the
// digest's first 16 bytes (the reference reverses here and reads .little, where challengeU128 reverses and reads .big) — as a proper
// Montgomery element
ZG_DEV u64 fs_bswap64(u64 x) {
    x = ((x & 0x00ff00ff00ff00ffull) << 8) | ((x >> 8) & 0x00ff00ff00ff00ffull);
    x = ((x & 0x0000ffff0000ffffull) << 16) | ((x >> 16) & 0x0000ffff0000ffffull);
    return (x << 32) | (x >> 32);
}
ZG_DEV FsFr fs_challenge_scalar_full(FsT &t) {
    u64 w0, w1;
    fs_challenge_u128(t, w0, w1);
    const u64 lo = fs_bswap64(w1), hi = fs_bswap64(w0);
    FsFr r = FsFr::zero();
    r.l[0] = (u32)lo;
    r.l[1] = (u32)(lo >> 32);
    r.l[2] = (u32)hi;
    r.l[3] = (u32)(hi >> 32);
    return fe_to_mont(r);
}

// ---- the round step of a batched sumcheck over k <= 8 instances
constexpr int FS_MAX_INST = 8;
constexpr u32 FS_EVALS_ALL = 0, FS_DERIVE_1 = 1, FS_DERIVE_13 = 2, FS_QUADRATIC = 3;
// what a run keeps resident, as words in HBM. The kernels of a round write an instance's sums to sums[i]; the step reads them, and
// leaves the challenge in r, where the next round's folds read it.
struct FsRunState {
    u64 claim[4];                  // the combined claim
    u64 r[4];                      // the last challenge (raw limbs [0, 0, lo, hi])
    u64 inst_claim[FS_MAX_INST][4];
    u64 coeff[FS_MAX_INST][4];
    u64 sums[FS_MAX_INST][16];     // s(0), s(1), s(2), s(3) of the instance's current round
    u32 num_rounds[FS_MAX_INST], kind[FS_MAX_INST];
    u32 k, max_rounds, round, rule;  // rule 0: an inactive instance weighs 2^(M - n_i - j - 1) (the proof converter's), 1: 2^(M - n_i - j)
};
ZG_DEV FsFr fs_ld(const u64 *w) {
    FsFr r;
    for (int i = 0; i < 4; i++) {
        r.l[2 * i] = (u32)w[i];
        r.l[2 * i + 1] = (u32)(w[i] >> 32);
    }
    return r;
}
ZG_DEV void fs_st(u64 *w, const FsFr &v) {
    for (int i = 0; i < 4; i++) w[i] = (u64)v.l[2 * i] | ((u64)v.l[2 * i + 1] << 32);
}
ZG_DEV FsFr fs_const(const u32 (&w)[8]) {
    FsFr r;
    for (int i = 0; i < 8; i++) r.l[i] = w[i];
    return r;
}
ZG_DEV FsFr fs_inv2() {  // 1/2 and 1/6 as Montgomery elements
    const u32 w[8] = {0x1ffffffeu, 0x783c14d8u, 0x0c8d1eddu, 0xaf982f6fu, 0xfcfd4f45u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au};
    return fs_const(w);
}
ZG_DEV FsFr fs_inv6() {
    const u32 w[8] = {0x0aaaaaaau, 0x7d695c48u, 0xaed9b4f4u, 0x3a880fcfu, 0xa9a9c517u, 0xda7526dbu, 0x69deea8eu, 0x0a67cbb3u};
    return fs_const(w);
}
ZG_DEV FsFr fs_times(const FsFr &a, u32 n) {  // n a, n small
    FsFr r = FsFr::zero();
    for (u32 i = 0; i < n; i++) r = fe_add(r, a);
    return r;
}
ZG_DEV FsFr fs_shl(FsFr a, u32 n) {  // a 2^n
    for (u32 i = 0; i < n; i++) a = fe_dbl(a);
    return a;
}
// UniPoly.interpolateDegree3 (src/poly/mod.zig:632-677): the coefficients of the cubic through p(0..3)
ZG_DEV void fs_interpolate3(const FsFr (&p)[4], FsFr (&c)[4]) {
    const FsFr inv2 = fs_inv2(), inv6 = fs_inv6();
    c[0] = p[0];
    // c1 = (-11 p0 + 18 p1 - 9 p2 + 2 p3) / 6, c2 = (2 p0 - 5 p1 + 4 p2 - p3) / 2, c3 = (-p0 + 3 p1 - 3 p2 + p3) / 6
    const FsFr n1 = fe_sub(fe_add(fs_times(p[1], 18), fe_dbl(p[3])), fe_add(fs_times(p[0], 11), fs_times(p[2], 9)));
    const FsFr n2 = fe_sub(fe_add(fe_dbl(p[0]), fs_times(p[2], 4)), fe_add(fs_times(p[1], 5), p[3]));
    const FsFr n3 = fe_sub(fe_add(fs_times(p[1], 3), p[3]), fe_add(p[0], fs_times(p[2], 3)));
    c[1] = fe_mul(n1, inv6);
    c[2] = fe_mul(n2, inv2);
    c[3] = fe_mul(n3, inv6);
}
ZG_DEV FsFr fs_horner3(const FsFr (&c)[4], const FsFr &r) {  // c0 + c1 r + c2 r^2 + c3 r^3
    FsFr v = fe_add(fe_mul(c[3], r), c[2]);
    v = fe_add(fe_mul(v, r), c[1]);
    return fe_add(fe_mul(v, r), c[0]);
}
// the decompression of :380-400: c1 = claim - 2 c0 - c2 - c3 — from the CLAIM, not from the combined values (c[1] is not read) —
// and the next claim c0 + c1 r + c2 r^2 + c3 r^3
ZG_DEV FsFr fs_next_claim(const FsFr &claim, const FsFr (&c)[4], const FsFr &r) {
    const FsFr d[4] = {c[0], fe_sub(fe_sub(fe_sub(claim, fe_dbl(c[0])), c[2]), c[3]), c[2], c[3]};
    return fs_horner3(d, r);
}
// One round (batched_sumcheck.zig:193-247, 362-400; the loop of proof_converter.zig:3026-3400): completes the instances' values by
// their kinds, combines them, compresses, absorbs, draws r, moves every claim on. log16: [c0, c2, c3, r], what the proof records.
ZG_DEV void fs_round_step(FsRunState &S, FsT &t, u64 *log16) {
    const u32 j = S.round, M = S.max_rounds;
    FsFr comb[4] = {FsFr::zero(), FsFr::zero(), FsFr::zero(), FsFr::zero()};
    for (u32 i = 0; i < S.k && i < (u32)FS_MAX_INST; i++) {
        const u32 start = M - S.num_rounds[i];
        const FsFr co = fs_ld(S.coeff[i]), cl = fs_ld(S.inst_claim[i]);
        if (j >= start) {
            FsFr s[4];
            for (int q = 0; q < 4; q++) s[q] = fs_ld(S.sums[i] + 4 * q);
            const u32 kind = S.kind[i];
            if (kind == FS_DERIVE_1 || kind == FS_DERIVE_13) s[1] = fe_sub(cl, s[0]);
            if (kind == FS_DERIVE_13) s[3] = fe_add(fe_sub(s[0], fs_times(s[1], 3)), fs_times(s[2], 3));
            if (kind == FS_QUADRATIC) s[3] = fe_add(fe_sub(fs_times(s[2], 3), fs_times(s[1], 3)), s[0]);
            for (int q = 0; q < 4; q++) {
                fs_st(S.sums[i] + 4 * q, s[q]);
                comb[q] = fe_add(comb[q], fe_mul(co, s[q]));
            }
        } else {
            const FsFr w = fe_mul(co, fs_shl(cl, start - j - (S.rule == 0 ? 1u : 0u)));
            for (int q = 0; q < 4; q++) comb[q] = fe_add(comb[q], w);
        }
    }
    FsFr c[4];
    fs_interpolate3(comb, c);
    fs_append_message(t, "UniPoly_begin", 13);
    fs_append_scalar(t, c[0]);
    fs_append_scalar(t, c[2]);
    fs_append_scalar(t, c[3]);
    fs_append_message(t, "UniPoly_end", 11);
    const FsFr r = fs_challenge_scalar(t);
    fs_st(S.claim, fs_next_claim(fs_ld(S.claim), c, r));
    for (u32 i = 0; i < S.k && i < (u32)FS_MAX_INST; i++) {
        if (j < M - S.num_rounds[i]) continue;
        FsFr s[4], ci[4];
        for (int q = 0; q < 4; q++) s[q] = fs_ld(S.sums[i] + 4 * q);
        fs_interpolate3(s, ci);
        fs_st(S.inst_claim[i], fs_horner3(ci, r));
    }
    fs_st(S.r, r);
    fs_st(log16, c[0]);
    fs_st(log16 + 4, c[2]);
    fs_st(log16 + 8, c[3]);
    fs_st(log16 + 12, r);
    S.round = j + 1;
}
// setupBatching (:127-186): every input claim absorbed, one challengeScalarFull per instance (when sampled), then the combined claim
// sum coeff_i 2^(M - n_i) claim_i
ZG_DEV void fs_setup_batching(FsRunState &S, FsT &t, bool sample) {
    const u32 k = S.k < (u32)FS_MAX_INST ? S.k : (u32)FS_MAX_INST;  // S may lie in device memory: never index past the arrays
    if (sample) {
        for (u32 i = 0; i < k; i++) fs_append_scalar(t, fs_ld(S.inst_claim[i]));
        for (u32 i = 0; i < k; i++) fs_st(S.coeff[i], fs_challenge_scalar_full(t));
    }
    FsFr acc = FsFr::zero();
    for (u32 i = 0; i < k; i++)
        acc = fe_add(acc, fe_mul(fs_ld(S.coeff[i]), fs_shl(fs_ld(S.inst_claim[i]), S.max_rounds - S.num_rounds[i])));
    fs_st(S.claim, acc);
}

}  // namespace zg
