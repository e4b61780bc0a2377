// msm.hpp — zolt.msm: AffinePoint, G2Point, MSM, BatchMSM, ParallelMSM, Dory row commitments and fold steps, device / sharded base handles.
// Part of zolt_host.hpp (the C++ host mirror over include/zolt_gpu.h); included by it, after the parts it depends on.
#pragma once
#ifndef ZOLT_HOST_UMBRELLA
#error "include zolt_host.hpp"
#endif
namespace zolt {

// ---------------------------------------------------------------- msm
struct AffinePoint {  // src/msm/mod.zig:15-49
    Fp x, y;
    bool infinity;
    static AffinePoint identity() { return AffinePoint{{{0, 0, 0, 0}}, {{0, 0, 0, 0}}, true}; }
    static AffinePoint generator() {
        AffinePoint g;
        std::memcpy(g.x.limbs, Fp::ONE, 32);
        std::memcpy(g.y.limbs, Fp::TWO, 32);
        g.infinity = false;
        return g;
    }
    bool isIdentity() const { return infinity; }
    bool eql(const AffinePoint &o) const {
        if (infinity && o.infinity) return true;
        if (infinity || o.infinity) return false;
        return std::memcmp(x.limbs, o.x.limbs, 32) == 0 && std::memcmp(y.limbs, o.y.limbs, 32) == 0;
    }
    // add (:74-103) / double (:118-138): lambda formulas, one inversion; on the device (zg_g1_affine_add_batch)
    AffinePoint add(const AffinePoint &o) const {
        uint64_t a[8], b[8], out[8];
        uint8_t ai = infinity ? 1 : 0, bi = o.infinity ? 1 : 0, oi = 0;
        std::memcpy(a, x.limbs, 32); std::memcpy(a + 4, y.limbs, 32);
        std::memcpy(b, o.x.limbs, 32); std::memcpy(b + 4, o.y.limbs, 32);
        check(zg_g1_affine_add_batch(a, &ai, b, &bi, 1, out, &oi), "zg_g1_affine_add_batch");
        AffinePoint r;
        std::memcpy(r.x.limbs, out, 32); std::memcpy(r.y.limbs, out + 4, 32);
        r.infinity = oi != 0;
        return r;
    }
    AffinePoint dbl() const { return add(*this); }  // `double` is a C++ keyword
};

inline void pack_points(const std::vector<AffinePoint> &pts, std::vector<uint64_t> &xy, std::vector<uint8_t> &inf) {
    xy.resize(pts.size() * 8);
    inf.resize(pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
        std::memcpy(&xy[8 * i], pts[i].x.limbs, 32);
        std::memcpy(&xy[8 * i + 4], pts[i].y.limbs, 32);
        inf[i] = pts[i].infinity ? 1 : 0;
    }
}
inline AffinePoint unpack_point(const uint64_t *xy, uint8_t inf) {
    AffinePoint p;
    std::memcpy(p.x.limbs, xy, 32);
    std::memcpy(p.y.limbs, xy + 4, 32);
    p.infinity = inf != 0;
    return p;
}

// device-resident bases: the GPU image of SetupParams.powers_of_tau_g1
class DeviceBases {
public:
    explicit DeviceBases(const std::vector<AffinePoint> &pts, const zg_msm_config *cfg = nullptr) : n_(pts.size()) {
        std::vector<uint64_t> xy;
        std::vector<uint8_t> inf;
        pack_points(pts, xy, inf);
        check(zg_g1_bases_upload(xy.data(), inf.data(), n_, cfg, &h_), "zg_g1_bases_upload");
    }
    // HyperKZG.setup's G1 side built on the device (zg_hyperkzg_setup): tau^i * base for i < n; the points come back only when asked for
    DeviceBases(const AffinePoint &base, const Fr &tau, size_t n, std::vector<uint64_t> *xy_out = nullptr, std::vector<uint8_t> *inf_out = nullptr,
                const zg_msm_config *cfg = nullptr) : n_(n) {
        uint64_t b[8];
        std::memcpy(b, base.x.limbs, 32);
        std::memcpy(b + 4, base.y.limbs, 32);
        if (xy_out) xy_out->resize(8 * n);
        if (inf_out) inf_out->resize(n);
        check(zg_hyperkzg_setup(b, tau.limbs, n, cfg, xy_out ? xy_out->data() : nullptr, inf_out ? inf_out->data() : nullptr, &h_), "zg_hyperkzg_setup");
    }
    // n records of a key file decoded, checked and built into the handle on the device (zg_g1_bases_from_bytes; encoding ZG_POINT_BYTES_*):
    // no point returns to the host. first_bad (optional) receives the smallest bad index before the GpuError of a bad record
    DeviceBases(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, const zg_msm_config *cfg = nullptr, size_t *first_bad = nullptr) : n_(n) {
        check(zg_g1_bases_from_bytes(bytes, n, encoding, flags, cfg, &h_, first_bad), "zg_g1_bases_from_bytes");
    }
    ~DeviceBases() { zg_g1_bases_free(h_); }
    DeviceBases(const DeviceBases &) = delete;
    DeviceBases &operator=(const DeviceBases &) = delete;
    size_t len() const { return n_; }
    AffinePoint msm(const Fr *scalars, size_t n, size_t off = 0) const {
        uint64_t out[8];
        uint8_t inf = 0;
        check(zg_msm_g1(h_, off, n, reinterpret_cast<const uint64_t *>(scalars), out, &inf), "zg_msm_g1");
        return unpack_point(out, inf);
    }
    // scalars given as u64 machine words: = msm(F.fromU64 of every word), 8 bytes per scalar across PCIe (zg_msm_g1_u64)
    AffinePoint msmU64(const uint64_t *values, size_t n, size_t off = 0) const {
        uint64_t out[8];
        uint8_t inf = 0;
        check(zg_msm_g1_u64(h_, off, n, values, out, &inf), "zg_msm_g1_u64");
        return unpack_point(out, inf);
    }
    zg_bases_t handle() const { return h_; }

private:
    zg_bases_t h_ = nullptr;
    size_t n_;
};

struct MSM {  // MSM(Fr, Fp), src/msm/mod.zig:345-542
    // compute(bases, scalars) — :355-372. Lengths must match (std.debug.assert :359).
    static AffinePoint compute(const std::vector<AffinePoint> &bases, const std::vector<Fr> &scalars) {
        if (bases.size() != scalars.size()) throw std::invalid_argument("MSM.compute: bases.len != scalars.len");
        if (bases.empty()) return AffinePoint::identity();
        DeviceBases d(bases);
        return d.msm(scalars.data(), scalars.size());
    }
    // scalarMul(base, scalar).toAffine() — :503-540
    static AffinePoint scalarMul(const AffinePoint &base, const Fr &scalar) {
        uint64_t xy[8], out[8];
        uint8_t inf = base.infinity ? 1 : 0, oinf = 0;
        std::memcpy(xy, base.x.limbs, 32);
        std::memcpy(xy + 4, base.y.limbs, 32);
        check(zg_g1_scalar_mul_batch(xy, &inf, scalar.limbs, 1, out, &oinf), "zg_g1_scalar_mul_batch");
        return unpack_point(out, oinf);
    }
};

struct BatchMSM {  // :545-565 (ParallelBatchMSM :683-748 returns the same values)
    static std::vector<AffinePoint> compute(const std::vector<AffinePoint> &bases, const std::vector<std::vector<Fr>> &batches) {
        std::vector<AffinePoint> out;
        if (batches.empty()) return out;
        DeviceBases d(bases);
        for (const auto &b : batches) out.push_back(d.msm(b.data(), b.size()));
        return out;
    }
};

// G2Point (src/field/pairing.zig:749-925): an affine point of the twist over Fp2 as the ABI lays it out — x.c0, x.c1, y.c0, y.c1
struct G2Point {
    uint64_t xy[16];
    bool infinity;
    static G2Point identity() {  // x = 0, y = (one, 0) (:754-760)
        G2Point p{};
        std::memcpy(p.xy + 8, Fp::ONE, 32);
        p.infinity = true;
        return p;
    }
    static G2Point generator() {  // :770-818, Montgomery limbs
        G2Point p{{
            0x8e83b5d102bc2026ULL, 0xdceb1935497b0172ULL, 0xfbb8264797811adfULL, 0x19573841af96503bULL,
            0xafb4737da84c6140ULL, 0x6043dd5a5802d8c4ULL, 0x09e950fc52a02f86ULL, 0x14fef0833aea7b6bULL,
            0x619dfa9d886be9f6ULL, 0xfe7fd297f59e9b78ULL, 0xff9e1a62231b7dfeULL, 0x28fd7eebae9e4206ULL,
            0x64095b56c71856eeULL, 0xdc57f922327d3cbbULL, 0x55f935be33351076ULL, 0x0da4a0e693fd6482ULL}, false};
        return p;
    }
    bool isIdentity() const { return infinity; }
    bool eql(const G2Point &o) const {
        if (infinity && o.infinity) return true;
        if (infinity || o.infinity) return false;
        return std::memcmp(xy, o.xy, 128) == 0;
    }
    G2Point add(const G2Point &o) const {  // :839-875, on the device (zg_g2_affine_add_batch)
        uint8_t ai = infinity ? 1 : 0, bi = o.infinity ? 1 : 0, oi = 0;
        G2Point r;
        check(zg_g2_affine_add_batch(xy, &ai, o.xy, &bi, 1, r.xy, &oi), "zg_g2_affine_add_batch");
        r.infinity = oi != 0;
        return r;
    }
    G2Point scalarMul(const Fr &s) const {  // :880-919 (zg_g2_scalar_mul_batch)
        uint8_t ai = infinity ? 1 : 0, oi = 0;
        G2Point r;
        check(zg_g2_scalar_mul_batch(xy, &ai, s.limbs, 1, r.xy, &oi), "zg_g2_scalar_mul_batch");
        r.infinity = oi != 0;
        return r;
    }
};

inline void pack_g2(const std::vector<G2Point> &pts, std::vector<uint64_t> &xy, std::vector<uint8_t> &inf) {
    xy.resize(pts.size() * 16);
    inf.resize(pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
        std::memcpy(&xy[16 * i], pts[i].xy, 128);
        inf[i] = pts[i].infinity ? 1 : 0;
    }
}
inline std::vector<G2Point> unpack_g2(const std::vector<uint64_t> &xy, const std::vector<uint8_t> &inf) {
    std::vector<G2Point> out(inf.size());
    for (size_t i = 0; i < inf.size(); i++) {
        std::memcpy(out[i].xy, &xy[16 * i], 128);
        out[i].infinity = inf[i] != 0;
    }
    return out;
}

// ---- Dory's wire forms (src/poly/commitment/dory.zig:41-210, src/field/pairing.zig:624-690): host arithmetic on single Fp values
// fromMontgomery of an Fp element: a * 1 / 2^256 mod p, canonical (src/field/mod.zig:642-645)
inline void fp_from_montgomery(const uint64_t a[4], uint64_t out[4]) {
    static const uint64_t MOD[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    const uint64_t INV = 0x87d20782e4866389ULL;  // -p^-1 mod 2^64
    uint64_t t[5] = {a[0], a[1], a[2], a[3], 0};
    for (int i = 0; i < 4; i++) {  // four reduction steps: t = (t + m * p) / 2^64
        const uint64_t m = t[0] * INV;
        unsigned __int128 c = (unsigned __int128)m * MOD[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; j++) {
            c += (unsigned __int128)m * MOD[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = (uint64_t)(c >> 64);
    }
    bool ge = t[4] != 0;
    if (!ge) {
        ge = true;
        for (int i = 3; i >= 0; i--)
            if (t[i] != MOD[i]) { ge = t[i] > MOD[i]; break; }
    }
    if (ge) {
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; i++) {
            unsigned __int128 x = (unsigned __int128)t[i] - MOD[i] - (uint64_t)br;
            t[i] = (uint64_t)x;
            br = (x >> 64) & 1;
        }
    }
    std::memcpy(out, t, 32);
}
// (y <= -y) as integers, y canonical: yIsPositive (dory.zig:162-175; equal — y = 0 — counts as positive)
inline bool fp_le_negation(const uint64_t y[4], int *cmp_out = nullptr) {
    static const uint64_t MOD[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    uint64_t neg[4] = {0, 0, 0, 0};
    if (y[0] | y[1] | y[2] | y[3]) {
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; i++) {
            unsigned __int128 x = (unsigned __int128)MOD[i] - y[i] - (uint64_t)br;
            neg[i] = (uint64_t)x;
            br = (x >> 64) & 1;
        }
    }
    int cmp = 0;
    for (int i = 3; i >= 0 && cmp == 0; i--) cmp = y[i] < neg[i] ? -1 : y[i] > neg[i] ? 1 : 0;
    if (cmp_out) *cmp_out = cmp;
    return cmp <= 0;
}
inline void put_le(const uint64_t v[4], uint8_t *out) {
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(v[i] >> (8 * b));
}
// compressG1 (:51-78): x little-endian, 0x40 in the last byte for the identity (all else zero), 0x80 when y > -y
inline std::array<uint8_t, 32> compressG1(const uint64_t xy[8], bool infinity) {
    std::array<uint8_t, 32> out{};
    if (infinity) {
        out[31] = 0x40;
        return out;
    }
    uint64_t x[4], y[4];
    fp_from_montgomery(xy, x);
    fp_from_montgomery(xy + 4, y);
    put_le(x, out.data());
    out[31] = (uint8_t)((out[31] & 0x3F) | (fp_le_negation(y) ? 0 : 0x80));
    return out;
}
inline std::array<uint8_t, 32> compressG1(const AffinePoint &p) {
    uint64_t xy[8];
    std::memcpy(xy, p.x.limbs, 32);
    std::memcpy(xy + 4, p.y.limbs, 32);
    return compressG1(xy, p.infinity);
}
// compressG2 (:179-210): x.c0, x.c1 little-endian, flags as compressG1; fp2IsPositive (:320-344) compares c1 first, then c0
inline std::array<uint8_t, 64> compressG2(const uint64_t xy[16], bool infinity) {
    std::array<uint8_t, 64> out{};
    if (infinity) {
        out[63] = 0x40;
        return out;
    }
    uint64_t c[4][4];
    for (int k = 0; k < 4; k++) fp_from_montgomery(xy + 4 * k, c[k]);
    put_le(c[0], out.data());
    put_le(c[1], out.data() + 32);
    int cmp1 = 0, cmp0 = 0;
    fp_le_negation(c[3], &cmp1);
    fp_le_negation(c[2], &cmp0);
    const bool positive = cmp1 < 0 || (cmp1 == 0 && cmp0 <= 0);
    out[63] = (uint8_t)((out[63] & 0x3F) | (positive ? 0 : 0x80));
    return out;
}
// Fp12.toBytes (pairing.zig:624-690) of a 48-word GT element: twelve canonical Fp values, little-endian
inline std::array<uint8_t, 384> gtToBytes(const uint64_t gt[48]) {
    std::array<uint8_t, 384> out{};
    for (int k = 0; k < 12; k++) {
        uint64_t c[4];
        fp_from_montgomery(gt + 4 * k, c);
        put_le(c, out.data() + 32 * k);
    }
    return out;
}

// DoryProof (:456-536) as the session's message records (include/zolt_gpu.h, "Dory opening (session)")
struct DoryProof {
    std::array<uint64_t, ZG_DORY_VMV_WORDS> vmv_message;
    std::vector<std::array<uint64_t, ZG_DORY_FIRST_WORDS>> first_messages;
    std::vector<std::array<uint64_t, ZG_DORY_SECOND_WORDS>> second_messages;
    std::array<uint64_t, ZG_DORY_FINAL_WORDS> final_message;
    uint32_t nu = 0, sigma = 0;
    // toBytes (:481-535): VMV, the round count, the first messages, the second messages, the final message, nu, sigma
    std::vector<uint8_t> toBytes() const {
        std::vector<uint8_t> out;
        auto gt = [&](const uint64_t *w) { auto b = gtToBytes(w); out.insert(out.end(), b.begin(), b.end()); };
        auto g1 = [&](const uint64_t *r) { auto b = compressG1(r, (r[8] & 1) != 0); out.insert(out.end(), b.begin(), b.end()); };
        auto g2 = [&](const uint64_t *r) { auto b = compressG2(r, (r[16] & 1) != 0); out.insert(out.end(), b.begin(), b.end()); };
        auto u32 = [&](uint32_t v) { for (int b = 0; b < 4; b++) out.push_back((uint8_t)(v >> (8 * b))); };
        gt(vmv_message.data()); gt(vmv_message.data() + 48); g1(vmv_message.data() + 96);
        u32((uint32_t)first_messages.size());
        for (const auto &m : first_messages) {
            for (int k = 0; k < 4; k++) gt(m.data() + 48 * k);
            g1(m.data() + 192); g2(m.data() + 201);
        }
        for (const auto &m : second_messages) {
            gt(m.data()); gt(m.data() + 48);
            g1(m.data() + 96); g1(m.data() + 105); g2(m.data() + 114); g2(m.data() + 131);
        }
        g1(final_message.data()); g2(final_message.data() + 9);
        u32(nu); u32(sigma);
        return out;
    }
    // writeDoryProof (src/zkvm/jolt_serialization.zig:148-185), the form a proof file carries. The reference's two serialisers write the
    // same fields in the same order and widths, so this is toBytes under the name of the writer
    std::vector<uint8_t> toArkBytes() const { return toBytes(); }
};

// Dory's data-parallel G1 / G2 / Fr pieces (src/poly/commitment/dory.zig) and openWithTranscript over the device-resident session;
// GT exponentiation and the verifier stay the reference's
struct Dory {
    // `x.inverse() orelse F.one()` (:1575, :1613, :1639)
    static Fr inverseOrOne(const Fr &x) {
        Fr r;
        return x.inverse(r) ? r : Fr::one();
    }
    // openWithTranscript (:1404-1669): the vectors cross once, at begin (zg_dory_open_begin); every round then moves two messages out and
    // its challenges in. row_commitments == nullptr: computed (:1417-1423). Transcript: appendGT / appendG1Compressed / appendG2Compressed /
    // challengeScalar (Blake2bTranscript).
    template <class TranscriptT>
    static DoryProof openWithTranscript(const std::vector<AffinePoint> &g1_vec, const std::vector<G2Point> &g2_vec, unsigned nu, unsigned sigma,
                                        const std::vector<Fr> &evals, const std::vector<Fr> &point, const std::vector<AffinePoint> *row_commitments,
                                        TranscriptT &transcript) {
        std::vector<AffinePoint> rows;
        if (row_commitments) rows = *row_commitments;
        else {
            zg_msm_config cfg = {0, 0, 4};
            DeviceBases bases(std::vector<AffinePoint>(g1_vec.begin(), g1_vec.begin() + std::min(g1_vec.size(), size_t(1) << sigma)), &cfg);
            rows = computeRowCommitments(bases, evals, size_t(1) << sigma);
        }
        auto lr = computeEvaluationVectors(point, nu, sigma);
        const std::vector<Fr> v_vec = computeVectorMatrixProduct(evals, lr.first, nu, sigma);
        std::vector<uint64_t> g1_xy, g2_xy, rows_xy;
        std::vector<uint8_t> g1_inf, g2_inf, rows_inf;
        pack_points(g1_vec, g1_xy, g1_inf);
        pack_g2(g2_vec, g2_xy, g2_inf);
        pack_points(rows, rows_xy, rows_inf);
        DoryProof proof;
        proof.nu = nu;
        proof.sigma = sigma;
        zg_dory_t ses = nullptr;
        check(zg_dory_open_begin(g1_xy.data(), g1_inf.data(), g2_xy.data(), g2_inf.data(), std::min(g1_vec.size(), g2_vec.size()), rows_xy.data(), rows_inf.data(),
                                 rows.size(), reinterpret_cast<const uint64_t *>(v_vec.data()), v_vec.size(), reinterpret_cast<const uint64_t *>(lr.second.data()),
                                 reinterpret_cast<const uint64_t *>(lr.first.data()), nu, sigma, proof.vmv_message.data(), &ses), "zg_dory_open_begin");
        struct Closer {
            zg_dory_t s;
            ~Closer() { zg_dory_open_close(s); }
        } closer{ses};
        const uint64_t *v = proof.vmv_message.data();
        transcript.appendGT(v);
        transcript.appendGT(v + 48);
        transcript.appendG1Compressed(v + 96, (v[104] & 1) != 0);
        for (unsigned rnd = 0; rnd < sigma; rnd++) {
            proof.first_messages.emplace_back();
            uint64_t *m = proof.first_messages.back().data();
            check(zg_dory_open_first_message(ses, m), "zg_dory_open_first_message");
            for (int k = 0; k < 4; k++) transcript.appendGT(m + 48 * k);
            transcript.appendG1Compressed(m + 192, (m[200] & 1) != 0);
            transcript.appendG2Compressed(m + 201, (m[217] & 1) != 0);
            const Fr beta = transcript.challengeScalar(), beta_inv = inverseOrOne(beta);
            proof.second_messages.emplace_back();
            m = proof.second_messages.back().data();
            check(zg_dory_open_second_message(ses, beta.limbs, beta_inv.limbs, m), "zg_dory_open_second_message");
            transcript.appendGT(m);
            transcript.appendGT(m + 48);
            transcript.appendG1Compressed(m + 96, (m[104] & 1) != 0);
            transcript.appendG1Compressed(m + 105, (m[113] & 1) != 0);
            transcript.appendG2Compressed(m + 114, (m[130] & 1) != 0);
            transcript.appendG2Compressed(m + 131, (m[147] & 1) != 0);
            const Fr alpha = transcript.challengeScalar(), alpha_inv = inverseOrOne(alpha);
            check(zg_dory_open_fold(ses, alpha.limbs, alpha_inv.limbs), "zg_dory_open_fold");
        }
        const Fr gamma = transcript.challengeScalar(), gamma_inv = inverseOrOne(gamma);
        check(zg_dory_open_final(ses, gamma.limbs, gamma_inv.limbs, proof.final_message.data()), "zg_dory_open_final");
        (void)transcript.challengeScalar();  // the final d challenge keeps the transcript in sync (:1658)
        return proof;
    }
    // computeRowCommitments (:646-670): row r = MSM(g1_vec[0..len(row)], row r); full rows in one fused launch set, a shorter last row after
    static std::vector<AffinePoint> computeRowCommitments(const DeviceBases &g1_vec, const std::vector<Fr> &evals, size_t num_columns) {
        const size_t full = evals.size() / num_columns, rest = evals.size() % num_columns;
        std::vector<AffinePoint> out;
        if (full) {
            std::vector<const uint64_t *> ptrs;
            for (size_t r = 0; r < full; r++) ptrs.push_back(reinterpret_cast<const uint64_t *>(evals.data() + r * num_columns));
            std::vector<uint64_t> xy(8 * full);
            std::vector<uint8_t> inf(full);
            check(zg_msm_g1_batch(g1_vec.handle(), num_columns, ptrs.data(), full, xy.data(), inf.data()), "zg_msm_g1_batch");
            for (size_t r = 0; r < full; r++) out.push_back(unpack_point(xy.data() + 8 * r, inf[r]));
        }
        if (rest) out.push_back(g1_vec.msm(evals.data() + full * num_columns, rest));
        return out;
    }
    // multilinearLagrangeBasis (:544-588): the eq table with the index's LOW bit on point[0] = the device's eq table of the reversed point;
    // a shorter output is its first entries
    static std::vector<Fr> multilinearLagrangeBasis(const std::vector<Fr> &point, size_t out_len = 0) {
        std::vector<Fr> full(size_t(1) << point.size(), Fr::one());
        if (!point.empty()) {
            std::vector<Fr> rev(point.rbegin(), point.rend());
            check(zg_fr_eq_table(reinterpret_cast<const uint64_t *>(rev.data()), rev.size(), nullptr, reinterpret_cast<uint64_t *>(full.data())), "zg_fr_eq_table");
        }
        if (out_len && out_len < full.size()) full.resize(out_len);
        return full;
    }
    // computeEvaluationVectors (:590-620) -> (left_vec of 2^nu, right_vec of 2^sigma entries)
    static std::pair<std::vector<Fr>, std::vector<Fr>> computeEvaluationVectors(const std::vector<Fr> &point, unsigned nu, unsigned sigma) {
        std::vector<Fr> left(size_t(1) << nu, Fr::zero()), right(size_t(1) << sigma, Fr::zero());
        const size_t d = point.size();
        auto put = [](std::vector<Fr> &dst, const std::vector<Fr> &src) { std::copy(src.begin(), src.end(), dst.begin()); };
        if (d <= sigma) {
            put(right, multilinearLagrangeBasis(point));
            left[0] = Fr::one();
        } else {
            put(right, multilinearLagrangeBasis(std::vector<Fr>(point.begin(), point.begin() + sigma)));
            put(left, multilinearLagrangeBasis(std::vector<Fr>(point.begin() + sigma, point.end()), d <= nu + sigma ? 0 : left.size()));
        }
        return {left, right};
    }
    // computeVectorMatrixProduct (:622-642): v[col] = sum_row left_vec[row] * evals[row * 2^sigma + col]
    static std::vector<Fr> computeVectorMatrixProduct(const std::vector<Fr> &evals, const std::vector<Fr> &left_vec, unsigned nu, unsigned sigma) {
        const size_t rows = size_t(1) << nu, cols = size_t(1) << sigma;
        std::vector<Fr> m(rows * cols, Fr::zero()), w(rows, Fr::zero()), out(cols);
        std::copy(evals.begin(), evals.begin() + std::min(evals.size(), rows * cols), m.begin());
        std::copy(left_vec.begin(), left_vec.begin() + std::min(left_vec.size(), rows), w.begin());
        check(zg_fr_weighted_colsum(reinterpret_cast<const uint64_t *>(m.data()), rows, cols, reinterpret_cast<const uint64_t *>(w.data()), 1,
                                    reinterpret_cast<uint64_t *>(out.data())), "zg_fr_weighted_colsum");
        return out;
    }
    // msmG2 (:693-703) over min(len) entries: one bucket MSM on the device instead of n scalar multiplications
    static G2Point msmG2(const std::vector<G2Point> &g2_vec, const std::vector<Fr> &scalars) {
        const size_t n = std::min(g2_vec.size(), scalars.size());
        std::vector<uint64_t> xy;
        std::vector<uint8_t> inf;
        pack_g2(g2_vec, xy, inf);
        G2Point r;
        uint8_t oi = 0;
        check(zg_msm_g2(xy.data(), inf.data(), reinterpret_cast<const uint64_t *>(scalars.data()), n, r.xy, &oi), "zg_msm_g2");
        r.infinity = oi != 0;
        return r;
    }
    // setup's g2_vec[i] = generator.scalarMul(hash_i) (:963-966) for scalars the caller derived; also v2's start (:1513-1519) with base g2_vec[0]
    static std::vector<G2Point> generateG2Points(const std::vector<Fr> &scalars, const G2Point &base = G2Point::generator()) {
        std::vector<uint64_t> xy(16 * scalars.size());
        std::vector<uint8_t> inf(scalars.size());
        check(zg_g2_fixed_base_mul_batch(base.xy, base.infinity ? 1 : 0, reinterpret_cast<const uint64_t *>(scalars.data()), scalars.size(), xy.data(), inf.data()),
              "zg_g2_fixed_base_mul_batch");
        return unpack_g2(xy, inf);
    }
    static std::vector<G2Point> initV2(const G2Point &g2_0, const std::vector<Fr> &v_vec, size_t vec_len) {
        std::vector<Fr> v(v_vec.begin(), v_vec.begin() + std::min(v_vec.size(), vec_len));
        std::vector<G2Point> out = generateG2Points(v, g2_0);
        out.resize(vec_len, G2Point::identity());
        return out;
    }
    // out[i] = s * a[i] + b[i] over the common length (zg_g2_axpy_batch / zg_g1_axpy_batch)
    static std::vector<G2Point> axpyG2(const std::vector<G2Point> &a, const std::vector<G2Point> &b, const Fr &s) {
        const size_t n = std::min(a.size(), b.size());
        std::vector<uint64_t> axy, bxy, oxy(16 * n);
        std::vector<uint8_t> ai, bi, oi(n);
        pack_g2(a, axy, ai);
        pack_g2(b, bxy, bi);
        check(zg_g2_axpy_batch(axy.data(), ai.data(), bxy.data(), bi.data(), s.limbs, n, oxy.data(), oi.data()), "zg_g2_axpy_batch");
        return unpack_g2(oxy, oi);
    }
    static std::vector<AffinePoint> axpyG1(const std::vector<AffinePoint> &a, const std::vector<AffinePoint> &b, const Fr &s) {
        const size_t n = std::min(a.size(), b.size());
        std::vector<uint64_t> axy, bxy, oxy(8 * n);
        std::vector<uint8_t> ai, bi, oi(n);
        pack_points(a, axy, ai);
        pack_points(b, bxy, bi);
        check(zg_g1_axpy_batch(axy.data(), ai.data(), bxy.data(), bi.data(), s.limbs, n, oxy.data(), oi.data()), "zg_g1_axpy_batch");
        std::vector<AffinePoint> out;
        for (size_t i = 0; i < n; i++) out.push_back(unpack_point(&oxy[8 * i], oi[i]));
        return out;
    }
    // :1578-1584 over the live entries (v1.size()): v1[i] += beta * g1_vec[i], v2[i] += beta_inv * g2_vec[i], in place
    static void applyFirstChallenge(std::vector<AffinePoint> &v1, std::vector<G2Point> &v2, const std::vector<AffinePoint> &g1_vec,
                                    const std::vector<G2Point> &g2_vec, const Fr &beta, const Fr &beta_inv) {
        v1 = axpyG1(std::vector<AffinePoint>(g1_vec.begin(), g1_vec.begin() + v1.size()), v1, beta);
        v2 = axpyG2(std::vector<G2Point>(g2_vec.begin(), g2_vec.begin() + v2.size()), v2, beta_inv);
    }
    // :1615-1632: the four vectors folded to their n2 = len / 2 live entries, in place
    static void foldVectors(std::vector<AffinePoint> &v1, std::vector<G2Point> &v2, std::vector<Fr> &s1, std::vector<Fr> &s2, const Fr &alpha,
                            const Fr &alpha_inv) {
        const size_t n2 = v1.size() / 2;
        v1 = axpyG1(std::vector<AffinePoint>(v1.begin(), v1.begin() + n2), std::vector<AffinePoint>(v1.begin() + n2, v1.begin() + 2 * n2), alpha);
        v2 = axpyG2(std::vector<G2Point>(v2.begin(), v2.begin() + n2), std::vector<G2Point>(v2.begin() + n2, v2.begin() + 2 * n2), alpha_inv);
        for (size_t i = 0; i < n2; i++) {
            s1[i] = alpha.mul(s1[i]).add(s1[i + n2]);
            s2[i] = alpha_inv.mul(s2[i]).add(s2[i + n2]);
        }
        s1.resize(n2);
        s2.resize(n2);
    }

    // ---- commitments over a resident key (include/zolt_gpu.h, "Dory commitments (key and batch)")
    // SHA3-256 of a message shorter than one block (136 bytes): all setup hashes (:952-955, :1676-1684)
    static std::array<uint8_t, 32> sha3_256_short(const uint8_t *msg, size_t n) {
        static const uint64_t RC[24] = {
            0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
            0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
            0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
            0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
        static const unsigned ROTC[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
        static const unsigned PILN[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
        if (n >= 136) throw std::invalid_argument("sha3_256_short: one block only");
        uint8_t block[136] = {0};
        std::memcpy(block, msg, n);
        block[n] ^= 0x06;  // SHA-3's domain bits, then pad10*1
        block[135] ^= 0x80;
        uint64_t st[25] = {0};
        for (int i = 0; i < 17; i++)
            for (int b = 7; b >= 0; b--) st[i] = (st[i] << 8) | block[8 * i + b];
        auto rotl = [](uint64_t x, unsigned r) { return (x << r) | (x >> (64 - r)); };
        for (int round = 0; round < 24; round++) {
            uint64_t bc[5];
            for (int i = 0; i < 5; i++) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
            for (int i = 0; i < 5; i++) {
                const uint64_t t = bc[(i + 4) % 5] ^ rotl(bc[(i + 1) % 5], 1);
                for (int j = i; j < 25; j += 5) st[j] ^= t;
            }
            uint64_t t = st[1];
            for (int i = 0; i < 24; i++) {
                const unsigned j = PILN[i];
                const uint64_t tmp = st[j];
                st[j] = rotl(t, ROTC[i]);
                t = tmp;
            }
            for (int row = 0; row < 25; row += 5) {
                for (int i = 0; i < 5; i++) bc[i] = st[row + i];
                for (int i = 0; i < 5; i++) st[row + i] = bc[i] ^ (~bc[(i + 1) % 5] & bc[(i + 2) % 5]);
            }
            st[0] ^= RC[round];
        }
        std::array<uint8_t, 32> out{};
        for (int i = 0; i < 4; i++)
            for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(st[i] >> (8 * b));
        return out;
    }
    struct SetupParams {  // :920-979 as far as the prover reads it
        std::vector<AffinePoint> g1_vec;
        std::vector<G2Point> g2_vec;
        unsigned nu = 0, sigma = 0;
    };
    // setup (:931-979): generator times Fr.fromBytes(SHA3-256(seed || u64le(index) || "G1" | "G2")), G2 indices offset by the column
    // count; the hashing is the host's, the points one fixed-base batch per group
    static SetupParams setup(unsigned max_num_vars) {
        SetupParams p;
        p.sigma = (max_num_vars + 1) / 2;
        p.nu = max_num_vars - p.sigma;
        const size_t cols = size_t(1) << p.sigma, rows = size_t(1) << p.nu;
        static const char URS[] = "Jolt Dory URS seed";
        const auto seed = sha3_256_short(reinterpret_cast<const uint8_t *>(URS), sizeof(URS) - 1);
        auto scalar = [&](uint64_t index, const char *tag) {
            uint8_t msg[42];
            std::memcpy(msg, seed.data(), 32);
            for (int b = 0; b < 8; b++) msg[32 + b] = (uint8_t)(index >> (8 * b));
            msg[40] = (uint8_t)tag[0];
            msg[41] = (uint8_t)tag[1];
            return Fr::fromBytes(sha3_256_short(msg, 42).data());
        };
        std::vector<Fr> a, b;
        for (size_t i = 0; i < cols; i++) a.push_back(scalar(i, "G1"));
        for (size_t i = 0; i < rows; i++) b.push_back(scalar(i + cols, "G2"));
        const AffinePoint g = AffinePoint::generator();
        uint64_t gxy[8];
        std::memcpy(gxy, g.x.limbs, 32);
        std::memcpy(gxy + 4, g.y.limbs, 32);
        std::vector<uint64_t> xy(8 * cols);
        std::vector<uint8_t> inf(cols);
        check(zg_g1_fixed_base_mul_batch(gxy, 0, reinterpret_cast<const uint64_t *>(a.data()), cols, xy.data(), inf.data()), "zg_g1_fixed_base_mul_batch");
        for (size_t i = 0; i < cols; i++) p.g1_vec.push_back(unpack_point(&xy[8 * i], inf[i]));
        p.g2_vec = generateG2Points(b);
        return p;
    }
    // the device-resident key: both generator vectors, the digit table, an MSM handle (zg_dory_key_*)
    class Key {
    public:
        Key(const std::vector<AffinePoint> &g1_vec, const std::vector<G2Point> &g2_vec) {
            std::vector<uint64_t> g1_xy, g2_xy;
            std::vector<uint8_t> g1_inf, g2_inf;
            pack_points(g1_vec, g1_xy, g1_inf);
            pack_g2(g2_vec, g2_xy, g2_inf);
            check(zg_dory_key_create(g1_xy.data(), g1_inf.data(), g1_vec.size(), g2_xy.data(), g2_inf.data(), g2_vec.size(), &h_), "zg_dory_key_create");
        }
        explicit Key(const SetupParams &p) : Key(p.g1_vec, p.g2_vec) {}
        // both vectors as the records of a file (ZG_POINT_BYTES_*), decoded on the device and built where they lie (zg_dory_key_from_bytes)
        Key(const uint8_t *g1_bytes, size_t n_g1, uint32_t g1_encoding, const uint8_t *g2_bytes, size_t n_g2, uint32_t g2_encoding, uint32_t flags = 0,
            size_t *first_bad = nullptr) {
            check(zg_dory_key_from_bytes(g1_bytes, n_g1, g1_encoding, g2_bytes, n_g2, g2_encoding, flags, &h_, first_bad), "zg_dory_key_from_bytes");
        }
        ~Key() { zg_dory_key_free(h_); }
        Key(const Key &) = delete;
        Key &operator=(const Key &) = delete;
        zg_dory_key_t handle() const { return h_; }

    private:
        zg_dory_key_t h_ = nullptr;
    };
    // loadFromFile (:740-822), the Jolt-exported SRS of `zolt prove --srs FILE`: "JOLT_DORY_SRS_V1" | u64 max_num_vars | u64 count + 64-byte
    // records | u64 count + 128-byte records | 192 bytes of h1 / h2 (skipped). The arkworks records (:828-924) are decoded on the device
    // and the key is built from them there. Errors: InvalidSrsFormat for a wrong magic, TruncatedData for a short file
    struct SrsError : std::runtime_error { using std::runtime_error::runtime_error; };
    struct LoadedKey {
        std::unique_ptr<Key> key;
        uint64_t max_num_vars = 0;
        unsigned nu = 0, sigma = 0;
    };
    static LoadedKey loadFromFile(const std::vector<uint8_t> &data) {
        size_t pos = 0;
        auto take = [&](size_t size) {
            if (size > data.size() - pos) throw SrsError("TruncatedData");
            const uint8_t *p = data.data() + pos;
            pos += size;
            return p;
        };
        auto u64le = [&] {
            const uint8_t *p = take(8);
            uint64_t v = 0;
            for (int b = 0; b < 8; b++) v |= (uint64_t)p[b] << (8 * b);
            return v;
        };
        if (data.size() < 16) throw SrsError("TruncatedData");
        if (std::memcmp(take(16), "JOLT_DORY_SRS_V1", 16) != 0) throw SrsError("InvalidSrsFormat");
        LoadedKey out;
        out.max_num_vars = u64le();
        const uint64_t n1 = u64le();
        if (n1 > data.size() / 64) throw SrsError("TruncatedData");
        const uint8_t *g1 = take((size_t)n1 * 64);
        const uint64_t n2 = u64le();
        if (n2 > data.size() / 128) throw SrsError("TruncatedData");
        const uint8_t *g2 = take((size_t)n2 * 128);
        take(64 + 128);
        out.sigma = (unsigned)((out.max_num_vars + 1) / 2);
        out.nu = (unsigned)(out.max_num_vars - out.sigma);
        out.key.reset(new Key(g1, (size_t)n1, ZG_POINT_BYTES_ARK, g2, (size_t)n2, ZG_POINT_BYTES_ARK));
        return out;
    }
    // one polynomial of a batch: kind ZG_DORY_POLY_*, data = len entries of 4 / 1 / 1 / 2 words, aux = sign bytes (ZG_DORY_POLY_U64) or null
    struct Poly {
        uint32_t kind;
        const uint64_t *data;
        size_t len;
        const uint8_t *aux = nullptr;
        uint32_t shift = 0, bits = 0;
    };
    using GT = std::array<uint64_t, 48>;
    // commit (:989-1042) for every polynomial in one call; row_commitments (optional): polynomial j's rows, what openWithTranscript takes
    static std::vector<GT> batchCommit(const Key &key, const std::vector<Poly> &polys, std::vector<std::vector<AffinePoint>> *row_commitments = nullptr) {
        const size_t k = polys.size();
        std::vector<uint32_t> kinds(k), shifts(k), bits(k);
        std::vector<const uint64_t *> data(k);
        std::vector<const uint8_t *> aux(k);
        std::vector<size_t> lens(k);
        std::vector<uint64_t> off(k + 1, 0);
        size_t total = 0;
        for (size_t j = 0; j < k; j++) {
            kinds[j] = polys[j].kind; data[j] = polys[j].data; aux[j] = polys[j].aux; lens[j] = polys[j].len; shifts[j] = polys[j].shift; bits[j] = polys[j].bits;
            size_t nv = 0;
            while ((size_t(2) << nv) <= lens[j]) nv++;
            if (lens[j] <= 1) nv = 1;
            total += lens[j] ? size_t(1) << (nv - (nv + 1) / 2) : 0;
        }
        std::vector<GT> out(k);
        std::vector<uint64_t> rows(9 * (total ? total : 1));
        check(zg_dory_commit_batch(key.handle(), k, kinds.data(), data.data(), aux.data(), lens.data(), shifts.data(), bits.data(),
                                   k ? out[0].data() : nullptr, row_commitments ? rows.data() : nullptr, off.data()), "zg_dory_commit_batch");
        if (row_commitments) {
            row_commitments->assign(k, {});
            for (size_t j = 0; j < k; j++)
                for (size_t r = off[j]; r < off[j + 1]; r++) (*row_commitments)[j].push_back(unpack_point(&rows[9 * r], (uint8_t)(rows[9 * r + 8] & 1)));
        }
        return out;
    }
    // open's constants in the place of a transcript (:1274, :1316, :1349): beta = round + 1 and alpha = round + 100 per round, then
    // gamma = 999, each followed by its `inverse() orelse one` — what zg_dory_open_run takes
    static std::vector<Fr> openChallenges(unsigned sigma) {
        std::vector<Fr> out;
        auto put = [&](uint64_t c) { const Fr x = Fr::fromU64(c); out.push_back(x); out.push_back(inverseOrOne(x)); };
        for (unsigned t = 0; t < sigma; t++) { put(t + 1); put(t + 100); }
        put(999);
        return out;
    }
    // openWithRowCommitments (:1062-1378), the opening the prover calls (src/zkvm/mod.zig:1374, :1485), over a resident key of the
    // params' generators — 2^sigma of G1, 2^nu of G2, read where the key holds them: ONE begin and ONE run (zolt_gpu.h, "Dory opening
    // (over a key, `open`)"). row_commitments == nullptr: computed (:1073-1080)
    static DoryProof openWithRowCommitments(const Key &key, const SetupParams &params, const std::vector<Fr> &evals, const std::vector<Fr> &point,
                                            const std::vector<AffinePoint> *row_commitments) {
        const unsigned nu = params.nu, sigma = params.sigma;
        std::vector<AffinePoint> rows;
        if (row_commitments) rows = *row_commitments;
        else {
            zg_msm_config cfg = {0, 0, 4};
            DeviceBases bases(std::vector<AffinePoint>(params.g1_vec.begin(), params.g1_vec.begin() + std::min(params.g1_vec.size(), size_t(1) << sigma)), &cfg);
            rows = computeRowCommitments(bases, evals, size_t(1) << sigma);
        }
        auto lr = computeEvaluationVectors(point, nu, sigma);
        const std::vector<Fr> v_vec = computeVectorMatrixProduct(evals, lr.first, nu, sigma);
        std::vector<uint64_t> rows_xy;
        std::vector<uint8_t> rows_inf;
        pack_points(rows, rows_xy, rows_inf);
        DoryProof proof;
        proof.nu = nu;
        proof.sigma = sigma;
        zg_dory_t ses = nullptr;
        check(zg_dory_open_key_begin(key.handle(), rows_xy.data(), rows_inf.data(), rows.size(), reinterpret_cast<const uint64_t *>(v_vec.data()), v_vec.size(),
                                     reinterpret_cast<const uint64_t *>(lr.second.data()), reinterpret_cast<const uint64_t *>(lr.first.data()), nu, sigma,
                                     proof.vmv_message.data(), &ses), "zg_dory_open_key_begin");
        struct Closer {
            zg_dory_t s;
            ~Closer() { zg_dory_open_close(s); }
        } closer{ses};
        const std::vector<Fr> ch = openChallenges(sigma);
        proof.first_messages.resize(sigma);
        proof.second_messages.resize(sigma);
        check(zg_dory_open_run(ses, reinterpret_cast<const uint64_t *>(ch.data()), sigma ? proof.first_messages[0].data() : nullptr,
                               sigma ? proof.second_messages[0].data() : nullptr, proof.final_message.data()), "zg_dory_open_run");
        return proof;
    }
    // open (:1052-1059)
    static DoryProof open(const Key &key, const SetupParams &params, const std::vector<Fr> &evals, const std::vector<Fr> &point) {
        return openWithRowCommitments(key, params, evals, point, nullptr);
    }
};

// zolt_gpu.h, "Pairings (engine)": runs a scope under one of the two pairing engines and puts back the engine that was set before. The
// setting is process-wide and the results have the same bits under either.
struct PairingEngine {
    int before;
    explicit PairingEngine(int engine) : before(zg_pairing_engine_get()) { check(zg_pairing_engine_set(engine), "zg_pairing_engine_set"); }
    ~PairingEngine() { (void)zg_pairing_engine_set(before); }
    PairingEngine(const PairingEngine &) = delete;
    PairingEngine &operator=(const PairingEngine &) = delete;
};

// DoryVerifierSetup (src/zkvm/preprocessing.zig:852-1166): the verifier half of the Dory key. Every pairing of fromSRS (:889-973) is one
// device call (zg_dory_verifier_setup[_points]); the copies the reference makes — delta_1l = delta_2l = (one, chi[0..K-1]), ht = chi[0] — are
// made here, and serialize writes that file's bytes with its own point encodings (not dory.zig's compressG1 / compressG2).
struct DoryVerifierSetup {
    using GT = std::array<uint64_t, 48>;
    std::vector<GT> delta_1l, delta_1r, delta_2l, delta_2r, chi;
    AffinePoint g1_0, h1;
    G2Point g2_0, h2;
    GT ht;
    size_t max_log_n = 0;

    static GT gtOne() {
        GT one{};
        std::memcpy(one.data(), Fp::ONE, 32);
        return one;
    }
    // fromSRS over host generators, as src/main.zig:431-489 builds them only for this: no key, no digit table
    static DoryVerifierSetup fromSRS(const std::vector<AffinePoint> &g1_vec, const std::vector<G2Point> &g2_vec) {
        std::vector<uint64_t> g1_xy, g2_xy;
        std::vector<uint8_t> g1_inf, g2_inf;
        pack_points(g1_vec, g1_xy, g1_inf);
        pack_g2(g2_vec, g2_xy, g2_inf);
        const size_t cap = zg_dory_verifier_setup_levels(g1_vec.size());
        std::vector<uint64_t> out(3 * 48 * (cap ? cap : 1));
        size_t levels = 0;
        check(zg_dory_verifier_setup_points(g1_xy.data(), g1_inf.data(), g1_vec.size(), g2_xy.data(), g2_inf.data(), g2_vec.size(), out.data(), cap, &levels),
              "zg_dory_verifier_setup_points");
        return assemble(out, levels, g1_vec[0], g2_vec[0]);
    }
    static DoryVerifierSetup fromSRS(const Dory::SetupParams &srs) { return fromSRS(srs.g1_vec, srs.g2_vec); }
    // fromSRS over a resident key; the first generators are the host's (a key hands no point back)
    static DoryVerifierSetup fromSRS(const Dory::Key &key, const AffinePoint &g1_first, const G2Point &g2_first) {
        size_t n_g1 = 0;
        check(zg_dory_key_len(key.handle(), &n_g1, nullptr), "zg_dory_key_len");
        const size_t cap = zg_dory_verifier_setup_levels(n_g1);
        std::vector<uint64_t> out(3 * 48 * (cap ? cap : 1));
        size_t levels = 0;
        check(zg_dory_verifier_setup(key.handle(), out.data(), cap, &levels), "zg_dory_verifier_setup");
        return assemble(out, levels, g1_first, g2_first);
    }
    // serialize (:977-1025): five length-prefixed GT vectors, g1_0, g2_0, h1, h2, ht, max_log_n as u64
    std::vector<uint8_t> serialize() const {
        std::vector<uint8_t> out;
        auto u64 = [&](uint64_t v) { for (int b = 0; b < 8; b++) out.push_back((uint8_t)(v >> (8 * b))); };
        auto gt = [&](const GT &g) { auto b = gtToBytes(g.data()); out.insert(out.end(), b.begin(), b.end()); };  // serializeGT (:1029-1059)
        for (const auto *vec : {&delta_1l, &delta_1r, &delta_2l, &delta_2r, &chi}) {
            u64(vec->size());
            for (const GT &g : *vec) gt(g);
        }
        auto g1 = [&](const AffinePoint &p) {
            uint64_t xy[8];
            std::memcpy(xy, p.x.limbs, 32);
            std::memcpy(xy + 4, p.y.limbs, 32);
            auto b = serializeG1(xy, p.infinity);
            out.insert(out.end(), b.begin(), b.end());
        };
        auto g2 = [&](const G2Point &p) { auto b = serializeG2(p.xy, p.infinity); out.insert(out.end(), b.begin(), b.end()); };
        g1(g1_0); g2(g2_0); g1(h1); g2(h2);
        gt(ht);
        u64(max_log_n);
        return out;
    }
    // serializeG1 (:1061-1090): bit 62 of the last limb alone for the identity; bit 63 unless y is lexicographicallyLess than -y (:1129-1139:
    // strictly — y = -y sets it, where compressG1 counts it positive)
    static std::array<uint8_t, 32> serializeG1(const uint64_t xy[8], bool infinity) {
        std::array<uint8_t, 32> out{};
        if (infinity) {
            out[31] = 0x40;
            return out;
        }
        uint64_t x[4], y[4];
        fp_from_montgomery(xy, x);
        fp_from_montgomery(xy + 4, y);
        int cmp = 0;
        fp_le_negation(y, &cmp);
        if (cmp >= 0) x[3] |= 0x8000000000000000ULL;
        put_le(x, out.data());
        return out;
    }
    // serializeG2 (:1092-1127): the flags in the last limb of x.c1; lexicographicallyLessFp2 (:1141-1166) compares c1 before c0, strictly
    static std::array<uint8_t, 64> serializeG2(const uint64_t xy[16], bool infinity) {
        std::array<uint8_t, 64> out{};
        if (infinity) {
            out[63] = 0x40;
            return out;
        }
        uint64_t c[4][4];
        for (int k = 0; k < 4; k++) fp_from_montgomery(xy + 4 * k, c[k]);
        int cmp1 = 0, cmp0 = 0;
        fp_le_negation(c[3], &cmp1);
        fp_le_negation(c[2], &cmp0);
        const bool positive = cmp1 < 0 || (cmp1 == 0 && cmp0 < 0);
        if (!positive) c[1][3] |= 0x8000000000000000ULL;
        put_le(c[0], out.data());
        put_le(c[1], out.data() + 32);
        return out;
    }

private:
    static DoryVerifierSetup assemble(const std::vector<uint64_t> &out, size_t levels, const AffinePoint &g1_first, const G2Point &g2_first) {
        DoryVerifierSetup vs;
        auto take = [&](std::vector<GT> &dst, size_t first) {
            dst.resize(levels);
            for (size_t k = 0; k < levels; k++) std::memcpy(dst[k].data(), &out[48 * (first + k)], 384);
        };
        take(vs.chi, 0);
        take(vs.delta_1r, levels);
        take(vs.delta_2r, 2 * levels);
        vs.delta_1l.push_back(gtOne());                                               // :905
        for (size_t k = 1; k < levels; k++) vs.delta_1l.push_back(vs.chi[k - 1]);     // :926
        vs.delta_2l = vs.delta_1l;                                                    // :940-945
        vs.g1_0 = vs.h1 = g1_first;                                                   // :950, :965
        vs.g2_0 = vs.h2 = g2_first;                                                   // :951, :966
        vs.ht = vs.chi[0];                                                            // :957: the pairing chi[0] is
        vs.max_log_n = 2 * (levels - 1);                                              // :970
        return vs;
    }
};

// the SRS sharded over the devices bound by zg_init_devices (one resident table per GPU)
class ShardedDeviceBases {
public:
    explicit ShardedDeviceBases(const std::vector<AffinePoint> &pts, const zg_msm_config *cfg = nullptr) : n_(pts.size()) {
        std::vector<uint64_t> xy;
        std::vector<uint8_t> inf;
        pack_points(pts, xy, inf);
        check(zg_g1_bases_upload_sharded(xy.data(), inf.data(), n_, cfg, &h_), "zg_g1_bases_upload_sharded");
    }
    ~ShardedDeviceBases() { zg_g1_sbases_free(h_); }
    ShardedDeviceBases(const ShardedDeviceBases &) = delete;
    ShardedDeviceBases &operator=(const ShardedDeviceBases &) = delete;
    size_t len() const { return n_; }
    int shards() const { return zg_g1_sbases_shards(h_); }
    AffinePoint msm(const Fr *scalars, size_t n) const {
        uint64_t out[8];
        uint8_t inf = 0;
        check(zg_msm_g1_sharded(h_, n, reinterpret_cast<const uint64_t *>(scalars), out, &inf), "zg_msm_g1_sharded");
        return unpack_point(out, inf);
    }
    std::vector<AffinePoint> msmBatch(const std::vector<std::vector<Fr>> &batches, size_t n) const {
        std::vector<const uint64_t *> ptrs;
        for (const auto &b : batches) ptrs.push_back(reinterpret_cast<const uint64_t *>(b.data()));
        std::vector<uint64_t> xy(8 * batches.size());
        std::vector<uint8_t> inf(batches.size());
        check(zg_msm_g1_batch_sharded(h_, n, ptrs.data(), batches.size(), xy.data(), inf.data()), "zg_msm_g1_batch_sharded");
        std::vector<AffinePoint> out;
        for (size_t i = 0; i < batches.size(); i++) out.push_back(unpack_point(&xy[8 * i], inf[i]));
        return out;
    }

private:
    zg_sbases_t h_ = nullptr;
    size_t n_;
};

struct ParallelMSM {  // :572-680 — contiguous chunks of ceil(n / T), one partial per worker, serial combine: one worker = one GPU
    static AffinePoint compute(const std::vector<AffinePoint> &bases, const std::vector<Fr> &scalars, size_t /*num_threads*/) {
        if (bases.size() != scalars.size()) throw std::invalid_argument("ParallelMSM.compute: bases.len != scalars.len");
        if (bases.empty()) return AffinePoint::identity();
        zg_msm_config cfg{0, 0, 1};  // a one-shot slice: no precompute table
        ShardedDeviceBases d(bases, &cfg);
        return d.msm(scalars.data(), scalars.size());
    }
};

struct ParallelBatchMSM {  // :683-748 — k vectors, k partials per GPU, one exchange
    static std::vector<AffinePoint> compute(const std::vector<AffinePoint> &bases, const std::vector<std::vector<Fr>> &batches) {
        if (batches.empty()) return {};
        zg_msm_config cfg{0, 0, 1};
        ShardedDeviceBases d(bases, &cfg);
        return d.msmBatch(batches, batches[0].size());
    }
};

}  // namespace zolt
