// test_g2_mirror.cpp — the G2 side of the C++ host mirror (zolt_amd/host/msm.hpp: G2Point, Dory::msmG2 and one reduce-and-fold step)
// over libzolt_gpu.so. Self-checking through group identities; exit code 0 = all passed. Built and run by tests/test_gpu_g2.py.
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

static int g_failed = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

int main() {
    const G2Point g = G2Point::generator();
    // the cases G2Point.add distinguishes (src/field/pairing.zig:839-875)
    EXPECT(g.add(G2Point::identity()).eql(g) && G2Point::identity().add(g).eql(g));
    EXPECT(g.scalarMul(Fr::zero()).isIdentity() && G2Point::identity().scalarMul(Fr::fromU64(7)).isIdentity());
    EXPECT(g.add(g).eql(g.scalarMul(Fr::fromU64(2))));
    Fr minus_one = Fr::zero().sub(Fr::one());
    EXPECT(g.add(g.scalarMul(minus_one)).isIdentity());
    G2Point id = g.add(g.scalarMul(minus_one));
    EXPECT(std::memcmp(id.xy, G2Point::identity().xy, 128) == 0);

    // msmG2 (dory.zig:693-703) on bases k_i * G: the closed form (sum s_i k_i) * G and the literal loop
    const size_t n = 37;
    std::vector<Fr> k, s;
    Fr dot = Fr::zero();
    for (size_t i = 0; i < n; i++) {
        k.push_back(Fr::fromU64(3 * i + 1));
        s.push_back(Fr::fromU64(0x9e3779b97f4a7c15ULL * (i + 1)).mul(Fr::fromU64(0xbf58476d1ce4e5b9ULL + i)));
        dot = dot.add(k[i].mul(s[i]));
    }
    std::vector<G2Point> bases = Dory::generateG2Points(k);
    EXPECT(bases[0].eql(g) && bases[1].eql(g.scalarMul(Fr::fromU64(4))));
    bases[5] = G2Point::identity();  // an identity entry contributes nothing
    dot = dot.sub(k[5].mul(s[5]));
    G2Point got = Dory::msmG2(bases, s);
    EXPECT(got.eql(g.scalarMul(dot)) && !got.isIdentity());
    G2Point loop = G2Point::identity();
    for (size_t i = 0; i < n; i++) loop = loop.add(bases[i].scalarMul(s[i]));
    EXPECT(got.eql(loop));
    EXPECT(Dory::msmG2({}, {}).isIdentity());

    // one reduce-and-fold step (dory.zig:1578-1632) on 8-entry vectors, against per-element scalarMul + add
    const size_t len = 8;
    std::vector<Fr> hk, vv, s1, s2;
    for (size_t i = 0; i < len; i++) {
        hk.push_back(Fr::fromU64(1000 + 17 * i));
        s1.push_back(Fr::fromU64(5 + i).mul(Fr::fromU64(0x94d049bb133111ebULL)));
        s2.push_back(Fr::fromU64(11 + i));
    }
    for (size_t i = 0; i < 6; i++) vv.push_back(Fr::fromU64(77 + i * i));
    std::vector<G2Point> g2_vec = Dory::generateG2Points(hk);
    std::vector<G2Point> v2 = Dory::initV2(g2_vec[0], vv, len);
    EXPECT(v2.size() == len && v2[6].isIdentity() && v2[7].isIdentity() && v2[1].eql(g2_vec[0].scalarMul(vv[1])));
    std::vector<AffinePoint> g1_vec, v1;
    for (size_t i = 0; i < len; i++) {
        g1_vec.push_back(MSM::scalarMul(AffinePoint::generator(), Fr::fromU64(i + 2)));
        v1.push_back(i < 5 ? MSM::scalarMul(AffinePoint::generator(), Fr::fromU64(50 + i)) : AffinePoint::identity());
    }
    const Fr beta = Fr::fromU64(0x1234567).mul(Fr::fromU64(0xfedcba987ULL)), alpha = Fr::fromU64(0xabcdef).mul(Fr::fromU64(0x13579bdf2468ULL));
    Fr beta_inv, alpha_inv;
    EXPECT(beta.inverse(beta_inv) && alpha.inverse(alpha_inv));
    std::vector<AffinePoint> w1 = v1;
    std::vector<G2Point> w2 = v2;
    std::vector<Fr> t1 = s1, t2 = s2;
    Dory::applyFirstChallenge(w1, w2, g1_vec, g2_vec, beta, beta_inv);
    for (size_t i = 0; i < len; i++) {
        EXPECT(w1[i].eql(v1[i].add(MSM::scalarMul(g1_vec[i], beta))));
        EXPECT(w2[i].eql(v2[i].add(g2_vec[i].scalarMul(beta_inv))));
    }
    std::vector<AffinePoint> f1 = w1;
    std::vector<G2Point> f2 = w2;
    Dory::foldVectors(f1, f2, t1, t2, alpha, alpha_inv);
    EXPECT(f1.size() == len / 2 && f2.size() == len / 2 && t1.size() == len / 2 && t2.size() == len / 2);
    for (size_t i = 0; i < len / 2; i++) {
        EXPECT(f1[i].eql(MSM::scalarMul(w1[i], alpha).add(w1[i + len / 2])));
        EXPECT(f2[i].eql(w2[i].scalarMul(alpha_inv).add(w2[i + len / 2])));
        EXPECT(t1[i].eql(alpha.mul(s1[i]).add(s1[i + len / 2])) && t2[i].eql(alpha_inv.mul(s2[i]).add(s2[i + len / 2])));
    }
    std::printf("%d failures\n", g_failed);
    return g_failed ? 1 : 0;
}
