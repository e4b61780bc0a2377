// test_dory_vsetup_mirror.cpp — zolt::DoryVerifierSetup (zolt_amd/host/msm.hpp) over libzolt_gpu.so at the reference's own test shape
// (src/zkvm/preprocessing.zig:1187-1216: setup(4), four generators a side, three levels): prints the serialised bytes from host points
// and over a resident key as hex. tests/test_gpu_dory_vsetup.py builds and runs it and compares the lines with the Python mirror's bytes.
// With a file name as its argument — 24 u64 words, a G1 point (x, y) and a G2 point (x.c0, x.c1, y.c0, y.c1) in Montgomery limbs — it
// prints instead the serialised setup of that ONE generator pair (K = 0), from points and over a key, under each pairing engine
// (tests/test_gpu_dory_captured_setup.py: the pair is the reference's own g1_0, g2_0).
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

static void hex(const char *name, const std::vector<uint8_t> &b) {
    std::printf("%s ", name);
    for (uint8_t v : b) std::printf("%02x", v);
    std::printf("\n");
}

static int one_pair(const char *path) {
    uint64_t w[24];
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(w, 8, 24, f) != 24) {
        std::printf("FAIL: %s does not hold 24 words\n", path);
        return 1;
    }
    std::fclose(f);
    AffinePoint p;
    std::memcpy(p.x.limbs, w, 32);
    std::memcpy(p.y.limbs, w + 4, 32);
    p.infinity = false;
    G2Point q{};
    std::memcpy(q.xy, w + 8, 128);
    const std::vector<AffinePoint> g1_vec{p};
    const std::vector<G2Point> g2_vec{q};
    const struct { const char *points, *key; int engine; } runs[] = {{"lane_points", "lane_key", ZG_PAIRING_ENGINE_LANE},
                                                                   {"wave_points", "wave_key", ZG_PAIRING_ENGINE_WAVE}};
    for (const auto &r : runs) {
        const PairingEngine scope(r.engine);
        const DoryVerifierSetup a = DoryVerifierSetup::fromSRS(g1_vec, g2_vec);
        if (a.chi.size() != 1 || a.max_log_n != 0 || a.delta_1l[0] != DoryVerifierSetup::gtOne() || a.ht != a.chi[0]) {
            std::printf("FAIL: fromSRS shapes and copies at K = 0\n");
            return 1;
        }
        hex(r.points, a.serialize());
        const Dory::Key key(g1_vec, g2_vec);
        hex(r.key, DoryVerifierSetup::fromSRS(key, p, q).serialize());
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return one_pair(argv[1]);
    const Dory::SetupParams params = Dory::setup(4);
    if (params.g1_vec.size() != 4 || params.g2_vec.size() != 4) {
        std::printf("FAIL: setup(4) layout\n");
        return 1;
    }
    const DoryVerifierSetup a = DoryVerifierSetup::fromSRS(params);
    if (a.chi.size() != 3 || a.delta_1l.size() != 3 || a.delta_1r.size() != 3 || a.delta_2l.size() != 3 || a.delta_2r.size() != 3 || a.max_log_n != 4 ||
        a.delta_1l[0] != DoryVerifierSetup::gtOne() || a.delta_1r[0] != DoryVerifierSetup::gtOne() || a.delta_2r[0] != DoryVerifierSetup::gtOne() ||
        a.delta_1l[2] != a.chi[1] || a.delta_2l != a.delta_1l || a.ht != a.chi[0]) {
        std::printf("FAIL: fromSRS shapes and copies\n");
        return 1;
    }
    hex("points", a.serialize());
    const Dory::Key key(params);
    hex("key", DoryVerifierSetup::fromSRS(key, params.g1_vec[0], params.g2_vec[0]).serialize());
    // the identity encodings
    uint64_t xy[8] = {0};
    hex("id1", [&] { auto b = DoryVerifierSetup::serializeG1(xy, true); return std::vector<uint8_t>(b.begin(), b.end()); }());
    hex("id2", [&] { auto b = DoryVerifierSetup::serializeG2(G2Point::identity().xy, true); return std::vector<uint8_t>(b.begin(), b.end()); }());
    return 0;
}
