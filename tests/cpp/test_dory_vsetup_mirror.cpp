// test_dory_vsetup_mirror.cpp — zolt::DoryVerifierSetup (zolt_amd/host/msm.hpp) over libzolt_gpu.so at the reference's own test shape
// (src/zkvm/preprocessing.zig:1187-1216: setup(4), four generators a side, three levels): prints the serialised bytes from host points
// and over a resident key as hex. tests/test_gpu_dory_vsetup.py builds and runs it and compares the lines with the Python mirror's bytes.
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

static void hex(const char *name, const std::vector<uint8_t> &b) {
    std::printf("%s ", name);
    for (uint8_t v : b) std::printf("%02x", v);
    std::printf("\n");
}

int main() {
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
