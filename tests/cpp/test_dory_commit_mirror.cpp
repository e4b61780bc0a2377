// test_dory_commit_mirror.cpp — zolt::Dory::setup and zolt::Dory::batchCommit (zolt_amd/host/msm.hpp) over libzolt_gpu.so for one fixed
// input: prints two generators of setup(6) and the three commitments as hex words. tests/test_gpu_dory_commit.py builds and runs it and
// compares the lines with the Python mirror's words for the same input.
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

static void words(const char *name, const uint64_t *w, int n) {
    std::printf("%s", name);
    for (int i = 0; i < n; i++) std::printf(" %llx", (unsigned long long)w[i]);
    std::printf("\n");
}

int main() {
    const Dory::SetupParams params = Dory::setup(6);
    if (params.sigma != 3 || params.nu != 3 || params.g1_vec.size() != 8 || params.g2_vec.size() != 8) {
        std::printf("FAIL: setup(6) layout\n");
        return 1;
    }
    uint64_t g[8];
    std::memcpy(g, params.g1_vec[0].x.limbs, 32);
    std::memcpy(g + 4, params.g1_vec[0].y.limbs, 32);
    words("g1_0", g, 8);
    words("g2_7", params.g2_vec[7].xy, 16);
    // evals[i] = 1000 + 17 i; words[i] = 3 i * 2^40 + i, every third negated; column[i] = i * 0x9e3779b97f4a7c15 mod 2^64, its top nibble
    const size_t n = 64;
    std::vector<Fr> evals;
    std::vector<uint64_t> w64, col;
    std::vector<uint8_t> signs;
    for (size_t i = 0; i < n; i++) {
        evals.push_back(Fr::fromU64(1000 + 17 * i));
        w64.push_back((uint64_t(3 * i) << 40) + i);
        signs.push_back(i % 3 == 0 ? 1 : 0);
        col.push_back(uint64_t(i) * 0x9e3779b97f4a7c15ULL);
    }
    const Dory::Key key(params);
    std::vector<std::vector<AffinePoint>> rows;
    const std::vector<Dory::GT> gt = Dory::batchCommit(key, {{ZG_DORY_POLY_FR, reinterpret_cast<const uint64_t *>(evals.data()), n},
                                                              {ZG_DORY_POLY_U64, w64.data(), n, signs.data()},
                                                              {ZG_DORY_POLY_CHUNK64, col.data(), n, nullptr, 60, 4}}, &rows);
    if (gt.size() != 3 || rows.size() != 3 || rows[0].size() != 8 || rows[2].size() != 8) {
        std::printf("FAIL: batchCommit shapes\n");
        return 1;
    }
    for (int j = 0; j < 3; j++) {
        char name[16];
        std::snprintf(name, sizeof name, "gt_%d", j);
        words(name, gt[j].data(), 48);
    }
    return 0;
}
