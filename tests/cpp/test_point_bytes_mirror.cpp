// test_point_bytes_mirror.cpp — the C++ mirror of "Points from bytes" (zolt_amd/host/wire.hpp: srsFromRaw, srsFromPtau, decompressG1 /
// decompressG2; zolt_amd/host/msm.hpp: Dory::loadFromFile) over libzolt_gpu.so. Arguments: a raw SRS file, a ptau file, a Jolt Dory SRS
// file, a file of compressed G1 records, a file of compressed G2 records. Prints one line of hex per file — what was decoded, as
// Montgomery words, and what the handles compute — which tests/test_gpu_point_bytes.py compares with the Python mirror's.
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> out;
    FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    uint8_t buf[4096];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
    std::fclose(f);
    return out;
}
static void words(const uint64_t *w, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%016llx", (unsigned long long)w[i]);
}
static void point(const AffinePoint &p) {
    words(p.x.limbs, 4);
    words(p.y.limbs, 4);
    std::printf("%d", p.infinity ? 1 : 0);
}
static std::vector<uint64_t> counting(size_t n) {
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = 3 * i + 1;
    return v;
}

int main(int argc, char **argv) {
    if (argc != 6) {
        std::printf("FAIL: five files expected\n");
        return 1;
    }
    try {
        {
            const wire::Srs srs = wire::srsFromRaw(slurp(argv[1]));
            std::printf("raw %zu ", srs.max_degree);
            point(srs.bases->msmU64(counting(srs.max_degree).data(), srs.max_degree));
            words(srs.tau_g2.xy, 16);
            point(srs.g1);
            words(srs.g2.xy, 16);
            std::printf("\n");
        }
        {
            const wire::PtauSrs p = wire::srsFromPtau(slurp(argv[2]));
            std::printf("ptau %u %u %zu ", p.power, p.ceremony_power, p.n_g1);
            point(p.bases->msmU64(counting(p.n_g1).data(), p.n_g1));
            words(p.powers_of_tau_g2.xy.data(), p.powers_of_tau_g2.xy.size());
            words(p.alpha_tau_g1.xy.data(), p.alpha_tau_g1.xy.size());
            words(p.beta_tau_g1.xy.data(), p.beta_tau_g1.xy.size());
            words(p.beta_g2.xy, 16);
            std::printf("\n");
        }
        {
            const Dory::LoadedKey k = Dory::loadFromFile(slurp(argv[3]));
            const std::vector<uint64_t> v = counting(size_t(1) << k.max_num_vars);
            const auto gt = Dory::batchCommit(*k.key, {Dory::Poly{ZG_DORY_POLY_U64, v.data(), v.size()}});
            std::printf("dory %u %u ", k.sigma, k.nu);
            words(gt[0].data(), 48);
            std::printf("\n");
        }
        {
            const wire::G1Points a = wire::decompressG1(slurp(argv[4]));
            const wire::G2Points b = wire::decompressG2(slurp(argv[5]));
            std::printf("points ");
            words(a.xy.data(), a.xy.size());
            words(b.xy.data(), b.xy.size());
            for (uint8_t f : a.inf) std::printf("%d", f);
            for (uint8_t f : b.inf) std::printf("%d", f);
            std::printf("\n");
        }
        // the error names
        std::vector<uint8_t> bad = slurp(argv[1]);
        bad[4 + 64 * 2 + 63] ^= 1;
        try {
            wire::srsFromRaw(bad);
            std::printf("FAIL: an off-curve record was accepted\n");
            return 1;
        } catch (const wire::SRSError &e) {
            std::printf("bad %s\n", e.what());
        }
        try {
            std::vector<uint8_t> d = slurp(argv[3]);
            d.resize(d.size() - 1);
            Dory::loadFromFile(d);
            std::printf("FAIL: a short Dory SRS was accepted\n");
            return 1;
        } catch (const Dory::SrsError &e) {
            std::printf("short %s\n", e.what());
        }
    } catch (const std::exception &e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
    return 0;
}
