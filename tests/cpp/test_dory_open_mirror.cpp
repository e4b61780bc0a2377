// test_dory_open_mirror.cpp — zolt::Dory::openWithTranscript (zolt_amd/host/msm.hpp) with the Blake2b transcript (sumcheck.hpp) over
// libzolt_gpu.so, for one fixed input: prints the proof bytes as hex ("proof <hex>"). tests/test_gpu_dory_open.py builds and runs it and
// compares the line with the Python mirror's bytes for the same input.
#include <cstdio>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

int main() {
    // nu = 2, sigma = 3, g1_vec[i] = (i + 1) G, g2_vec[i] = (7 i + 3) H, evals[j] = 1000 + 17 j, point[k] = 5 + 3 k
    const unsigned nu = 2, sigma = 3;
    const size_t n = size_t(1) << sigma;
    std::vector<AffinePoint> g1_vec;
    std::vector<Fr> hk, evals, point;
    for (size_t i = 0; i < n; i++) {
        g1_vec.push_back(MSM::scalarMul(AffinePoint::generator(), Fr::fromU64(i + 1)));
        hk.push_back(Fr::fromU64(7 * i + 3));
    }
    const std::vector<G2Point> g2_vec = Dory::generateG2Points(hk);
    for (size_t j = 0; j < (size_t(1) << (nu + sigma)); j++) evals.push_back(Fr::fromU64(1000 + 17 * j));
    for (size_t k = 0; k < nu + sigma; k++) point.push_back(Fr::fromU64(5 + 3 * k));
    Blake2bTranscript transcript("Jolt");
    const DoryProof proof = Dory::openWithTranscript(g1_vec, g2_vec, nu, sigma, evals, point, nullptr, transcript);
    const std::vector<uint8_t> bytes = proof.toBytes();
    if (bytes.size() != 800 + 4 + sigma * (1632 + 960) + 96 + 8 || proof.first_messages.size() != sigma) {
        std::printf("FAIL: %zu proof bytes\n", bytes.size());
        return 1;
    }
    // the wire forms on values whose answers are known: the identity, the generator (y = 2 is the smaller of y and -y), its negation
    const auto id = compressG1(AffinePoint::identity());
    const auto gen = compressG1(AffinePoint::generator());
    bool ok = id[31] == 0x40 && gen[0] == 1 && gen[31] == 0;
    for (int i = 0; i < 31; i++) ok = ok && id[i] == 0 && (i == 0 || gen[i] == 0);
    const AffinePoint neg = MSM::scalarMul(AffinePoint::generator(), Fr::zero().sub(Fr::one()));
    ok = ok && compressG1(neg)[0] == 1 && compressG1(neg)[31] == 0x80;
    if (!ok) {
        std::printf("FAIL: compressG1\n");
        return 1;
    }
    std::printf("proof ");
    for (uint8_t b : bytes) std::printf("%02x", b);
    std::printf("\n");
    return 0;
}
