// test_dory_open_key_mirror.cpp — zolt::Dory::open (zolt_amd/host/msm.hpp) over libzolt_gpu.so on the call the reference's prover makes
// when it serialises a proof (src/zkvm/mod.zig:1471-1492): open(setup(9), bytecode_evals, point) with the bytes of the program given as
// hex in argv[1], zero-padded to 128 evaluations, and point[i] = (i + 1) * 12345. Prints the arkworks bytes as hex ("proof <hex>");
// tests/test_gpu_dory_open_key.py builds and runs it and compares the line with tests/golden/dory_open_captured.bin.
#include <cstdio>
#include <cstring>

#include "../../zolt_amd/host/zolt_host.hpp"

using namespace zolt;

int main(int argc, char **argv) {
    if (argc != 2 || std::strlen(argv[1]) % 2) {
        std::printf("usage: test_dory_open_key_mirror <program bytes as hex>\n");
        return 2;
    }
    std::vector<Fr> evals, point;
    for (const char *p = argv[1]; *p; p += 2) {
        unsigned byte = 0;
        if (std::sscanf(p, "%2x", &byte) != 1) return 2;
        evals.push_back(Fr::fromU64(byte));
    }
    evals.resize(128, Fr::zero());
    for (uint64_t i = 0; i < 9; i++) point.push_back(Fr::fromU64(i + 1).mul(Fr::fromU64(12345)));
    const Dory::SetupParams params = Dory::setup(9);
    std::vector<uint8_t> bytes;
    {
        const Dory::Key key(params);
        const DoryProof proof = Dory::open(key, params, evals, point);
        if (proof.nu != 4 || proof.sigma != 5 || proof.first_messages.size() != 5 || proof.second_messages.size() != 5) {
            std::printf("FAIL: nu = %u, sigma = %u\n", proof.nu, proof.sigma);
            return 1;
        }
        bytes = proof.toArkBytes();
    }
    std::printf("proof ");
    for (uint8_t b : bytes) std::printf("%02x", b);
    std::printf("\n");
    return 0;
}
