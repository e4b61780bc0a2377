// blake2b_device_compile.hip — the Fiat-Shamir lane functions (zolt_amd/csrc/blake2b.hip.h) compiled for gfx950, and nothing more:
// tests/test_device_transcript_model.py builds this file with
//     hipcc --offload-arch=gfx950 --offload-device-only -std=c++17 -O3 -I zolt_amd/csrc -c tests/cpp/blake2b_device_compile.hip
// so that a change which only compiles for the host is caught. The kernels below name every entry of the header once; nothing launches
// them (the header is verified on the host only).
#include "blake2b.hip.h"

using namespace zg;

__global__ void __launch_bounds__(64) compile_transcript_ops(uint64_t *state, const uint8_t *bytes, uint32_t len, const uint64_t *scalars, uint64_t *out) {
    __shared__ u64 m[16];
    if (threadIdx.x != 0) return;
    FsT t = fs_load(state, m);
    fs_init(t, bytes, len);
    fs_append_bytes(t, bytes, len);
    fs_append_message(t, "UniPoly_begin", 13);
    fs_append_u64(t, len);
    fs_append_scalar(t, fs_ld(scalars));
    fs_st(out, fs_challenge_scalar(t));
    fs_st(out + 4, fs_challenge_scalar_full(t));
    fs_store(t, state);
}

__global__ void __launch_bounds__(64) compile_round_step(uint64_t *run, uint64_t *state, uint64_t *log16, int sample) {
    __shared__ u64 m[16];
    if (threadIdx.x != 0) return;
    FsT t = fs_load(state, m);
    FsRunState &S = *reinterpret_cast<FsRunState *>(run);
    if (sample >= 0) fs_setup_batching(S, t, sample != 0);
    fs_round_step(S, t, log16);
    fs_store(t, state);
}
