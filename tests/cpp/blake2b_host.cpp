// blake2b_host.cpp — the Fiat-Shamir lane functions (zolt_amd/csrc/blake2b.hip.h) run on the CPU: the same header, compiled
// for the host. tests/test_device_transcript_model.py builds it with
//     hipcc -x hip --offload-host-only -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/blake2b_host.cpp
// once as it is and once with -fsanitize=address,undefined (a stand-alone program: nothing here is loaded into another process). The
// function qualifiers are the only things replaced.
//
// stdin: "<op> <n>\n", then binary.
//   op 0  n + 1 u64 offsets, then offsets[n] message bytes                    -> n digests of 32 bytes
//   op 1  n records { u32 code, u32 len, len bytes }                          -> per record 32 bytes of result (zero when the operation has
//         code 0 init(label) 1 import(32 state bytes, u32 n_rounds)              none), the 32 state bytes, n_rounds as u64
//              2 appendBytes 3 appendMessage 4 appendU64(8 bytes LE)
//              5 appendScalar(4 u64) 6 challengeScalar 7 challengeScalarFull
//   op 2  an FsRunState, 5 u64 of transcript state, u32 setup (0 none, 1 given coefficients, 2 sampled), then n rounds of 8 x 16 u64 sums
//         -> after the setup: the FsRunState and the 5 state words; per round: 16 u64 of log, the FsRunState, the 5 state words
//   op 3  n records { claim, c0, c2, c3, r } of 4 u64 each                    -> n next claims (fs_next_claim)
#define ZG_DEV __host__ __device__ inline
#define ZG_DEV_CALL static __host__ __device__ __attribute__((noinline))
#include <stdio.h>
#include <string.h>

#include <vector>

#include "blake2b.hip.h"

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static bool wr(const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, stdout) == n; }

static int op_hash(unsigned long n) {
    std::vector<uint64_t> off(n + 1);
    if (!rd(off.data(), 8 * (n + 1)) || off[0] != 0) return 2;
    for (unsigned long i = 0; i < n; i++)
        if (off[i] > off[i + 1]) return 2;
    if (off[n] > (1ul << 24)) return 2;
    std::vector<uint8_t> bytes(off[n] + 1);
    if (!rd(bytes.data(), off[n])) return 2;
    for (unsigned long i = 0; i < n; i++) {
        uint64_t m[16], out[4];
        zg::B2b b;
        zg::b2b_init(b, m);
        zg::b2b_bytes(b, bytes.data() + off[i], off[i + 1] - off[i]);
        zg::b2b_final(b, out);
        if (!wr(out, 32)) return 1;
    }
    return 0;
}

static int op_script(unsigned long n) {
    uint64_t m[16], st[zg::FS_STATE_WORDS] = {0, 0, 0, 0, 0};
    zg::FsT t = zg::fs_load(st, m);
    for (unsigned long i = 0; i < n; i++) {
        uint32_t hd[2];
        if (!rd(hd, 8) || hd[1] > (1u << 20)) return 2;
        std::vector<uint8_t> p(hd[1] + 8);
        if (!rd(p.data(), hd[1])) return 2;
        uint64_t res[4] = {0, 0, 0, 0}, w[4];
        switch (hd[0]) {
            case 0: zg::fs_init(t, p.data(), hd[1]); break;
            case 1:
                memcpy(t.s, p.data(), 32);
                memcpy(&t.n_rounds, p.data() + 32, 4);
                break;
            case 2: zg::fs_append_bytes(t, p.data(), hd[1]); break;
            case 3: zg::fs_append_message(t, reinterpret_cast<const char *>(p.data()), hd[1]); break;
            case 4:
                memcpy(w, p.data(), 8);
                zg::fs_append_u64(t, w[0]);
                break;
            case 5:
                memcpy(w, p.data(), 32);
                zg::fs_append_scalar(t, zg::fs_ld(w));
                break;
            case 6: zg::fs_st(res, zg::fs_challenge_scalar(t)); break;
            case 7: zg::fs_st(res, zg::fs_challenge_scalar_full(t)); break;
            default: return 2;
        }
        const uint64_t nr = t.n_rounds;
        if (!wr(res, 32) || !wr(t.s, 32) || !wr(&nr, 8)) return 1;
    }
    return 0;
}

static int op_rounds(unsigned long n) {
    zg::FsRunState S;
    uint64_t m[16], st[zg::FS_STATE_WORDS];
    uint32_t setup = 0;
    if (!rd(&S, sizeof(S)) || !rd(st, sizeof(st)) || !rd(&setup, 4) || S.k < 1 || S.k > (uint32_t)zg::FS_MAX_INST) return 2;
    zg::FsT t = zg::fs_load(st, m);
    if (setup) zg::fs_setup_batching(S, t, setup == 2);
    zg::fs_store(t, st);
    if (!wr(&S, sizeof(S)) || !wr(st, sizeof(st))) return 1;
    for (unsigned long j = 0; j < n; j++) {
        uint64_t log16[16];
        if (!rd(S.sums, sizeof(S.sums))) return 2;
        zg::fs_round_step(S, t, log16);
        zg::fs_store(t, st);
        if (!wr(log16, sizeof(log16)) || !wr(&S, sizeof(S)) || !wr(st, sizeof(st))) return 1;
    }
    return 0;
}

static int op_next_claim(unsigned long n) {
    for (unsigned long i = 0; i < n; i++) {
        uint64_t w[20], out[4];
        if (!rd(w, sizeof(w))) return 2;
        const zg::FsFr c[4] = {zg::fs_ld(w + 4), zg::FsFr::zero(), zg::fs_ld(w + 8), zg::fs_ld(w + 12)};
        zg::fs_st(out, zg::fs_next_claim(zg::fs_ld(w), c, zg::fs_ld(w + 16)));
        if (!wr(out, 32)) return 1;
    }
    return 0;
}

int main() {
    int op = -1;
    unsigned long n = 0;
    if (scanf("%d %lu", &op, &n) != 2 || fgetc(stdin) != '\n' || op < 0 || op > 3 || n > (1ul << 16)) {
        fprintf(stderr, "blake2b_host: bad header (op 0..3, n <= 2^16)\n");
        return 2;
    }
    const int rc = op == 0 ? op_hash(n) : op == 1 ? op_script(n) : op == 2 ? op_rounds(n) : op_next_claim(n);
    if (rc == 2) fprintf(stderr, "blake2b_host: short or malformed input\n");
    return rc;
}
