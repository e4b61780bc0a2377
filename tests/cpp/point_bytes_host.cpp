// point_bytes_host.cpp — the record decoders as ONE lane of the device runs them (zolt_amd/csrc/point_bytes.hip.h), on the CPU: the same
// header, the same functions, compiled for the host. tests/test_point_bytes_model.py builds it with
//     hipcc -x hip --offload-host-only -std=c++17 -O1 -I zolt_amd/csrc tests/cpp/point_bytes_host.cpp
// once as it is and once with -fsanitize=address,undefined, and holds it to tests/point_bytes_model.py. The function qualifiers are the
// only things replaced.
//
// stdin:  "<group 1|2> <encoding> <flags> <n>\n" then n records of the encoding's size, binary.
// stdout: one line per record: "<status> <identity flag> <8 or 16 words of xy, hex>", status 0 = ok, 1 = not on the curve, 2 = no root.
#define ZG_DEV __host__ __device__ inline
#define ZG_DEV_CALL static __host__ __device__ __attribute__((noinline))
#include <stdio.h>
#include <string.h>

#include <vector>

#include "point_bytes.hip.h"

template <class G>
static int run(unsigned encoding, unsigned flags, unsigned long n) {
    const size_t rec = zg::pb_record_bytes(G::COORDS, encoding);
    std::vector<uint4> in(n * rec / 16 + 1), xy(G::WORDS / 2);  // 16-byte aligned: the record loads and the element stores are vector accesses
    if (fread(in.data(), rec, n, stdin) != n) {
        fprintf(stderr, "point_bytes_host: short input\n");
        return 2;
    }
    for (unsigned long i = 0; i < n; i++) {
        zg::AffineT<typename G::F> p;
        bool inf = false;
        const uint4 *at = in.data() + i * rec / 16;
        const int status = encoding == ZG_POINT_BYTES_ARK_COMPRESSED ? zg::pb_decompress<G>(at, p, inf)
                                                                     : zg::pb_decode<G>(at, encoding, (flags & ZG_POINT_BYTES_CHECK) != 0, p, inf);
        zg::affine_store(xy.data(), p);
        printf("%d %d", status, inf ? 1 : 0);
        const uint64_t *w = reinterpret_cast<const uint64_t *>(xy.data());
        for (int k = 0; k < G::WORDS; k++) printf(" %016llx", (unsigned long long)w[k]);
        printf("\n");
    }
    return 0;
}

int main() {
    unsigned group = 0, encoding = 99, flags = 0;
    unsigned long n = 0;
    if (scanf("%u %u %u %lu", &group, &encoding, &flags, &n) != 4 || fgetc(stdin) != '\n' || group < 1 || group > 2 || encoding > ZG_POINT_BYTES_ARK_COMPRESSED ||
        n == 0 || n > (1ul << 16)) {
        fprintf(stderr, "point_bytes_host: bad header\n");
        return 2;
    }
    return group == 1 ? run<zg::PbG1>(encoding, flags, n) : run<zg::PbG2>(encoding, flags, n);
}
