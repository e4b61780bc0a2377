// point_bytes.hip — "Points from bytes" (include/zolt_gpu.h): the byte formats of key, proof and preprocessing files decoded on the
// device, one lane per record (point_bytes.hip.h holds the encodings, the lane functions and the deviations from the reference).
//
// Two kernels per group. The decode kernel (BE / LE / ARK) is four or two Montgomery conversions and, when asked, the on-curve check:
// it launches in the workgroups of points.hip (256 lanes for G1, 64 for G2). The decompress kernel is one square root in Fp (~330 Fp
// products) or in Fp2 (~700 and an inversion) per lane and launches in workgroups of 64, so that a short vector — a proof's points, a
// small key — spreads over as many SIMDs as it has waves.
// A bad record does not stop the launch: every lane writes its point, each wave takes the smallest bad index of its lanes from a ballot
// and issues at most one atomicMin on a 64-bit word, which the host reads once before it fetches or builds anything. The minimum over
// all waves does not depend on the order they ran in.
#include <string>

#include "common.hip.h"
#include "point_bytes.hip.h"

namespace zg {

static constexpr unsigned long long PB_NONE = ~0ull;  // the verdict word when every record is good

// lane `bad` of the wave with the smallest index wins the wave's one atomicMin (lanes are in index order)
ZG_DEV void pb_verdict(bool bad, size_t i, unsigned long long *first_bad) {
    const unsigned long long votes = __ballot(bad);
    if (votes == 0) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll(votes) - 1)) atomicMin(first_bad, (unsigned long long)i);
}

template <class G>
__global__ void __launch_bounds__(G::BLOCK) point_bytes_decode_kernel(const uint4 *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy, uint8_t *out_inf,
                                                                      unsigned long long *first_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        AffineT<typename G::F> p;
        bool inf;
        bad = pb_decode<G>(bytes + (size_t)(G::COORDS * 2) * i, encoding, (flags & ZG_POINT_BYTES_CHECK) != 0, p, inf) != PB_OK;
        affine_store(out_xy + G::WORDS * i, p);
        out_inf[i] = inf ? 1 : 0;
    }
    pb_verdict(bad, i, first_bad);
}

template <class G>
__global__ void __launch_bounds__(64) point_bytes_decompress_kernel(const uint4 *bytes, size_t n, uint64_t *out_xy, uint8_t *out_inf, unsigned long long *first_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        AffineT<typename G::F> p;
        bool inf;
        bad = pb_decompress<G>(bytes + (size_t)G::COORDS * i, p, inf) != PB_OK;
        affine_store(out_xy + G::WORDS * i, p);
        out_inf[i] = inf ? 1 : 0;
    }
    pb_verdict(bad, i, first_bad);
}

static constexpr size_t PB_MAX = (size_t)1 << 28;

static int pb_validate(const char *who, const void *bytes, size_t n, uint32_t encoding, uint32_t flags) {
    if (encoding > ZG_POINT_BYTES_ARK_COMPRESSED) return invalid(who, "unknown encoding");
    if (flags & ~ZG_POINT_BYTES_CHECK) return invalid(who, "unknown flag bits");
    if (n > PB_MAX) return invalid(who, "more than 2^28 records");
    if (n && !bytes) return invalid(who, "null data");
    return ZG_OK;
}

// n > 0 records of the host's cross once and are decoded into d_xy / d_inf on sg.st; *d_bad is the verdict word
template <class G>
static void pb_enqueue(Staging &sg, const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *d_xy, uint8_t *d_inf, unsigned long long *d_bad) {
    const uint4 *d_bytes = reinterpret_cast<const uint4 *>(sg.in(bytes, n * pb_record_bytes(G::COORDS, encoding)));
    if (!sg.ok()) return;
    if (!ZG_STAGE(sg, hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), sg.st))) return;
    if (encoding == ZG_POINT_BYTES_ARK_COMPRESSED)
        hipLaunchKernelGGL(point_bytes_decompress_kernel<G>, dim3(div_up(n, 64)), dim3(64), 0, sg.st, d_bytes, n, d_xy, d_inf, d_bad);
    else
        hipLaunchKernelGGL(point_bytes_decode_kernel<G>, dim3(div_up(n, G::BLOCK)), dim3(G::BLOCK), 0, sg.st, d_bytes, n, encoding, flags, d_xy, d_inf, d_bad);
    sg.launched();
}

static int pb_bad_record(const char *who, size_t index, uint32_t encoding) {
    return invalid(std::string(who) + ": record " + std::to_string(index) + ": " + (encoding == ZG_POINT_BYTES_ARK_COMPRESSED ? "DecompressionFailed" : "PointNotOnCurve"));
}

template <class G>
static int points_from_bytes(const char *who, const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy, uint8_t *out_inf, size_t *first_bad) {
    ZG_TRY(pb_validate(who, bytes, n, encoding, flags));
    if (n && !out_xy) return invalid(who, "no output");
    ZG_INIT();
    if (n == 0) {
        if (first_bad) *first_bad = 0;
        return ZG_OK;
    }
    Staging sg(lib_stream());
    uint64_t *d_xy = sg.out<uint64_t>(n * G::WORDS * 8);
    uint8_t *d_inf = sg.out<uint8_t>(n);
    unsigned long long *d_bad = sg.out<unsigned long long>(sizeof(unsigned long long)), h_bad = PB_NONE;
    pb_enqueue<G>(sg, bytes, n, encoding, flags, d_xy, d_inf, d_bad);
    sg.fetch(&h_bad, d_bad, sizeof h_bad);
    if (sg.ok()) ZG_STAGE(sg, hipStreamSynchronize(sg.st));  // the verdict before anything reaches the caller's memory
    if (!sg.ok()) return sg.finish();
    if (h_bad != PB_NONE) {
        if (first_bad) *first_bad = (size_t)h_bad;
        return pb_bad_record(who, (size_t)h_bad, encoding);
    }
    sg.fetch(out_xy, d_xy, n * G::WORDS * 8);
    sg.fetch(out_inf, d_inf, n);
    ZG_TRY(sg.finish());
    if (first_bad) *first_bad = n;
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_g1_points_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy, uint8_t *out_inf, size_t *first_bad) {
    return points_from_bytes<PbG1>("zg_g1_points_from_bytes", bytes, n, encoding, flags, out_xy, out_inf, first_bad);
}
int zg_g2_points_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy, uint8_t *out_inf, size_t *first_bad) {
    return points_from_bytes<PbG2>("zg_g2_points_from_bytes", bytes, n, encoding, flags, out_xy, out_inf, first_bad);
}

int zg_g1_bases_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, const zg_msm_config *cfg, zg_bases_t *out, size_t *first_bad) {
    const char *who = "zg_g1_bases_from_bytes";
    if (!out) return invalid(who, "no handle pointer");
    *out = nullptr;
    ZG_TRY(pb_validate(who, bytes, n, encoding, flags));
    if (n == 0) return invalid(who, "no records");
    ZG_INIT();
    Staging sg(lib_stream());  // the decoded points go back to the pool only after the table build that reads them has finished
    uint64_t *d_xy = sg.out<uint64_t>(n * 64);
    uint8_t *d_inf = sg.out<uint8_t>(n);
    unsigned long long *d_bad = sg.out<unsigned long long>(sizeof(unsigned long long)), h_bad = PB_NONE;
    pb_enqueue<PbG1>(sg, bytes, n, encoding, flags, d_xy, d_inf, d_bad);
    sg.fetch(&h_bad, d_bad, sizeof h_bad);
    if (sg.ok()) ZG_STAGE(sg, hipStreamSynchronize(sg.st));
    if (!sg.ok()) return sg.finish();
    if (h_bad != PB_NONE) {
        if (first_bad) *first_bad = (size_t)h_bad;
        return pb_bad_record(who, (size_t)h_bad, encoding);
    }
    sg.adopt(zg_g1_bases_upload_dev(d_xy, d_inf, n, cfg, sg.st, out));
    ZG_TRY(sg.finish());
    if (first_bad) *first_bad = n;
    return ZG_OK;
}

int zg_dory_key_from_bytes(const uint8_t *g1_bytes, size_t n_g1, uint32_t g1_encoding, const uint8_t *g2_bytes, size_t n_g2, uint32_t g2_encoding, uint32_t flags,
                           zg_dory_key_t *out, size_t *first_bad) {
    const char *who = "zg_dory_key_from_bytes";
    if (!out) return invalid(who, "no key pointer");
    *out = nullptr;
    ZG_TRY(pb_validate(who, g1_bytes, n_g1, g1_encoding, flags));
    ZG_TRY(pb_validate(who, g2_bytes, n_g2, g2_encoding, flags));
    if (n_g1 < 1 || n_g1 > ((size_t)1 << 16) || n_g2 > ((size_t)1 << 24)) return invalid(who, "1 <= n_g1 <= 2^16 and n_g2 <= 2^24 required");
    ZG_INIT();
    zg_dory_key_s *key = nullptr;
    ZG_TRY(dory_key_alloc(n_g1, n_g2, &key));
    int rc = ZG_OK;
    {
        Staging sg(lib_stream());
        unsigned long long *d_bad = sg.out<unsigned long long>(2 * sizeof(unsigned long long)), h_bad[2] = {PB_NONE, PB_NONE};
        uint8_t g2_0_inf = 0;
        pb_enqueue<PbG1>(sg, g1_bytes, n_g1, g1_encoding, flags, key->g1, key->g1_inf, d_bad);
        if (n_g2) pb_enqueue<PbG2>(sg, g2_bytes, n_g2, g2_encoding, flags, key->g2, key->g2_inf, d_bad + 1);
        sg.fetch(h_bad, d_bad, n_g2 ? sizeof h_bad : sizeof h_bad[0]);
        if (n_g2) sg.fetch(&g2_0_inf, key->g2_inf, 1);
        if (sg.ok()) ZG_STAGE(sg, hipStreamSynchronize(sg.st));
        if (sg.ok() && (h_bad[0] != PB_NONE || h_bad[1] != PB_NONE)) {
            const bool in_g1 = h_bad[0] != PB_NONE;
            const size_t at = in_g1 ? (size_t)h_bad[0] : n_g1 + (size_t)h_bad[1];
            if (first_bad) *first_bad = at;
            rc = pb_bad_record(who, at, in_g1 ? g1_encoding : g2_encoding);
        } else if (sg.ok()) {
            key->g2_0_inf = g2_0_inf != 0;
            sg.adopt(dory_key_tables(key, sg));
        }
        const int rc2 = sg.finish();
        if (rc == ZG_OK) rc = rc2;
    }
    if (rc != ZG_OK) {
        dory_key_drop(key);
        return rc;
    }
    *out = key;
    if (first_bad) *first_bad = n_g1 + n_g2;
    return ZG_OK;
}

}  // extern "C"
