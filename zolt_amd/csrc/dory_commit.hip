// dory_commit.hip — DoryCommitmentScheme.commit (src/poly/commitment/dory.zig:989-1042) for all the polynomials of a proof at once, over
// a key that stays in HBM: both generator vectors, the digit table T[c][d] = d * g1_vec[c] (dory_commit.hip.h) and an MSM handle over
// g1_vec. Three kernels and a pair set of its own, then the pairing section's product and final exponentiation:
//   dory_commit_table_kernel    once per key: a lane per column, 254 mixed additions, one inversion, 255 affine rows
//   dory_commit_rowsum_kernel   the hot path: 2^lanes_log2 lanes per (virtual polynomial, row) stride the row's columns, gather the table row
//                               of every non-zero digit and add it in the MSM's lazy-limb law; a shuffle tree of complete additions joins them
//   dory_commit_finish_kernel   a lane per (polynomial, row): the sum of a chunk polynomial, or the Horner combine of a 64-bit polynomial's
//                               eight byte sums, to the affine record the MSM writes (one inversion per lane, all lanes at once)
//   DcRowPairs                  the pair set (pair_set.hip.h) of the (polynomial, row) of ALL polynomials: the row against g2_vec[row] of the
//                               key — (polynomial, row) comes from the pair index and the row offsets, which are pair_product_kernel's
//                               segment table as they are
// Montgomery Fr polynomials take the existing fused batch MSM into the same record array.
// Shape of the row sums, against the suggestion of a wave per row: the lanes of a row are 2^sigma / 16 (at most 64, at least 1), so a lane
// has 16 additions before the tree's log2(lanes) complete additions (14 products each against 10) instead of 2 at 128 columns; rows are
// so many (2^nu per virtual polynomial, ~58 of them in a proof of 2^20 cycles) that the launch fills the device without splitting a row further. The
// digits of polynomials that share a column are NOT decoded from one load: the 32 chunk polynomials of a column re-read 16 KB per row
// that the first of them left in L2, 16 bytes beside a 64-byte table row per addition.
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "common.hip.h"
#include "pair_set.hip.h"
#include "dory_commit.hip.h"

namespace zg {

__global__ void __launch_bounds__(64) dory_commit_table_kernel(const uint64_t *g1_xy, const uint8_t *g1_inf, uint32_t first, uint32_t count, char *table,
                                                               char *rec, char *pref) {
    const uint32_t li = blockIdx.x * 64 + threadIdx.x;
    if (li >= count) return;
    const uint32_t c = first + li;
    dc_table_column(affine_load(g1_xy + 8 * (size_t)c), g1_inf[c] != 0, table + 64 * (size_t)DC_DIGITS * c, rec + 144 * (size_t)li, 144 * (size_t)count,
                    pref + 48 * (size_t)li, 48 * (size_t)count);
}

// the last index i < n with off[i] <= x, for ascending off with off[0] <= x
template <class T, class Get>
ZG_DEV uint32_t dc_find(uint32_t n, T x, Get off) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// A wave belongs to one virtual polynomial (first_wave ascending; polynomials start on wave boundaries, so the 2^lanes_log2 lanes of a row
// never straddle waves). sums: 144-byte records, row g of virtual polynomial v at v.out + g.
__global__ void __launch_bounds__(256) dory_commit_rowsum_kernel(const char *table, const uint8_t *g1_inf, const DcVirt *virts, uint32_t n_virt, uint32_t waves,
                                                                 char *sums) {
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (wave >= waves) return;
    const DcVirt v = virts[dc_find(n_virt, wave, [&](uint32_t i) { return virts[i].first_wave; })];
    const uint32_t L = 1u << v.lanes_log2;
    const uint32_t g = (((wave - v.first_wave) << 6) + lane) >> v.lanes_log2;
    const bool live = g < v.rows;
    XYZZ29 val = live ? dc_lane_sum(table, g1_inf, v, g, lane & (L - 1), L) : xyzz29_identity();
#pragma unroll 1
    for (uint32_t s = 32; s >= 1; s >>= 1) {
        if (s < L) val = xyzz29_add(val, xyzz29_shfl_down(val, (int)s));  // L is the wave's: no divergence around the shuffle
    }
    if (live && (lane & (L - 1)) == 0) xyzz29_store(sums + 144 * ((size_t)v.out + g), val);
}

struct DcPoly {
    uint32_t n_virt;  // 0: the rows are written by the MSM; 1: a chunk polynomial; 8: the bytes of a 64-bit polynomial
    uint32_t rows;
    uint32_t sum0;    // the sum of virtual polynomial w, row r: sum0 + w * rows + r
};

__global__ void __launch_bounds__(64) dory_commit_finish_kernel(const DcPoly *polys, const size_t *row_off, uint32_t k, uint32_t total, const char *sums,
                                                                uint64_t *rows9) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= total) return;
    const uint32_t j = dc_find(k, (size_t)i, [&](uint32_t t) { return row_off[t]; });
    const DcPoly p = polys[j];
    if (p.n_virt == 0) return;
    const char *s = sums + 144 * ((size_t)p.sum0 + (i - (uint32_t)row_off[j]));
    dc_store_record(rows9 + 9 * (size_t)i, p.n_virt == 1 ? xyzz29_load(s) : dc_horner(s, 144 * (size_t)p.rows));
}

// pair i of the launch set = (row record i, g2_vec[i - row_off[j]]); a row past g2_vec is left out of the product (:1030): one. The
// record's flag is byte 0 of word 8.
struct DcRowPairs {
    const uint64_t *rows9;
    const size_t *row_off;
    uint32_t k;
    const uint64_t *g2_xy;
    const uint8_t *g2_inf;
    uint32_t n_g2;
    ZG_DEV PairOperands operator()(uint32_t i) const {
        const uint32_t j = dc_find(k, (size_t)i, [&](uint32_t t) { return row_off[t]; });
        const uint32_t row = i - (uint32_t)row_off[j];
        const uint64_t *rec = rows9 + 9 * (size_t)i;
        return {rec, g2_xy + 16 * (size_t)row, row >= n_g2 || (rec[8] & 0xff) || g2_inf[row]};
    }
};

}  // namespace zg

using namespace zg;

static constexpr size_t DC_MAX_G1 = (size_t)1 << 16, DC_MAX_G2 = (size_t)1 << 24, DC_MAX_POLYS = (size_t)1 << 16, DC_MAX_ROWS = (size_t)1 << 24;
static_assert(sizeof(size_t) == sizeof(uint64_t), "the row offsets cross as 64-bit words");
static constexpr size_t DC_TABLE_SLICE = 4096;  // columns per table-build launch: 255 records of 192 bytes of scratch each

// ZG_OP_DORY_COMMIT_SPLIT (zolt_gpu_internal.h): upload, row sums, Horner and affine, Miller, products and final exponentiations
static thread_local double t_dc_split[5];
static bool dc_timed() {
    static const bool on = [] { const char *v = getenv("ZG_DORY_COMMIT_TIMES"); return v && *v && *v != '0'; }();
    return on;
}
// closes stage `stage` of a timed call: waits for the stream and books the time since the last mark
struct DcClock {
    hipStream_t st;
    bool on = dc_timed();
    double last = on ? now_ms() : 0.0;
    explicit DcClock(hipStream_t s) : st(s) {}
    void mark(int stage) {
        if (!on) return;
        (void)hipStreamSynchronize(st);
        const double t = now_ms();
        t_dc_split[stage] = t - last;
        last = t;
    }
};

static void dc_key_free(zg_dory_key_s *key) {
    if (!key) return;
    if (key->bases) (void)zg_g1_bases_free(key->bases);
    for (void *p : key->blocks) pool_free(p);
    delete key;
}

static bool dc_key_alloc(zg_dory_key_s *key) {
    const size_t n1 = key->n_g1, n2 = key->n_g2;
    return pool_grab(key->blocks, key->g1, n1 * 64) && pool_grab(key->blocks, key->g1_inf, n1) && pool_grab(key->blocks, key->g2, n2 * 128) && pool_grab(key->blocks, key->g2_inf, n2) &&
           pool_grab(key->blocks, key->table, n1 * DC_DIGITS * 64);
}

// the digit table and the MSM handle over the generators the key already holds, on sg.st; the caller ends with sg.finish()
static int dc_key_tables(zg_dory_key_s *key, Staging &sg) {
    const size_t n1 = key->n_g1;
    hipStream_t st = sg.st;
    const size_t slice = n1 < DC_TABLE_SLICE ? n1 : DC_TABLE_SLICE;
    char *rec = sg.out<char>(slice * DC_DIGITS * 144), *pref = sg.out<char>(slice * DC_DIGITS * 48);
    if (!sg.ok()) return sg.rc;
    for (size_t first = 0; first < n1; first += slice) {
        const size_t count = n1 - first < slice ? n1 - first : slice;
        hipLaunchKernelGGL(dory_commit_table_kernel, dim3(div_up(count, 64)), dim3(64), 0, st, key->g1, key->g1_inf, (uint32_t)first, (uint32_t)count, key->table, rec,
                           pref);
    }
    sg.launched();
    const zg_msm_config cfg = {0, 0, 0};  // a key lives for the run: the planner's "many uses"
    return zg_g1_bases_upload_dev(key->g1, key->g1_inf, n1, &cfg, st, &key->bases);
}

static int dc_key_build(zg_dory_key_s *key, const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf) {
    const size_t n1 = key->n_g1, n2 = key->n_g2;
    if (!dc_key_alloc(key)) return ZG_ERR_NOMEM;
    Staging sg(lib_stream());
    hipStream_t st = sg.st;
    ZG_HIP(hipMemcpyAsync(key->g1, g1_xy, n1 * 64, hipMemcpyHostToDevice, st));
    if (g1_inf) ZG_HIP(hipMemcpyAsync(key->g1_inf, g1_inf, n1, hipMemcpyHostToDevice, st));
    else ZG_HIP(hipMemsetAsync(key->g1_inf, 0, n1, st));
    if (n2) {
        ZG_HIP(hipMemcpyAsync(key->g2, g2_xy, n2 * 128, hipMemcpyHostToDevice, st));
        if (g2_inf) ZG_HIP(hipMemcpyAsync(key->g2_inf, g2_inf, n2, hipMemcpyHostToDevice, st));
        else ZG_HIP(hipMemsetAsync(key->g2_inf, 0, n2, st));
    }
    const int rc = dc_key_tables(key, sg);
    const int rc2 = sg.finish();
    return rc != ZG_OK ? rc : rc2;
}

// the device-source form of the key's construction, for point_bytes.hip: a key with its blocks taken and nothing in them; the tables
// over generators the caller has written into key->g1 .. key->g2_inf on sg.st; and the way back when the caller gives up
int zg::dory_key_alloc(size_t n_g1, size_t n_g2, zg_dory_key_s **out) {
    zg_dory_key_s *key = new zg_dory_key_s();
    key->device = current_device();
    key->n_g1 = n_g1;
    key->n_g2 = n_g2;
    if (!dc_key_alloc(key)) {
        dc_key_free(key);
        return ZG_ERR_NOMEM;
    }
    *out = key;
    return ZG_OK;
}
int zg::dory_key_tables(zg_dory_key_s *key, Staging &sg) { return dc_key_tables(key, sg); }
void zg::dory_key_drop(zg_dory_key_s *key) { dc_key_free(key); }

// what one polynomial of a batch is, after validation
struct DcItem {
    uint32_t kind = 0, shift = 0, bits = 0, sigma = 0, nu = 0;
    size_t len = 0, read = 0, rows = 0;  // entries given; entries read; 2^nu (0 for an empty polynomial)
    size_t words() const { return kind == ZG_DORY_POLY_FR ? 4 : kind == ZG_DORY_POLY_CHUNK128 ? 2 : 1; }
};

static int dc_validate(const char *who, zg_dory_key_t key, size_t k, const uint32_t *kinds, const uint64_t *const *data, const size_t *lens,
                       const uint32_t *shifts, const uint32_t *bits, const void *out_gt, std::vector<DcItem> &items, std::vector<size_t> &row_off) {
    if (!key) return invalid(who, "null key");
    if (k > DC_MAX_POLYS) return invalid(who, "more than 2^16 polynomials");
    if (k && (!kinds || !data || !lens || !out_gt)) return invalid(who, "null argument");
    items.resize(k);
    row_off.assign(k + 1, 0);
    for (size_t j = 0; j < k; j++) {
        DcItem &it = items[j];
        it.kind = kinds[j];
        it.len = lens[j];
        if (it.kind > ZG_DORY_POLY_CHUNK128) return invalid(who, "unknown polynomial kind");
        if (it.len >> 40) return invalid(who, "a polynomial of 2^40 entries or more");
        if (it.len && !data[j]) return invalid(who, "a length without data");
        if (it.kind >= ZG_DORY_POLY_CHUNK64) {
            if (!shifts || !bits) return invalid(who, "chunk polynomials need shifts and bits");
            it.shift = shifts[j];
            it.bits = bits[j];
            const uint32_t width = it.kind == ZG_DORY_POLY_CHUNK128 ? 128u : 64u;
            if (it.bits < 1 || it.bits > 8 || it.shift > width || it.shift + it.bits > width) return invalid(who, "1 <= bits <= 8 and shift + bits <= width required");
        }
        if (it.len) {
            uint32_t nv = 0;
            while (((size_t)2 << nv) <= it.len) nv++;  // floor(log2 len)
            if (it.len <= 1) nv = 1;
            it.sigma = (nv + 1) / 2;
            it.nu = nv - it.sigma;
            it.read = it.len <= 1 ? it.len : (size_t)1 << nv;
            it.rows = (size_t)1 << it.nu;
            if (((size_t)1 << it.sigma) > key->n_g1) return invalid(who, "a polynomial needs 2^sigma columns and g1_vec is shorter");
        }
        row_off[j + 1] = row_off[j] + it.rows;
    }
    if (row_off[k] > DC_MAX_ROWS) return invalid(who, "more than 2^24 rows");
    return ZG_OK;
}

// Enqueues the whole batch on sg.st over DEVICE data: d_data[j] / d_aux[j] as validated, rows9 = row_off[k] records, d_out_gt = k values.
// The descriptor vectors are the caller's and outlive sg.finish().
struct DcTables {
    std::vector<DcVirt> virts;
    std::vector<DcPoly> polys;
};

static int dc_enqueue(zg_dory_key_s *key, const std::vector<DcItem> &items, const std::vector<size_t> &row_off, const std::vector<const uint64_t *> &d_data,
                      const std::vector<const uint8_t *> &d_aux, Staging &sg, DcTables &tb, uint64_t *d_rows9, uint64_t *d_out_gt) {
    const size_t k = items.size(), total = row_off[k];
    const int engine = pairing_engine();
    hipStream_t st = sg.st;
    const double t0 = dc_timed() ? now_ms() : 0.0;  // (the caller has waited for its uploads)
    size_t n_sums = 0, waves = 0;
    tb.polys.resize(k);
    for (size_t j = 0; j < k; j++) {
        const DcItem &it = items[j];
        DcPoly &p = tb.polys[j];
        p.rows = (uint32_t)it.rows;
        p.sum0 = (uint32_t)n_sums;
        p.n_virt = it.kind == ZG_DORY_POLY_FR || !it.len ? 0u : it.kind == ZG_DORY_POLY_U64 ? 8u : 1u;
        if (it.kind == ZG_DORY_POLY_FR && it.len) {
            const size_t cols = (size_t)1 << it.sigma;
            const uint64_t *src = d_data[j];
            if (it.read < cols * it.rows) {  // a one-entry polynomial: its row is one entry long — the other scalar is zero
                uint64_t *pad = sg.out<uint64_t>(cols * it.rows * 32);
                if (!sg.ok()) return sg.rc;
                ZG_HIP(hipMemsetAsync(pad, 0, cols * it.rows * 32, st));
                ZG_HIP(hipMemcpyAsync(pad, src, it.read * 32, hipMemcpyDeviceToDevice, st));
                src = pad;
            }
            ZG_TRY(zg_msm_g1_batch_dev(key->bases, cols, src, it.rows, st, d_rows9 + 9 * row_off[j]));
        }
        for (uint32_t w = 0; w < p.n_virt; w++) {
            DcVirt v;
            v.data = d_data[j];
            v.aux = it.kind == ZG_DORY_POLY_U64 ? d_aux[j] : nullptr;
            v.len = it.read;
            v.words = (uint32_t)it.words();
            v.shift = it.kind == ZG_DORY_POLY_U64 ? 8 * w : it.shift;
            v.mask = it.kind == ZG_DORY_POLY_U64 ? 255u : (1u << it.bits) - 1u;
            v.sigma = it.sigma;
            v.rows = (uint32_t)it.rows;
            v.lanes_log2 = it.sigma <= 4 ? 0u : it.sigma >= 10 ? 6u : it.sigma - 4;  // 2^sigma / 16 lanes, at most a wave
            v.first_wave = (uint32_t)waves;
            v.out = (uint32_t)n_sums;
            tb.virts.push_back(v);
            waves += ((it.rows << v.lanes_log2) + 63) >> 6;
            n_sums += it.rows;
        }
    }
    if (n_sums >> 31 || waves >> 24) return invalid("zg_dory_commit_batch", "the batch is too large for one launch set");
    const DcVirt *d_virts = tb.virts.empty() ? nullptr : sg.in(tb.virts.data(), tb.virts.size() * sizeof(DcVirt));
    const DcPoly *d_polys = sg.in(tb.polys.data(), k * sizeof(DcPoly));
    const size_t *d_row_off = sg.in(row_off.data(), (k + 1) * sizeof(size_t));
    char *d_sums = sg.out<char>((n_sums ? n_sums : 1) * 144);
    uint64_t *d_miller = sg.out<uint64_t>((total ? total : 1) * Fp12::BYTES), *d_prod = sg.out<uint64_t>(k * Fp12::BYTES);
    if (!sg.ok()) return sg.rc;
    DcClock clock(st);
    clock.last = t0;
    if (waves)
        hipLaunchKernelGGL(dory_commit_rowsum_kernel, dim3(div_up(waves * 64, 256)), dim3(256), 0, st, key->table, key->g1_inf, d_virts, (uint32_t)tb.virts.size(),
                           (uint32_t)waves, d_sums);
    clock.mark(1);
    if (total && waves) hipLaunchKernelGGL(dory_commit_finish_kernel, dim3(div_up(total, 64)), dim3(64), 0, st, d_polys, d_row_off, (uint32_t)k, (uint32_t)total, d_sums, d_rows9);
    clock.mark(2);
    pair_set_miller_enqueue(DcRowPairs{d_rows9, d_row_off, (uint32_t)k, key->g2, key->g2_inf, (uint32_t)key->n_g2}, total, st, d_miller, engine);
    clock.mark(3);
    pair_product_final_enqueue(d_miller, total, d_row_off, k, st, d_prod, d_out_gt, engine);
    clock.mark(4);
    sg.launched();
    return sg.rc;
}

int zg::dory_commit_split_read(int field, uint64_t *out, size_t n) {
    if (field != ZG_FIELD_FR || n != 5 || !out) return invalid("zg_field_op", "ZG_OP_DORY_COMMIT_SPLIT takes Fr, n = 5 and an output");
    memcpy(out, t_dc_split, sizeof t_dc_split);
    return ZG_OK;
}

extern "C" {

int zg_dory_key_create(const uint64_t *g1_xy, const uint8_t *g1_inf, size_t n_g1, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n_g2, zg_dory_key_t *out) {
    ZG_INIT();
    const char *who = "zg_dory_key_create";
    if (!out) return invalid(who, "no key pointer");
    *out = nullptr;
    if (n_g1 < 1 || n_g1 > DC_MAX_G1 || n_g2 > DC_MAX_G2) return invalid(who, "1 <= n_g1 <= 2^16 and n_g2 <= 2^24 required");
    if (!g1_xy || (n_g2 && !g2_xy)) return invalid(who, "null data");
    zg_dory_key_s *key = new zg_dory_key_s();
    key->device = current_device();
    key->n_g1 = n_g1;
    key->n_g2 = n_g2;
    key->g2_0_inf = n_g2 && g2_inf && g2_inf[0];
    const int rc = dc_key_build(key, g1_xy, g1_inf, g2_xy, g2_inf);
    if (rc != ZG_OK) {
        dc_key_free(key);
        return rc;
    }
    *out = key;
    return ZG_OK;
}

int zg_dory_key_free(zg_dory_key_t key) {
    if (!key) return ZG_OK;
    ZG_INIT();
    {
        std::lock_guard<std::mutex> lk(key->mu);
        if (key->sessions) return invalid("zg_dory_key_free", "an opening session over the key is still open");
    }
    DeviceGuard dg(key->device);
    (void)hipDeviceSynchronize();  // the blocks go back to the pool idle
    dc_key_free(key);
    return ZG_OK;
}

int zg_dory_key_len(zg_dory_key_t key, size_t *n_g1, size_t *n_g2) {
    if (!key) return invalid("zg_dory_key_len", "null key");
    if (n_g1) *n_g1 = key->n_g1;
    if (n_g2) *n_g2 = key->n_g2;
    return ZG_OK;
}

int zg_dory_commit_batch(zg_dory_key_t key, size_t k, const uint32_t *kinds, const uint64_t *const *data, const uint8_t *const *aux, const size_t *lens,
                         const uint32_t *shifts, const uint32_t *bits, uint64_t *out_gt, uint64_t *out_rows, uint64_t *out_rows_off) {
    ZG_INIT();
    std::vector<DcItem> items;
    std::vector<size_t> row_off;
    ZG_TRY(dc_validate("zg_dory_commit_batch", key, k, kinds, data, lens, shifts, bits, out_gt, items, row_off));
    if (k) {
        DeviceGuard dg(key->device);
        std::lock_guard<std::mutex> lk(key->mu);
        DcTables tb;  // declared before the staging object: the copies out of it are complete when it goes
        std::vector<const uint64_t *> d_data(k, nullptr);
        std::vector<const uint8_t *> d_aux(k, nullptr);
        Staging sg(lib_stream());
        DcClock upload(sg.st);
        // a column named by several polynomials crosses once: the 32 InstructionRa chunks read one
        std::map<std::pair<const void *, size_t>, const void *> seen;
        for (size_t j = 0; j < k && sg.ok(); j++) {
            const DcItem &it = items[j];
            if (!it.len) continue;
            const size_t bytes = it.read * it.words() * 8;
            auto at = seen.find({data[j], bytes});
            if (at == seen.end()) at = seen.emplace(std::make_pair((const void *)data[j], bytes), (const void *)sg.in(data[j], bytes)).first;
            d_data[j] = reinterpret_cast<const uint64_t *>(at->second);
            if (it.kind == ZG_DORY_POLY_U64 && aux && aux[j]) {
                auto as = seen.find({aux[j], it.read});
                if (as == seen.end()) as = seen.emplace(std::make_pair((const void *)aux[j], it.read), (const void *)sg.in(aux[j], it.read)).first;
                d_aux[j] = reinterpret_cast<const uint8_t *>(as->second);
            }
        }
        const size_t total = row_off[k];
        uint64_t *d_rows9 = sg.out<uint64_t>((total ? total : 1) * 72), *d_gt = sg.out<uint64_t>(k * Fp12::BYTES);
        upload.mark(0);
        if (sg.ok()) {
            const int rc = dc_enqueue(key, items, row_off, d_data, d_aux, sg, tb, d_rows9, d_gt);
            if (rc != ZG_OK && sg.ok()) return rc;  // (the staging object waits for what was enqueued)
        }
        sg.fetch(out_gt, d_gt, k * Fp12::BYTES);
        if (total) sg.fetch(out_rows, d_rows9, total * 72);
        ZG_TRY(sg.finish());
    }
    if (out_rows_off) memcpy(out_rows_off, row_off.data(), (k + 1) * sizeof(uint64_t));
    return ZG_OK;
}

int zg_dory_commit_batch_dev(zg_dory_key_t key, size_t k, const uint32_t *kinds, const uint64_t *const *data, const uint8_t *const *aux, const size_t *lens,
                             const uint32_t *shifts, const uint32_t *bits, void *stream, uint64_t *d_out_gt, uint64_t *d_out_rows, uint64_t *out_rows_off) {
    ZG_INIT();
    std::vector<DcItem> items;
    std::vector<size_t> row_off;
    ZG_TRY(dc_validate("zg_dory_commit_batch_dev", key, k, kinds, data, lens, shifts, bits, d_out_gt, items, row_off));
    if (k) {
        DeviceGuard dg(key->device);
        std::lock_guard<std::mutex> lk(key->mu);
        DcTables tb;
        std::vector<const uint64_t *> d_data(data, data + k);
        std::vector<const uint8_t *> d_aux(k, nullptr);
        for (size_t j = 0; j < k; j++) d_aux[j] = aux && items[j].len ? aux[j] : nullptr;
        Staging sg(pick_stream(stream));  // the scratch goes back to the pool on return: the launch set is complete by then
        t_dc_split[0] = 0.0;  // nothing is uploaded here: the split of this call does not carry an earlier call's figure
        const size_t total = row_off[k];
        uint64_t *d_rows9 = d_out_rows ? d_out_rows : sg.out<uint64_t>((total ? total : 1) * 72);
        if (sg.ok()) {
            const int rc = dc_enqueue(key, items, row_off, d_data, d_aux, sg, tb, d_rows9, d_out_gt);
            if (rc != ZG_OK && sg.ok()) return rc;
        }
        ZG_TRY(sg.finish());
    }
    if (out_rows_off) memcpy(out_rows_off, row_off.data(), (k + 1) * sizeof(uint64_t));
    return ZG_OK;
}

}  // extern "C"
