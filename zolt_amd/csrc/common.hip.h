// common.hip.h — host-side plumbing shared by the translation units of libzolt_gpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zolt_gpu_internal.h"

struct zg_dory_key_s;

namespace zg {

static constexpr int ZG_MAX_DEVICES = 16;

void set_error(const std::string &msg);
int ensure_init();          // ZG_OK or ZG_ERR_NO_DEVICE / ZG_ERR_HIP
int primary_device();       // the device zg_init / zg_init_devices bound this process to (valid after ensure_init)
int current_device();       // the calling thread's HIP device
hipStream_t lib_stream();   // the library's own stream on the calling thread's CURRENT device (created on first use)
hipStream_t stream_acquire();                     // an idle stream of the current device (created if none): sessions
void stream_release(hipStream_t st, int device);  // back to the free list (streams live until zg_shutdown)
// three streams created back to back (= on three different hardware queues), as a unit: launch sets that are meant to overlap
bool stream_group_acquire(hipStream_t out[3]);
void stream_group_release(const hipStream_t s[3], int device);

// HIP's current device is per host thread (a fresh std.Thread worker starts on device 0) and a handle's memory lives on
// the device it was created on: every entry point pins the calling thread to the right device for its duration.
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(int d) : dev(d) {
        if (d < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    ~DeviceGuard() {
        if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

inline hipStream_t pick_stream(void *s) { return s ? reinterpret_cast<hipStream_t>(s) : lib_stream(); }

#define ZG_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            zg::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
            return ZG_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

#define ZG_TRY(expr)                  \
    do {                              \
        int _r = (expr);              \
        if (_r != ZG_OK) return _r;   \
    } while (0)

// Multi-device code (sharded.hip) runs whole public entry points on another device: inside a DeviceScope the calling thread
// sits on `dev` AND primary_device() reports `dev`, so the ZG_INIT() of every nested entry point keeps it there.
void set_device_override(int dev);  // thread-local; -1 = none
int device_override();
struct DeviceScope {
    int prev_override;
    DeviceGuard guard;
    explicit DeviceScope(int d) : prev_override(device_override()), guard(d) { set_device_override(d); }
    ~DeviceScope() { set_device_override(prev_override); }
};

// every extern "C" compute entry point starts with this: library initialised, thread on the primary device
#define ZG_INIT()                \
    ZG_TRY(zg::ensure_init());   \
    zg::DeviceGuard _zg_primary_guard(zg::primary_device())

// a function attribute (dynamic LDS limit) belongs to the kernel's code object on ONE device: set it once per device
struct PerDeviceOnce {
    std::once_flag flag[ZG_MAX_DEVICES];
    hipError_t err[ZG_MAX_DEVICES];
    template <class F> hipError_t run(F f) {
        int d = current_device();
        if (d < 0 || d >= ZG_MAX_DEVICES) return hipErrorInvalidDevice;
        std::call_once(flag[d], [&] { err[d] = f(); });
        return err[d];
    }
};

// optional per-kernel HIP-event timing (bench.py's roofline leg); ids are ZG_PROF_*
void prof_begin(int id, hipStream_t st);
void prof_end(int id, hipStream_t st);
struct ProfScope {
    int id;
    hipStream_t st;
    ProfScope(int i, hipStream_t s) : id(i), st(s) { prof_begin(id, st); }
    ~ProfScope() { prof_end(id, st); }
};

// Cached device scratch for the host-pointer entry points: hipMalloc/hipFree per call cost more than the
// kernels they serve (hipFree also synchronises the device, which would stall other streams' work).
// A buffer is returned to the cache only after the work using it has been synchronised.
void *scratch_get(size_t bytes);  // nullptr on allocation failure (error set)
void scratch_put(void *p);
// the pool underneath (runtime.hip): size-classed blocks of device memory kept for reuse, for session tables as well as scratch.
// pool_free: the caller has synchronised the work that used the block. dev_malloc: hipMalloc for handle-lifetime allocations, with
// the pool trimmed and one retry when the device is out of memory.
void *pool_alloc(size_t bytes);
void pool_free(void *p);
void pool_trim();
hipError_t dev_malloc(void **p, size_t bytes);
// pinned host staging buffers, kept until zg_shutdown (nullptr + error on failure)
void *pinned_get(size_t bytes);
void pinned_put(void *p);
// a pool block of `bytes` (never empty) for an object that frees its `blocks` together: false when the pool has none
template <class T>
inline bool pool_grab(std::vector<void *> &blocks, T *&ptr, size_t bytes) {
    ptr = reinterpret_cast<T *>(pool_alloc(bytes ? bytes : 16));
    if (ptr) blocks.push_back(ptr);
    return ptr != nullptr;
}
// a mailbox: MAILBOX_WORDS words of pinned, mapped, coherent host memory for kernels that publish to a spinning host (mailbox_wait);
// the taker resets its own flag word. nullptr + error on failure
constexpr size_t MAILBOX_WORDS = 1024;
uint64_t *mailbox_get();
void mailbox_put(uint64_t *p);
// a counter block: `bytes` of device memory on the current device, all-zero when handed out (nullptr + error on failure). clean: every
// launch that used it ran to its end, so the kernels have left the counters at zero; otherwise it is zeroed again, or dropped
// *rc (optional) on failure: ZG_ERR_NOMEM when the pool had no block, ZG_ERR_HIP when a block could not be zeroed
uint64_t *counters_get(size_t bytes, int *rc = nullptr);
void counters_put(uint64_t *p, size_t bytes, int device, bool clean);

// What a device-resident session holds of the runtime's resources, and the one way all of it goes back. A session struct derives from
// this; its open fills it with the calls below (each false + error text on failure, and nothing is lost: release() returns whatever
// was taken so far).
struct SessionRes {
    int device = -1;               // the HIP device everything lives on
    hipStream_t st = nullptr;      // the stream the session works on: the caller's, or own_st
    hipStream_t own_st = nullptr;  // from stream_acquire
    std::vector<void *> blocks;    // device blocks (pool_grab)
    std::vector<void *> pinned;    // pinned staging buffers (pinned_get)
    uint64_t *h_pin = nullptr;     // mailbox
    uint64_t *d_misc = nullptr;    // counter block of misc_bytes
    size_t misc_bytes = 0;
    int fail = ZG_ERR_NOMEM;       // what a failed open returns: out of memory, unless a take says otherwise

    // the session's device and stream: own_st always (a session keeps one whether or not this open uses it), st = caller's if given
    bool take_stream(hipStream_t caller) {
        device = current_device();
        own_st = stream_acquire();
        st = caller ? caller : own_st;
        if (!own_st) set_error("no stream");
        return own_st != nullptr;
    }
    template <class T> bool take_block(T *&ptr, size_t bytes) { return pool_grab(blocks, ptr, bytes); }
    template <class T> bool take_pinned(T *&ptr, size_t bytes) {
        ptr = reinterpret_cast<T *>(pinned_get(bytes));
        if (ptr) pinned.push_back(ptr);
        return ptr != nullptr;
    }
    bool take_mailbox() { return (h_pin = mailbox_get()) != nullptr; }
    bool take_counters(size_t bytes) { return (d_misc = counters_get(misc_bytes = bytes, &fail)) != nullptr; }
    // Waits for `st` (the caller is on `device`, and a caller's stream is alive: this runs inside the close or the failed open), then
    // gives everything back. The wait is what pool_free's contract asks for, and its result says whether the counters are at zero.
    void release() {
        const bool drained = !st || hipStreamSynchronize(st) == hipSuccess;
        for (void *p : blocks) pool_free(p);
        for (void *p : pinned) pinned_put(p);
        mailbox_put(h_pin);
        counters_put(d_misc, misc_bytes, device, drained);
        stream_release(own_st, device);
        blocks.clear();
        pinned.clear();
        h_pin = d_misc = nullptr;
        st = own_st = nullptr;
    }
};

// the argument checks of every entry point: return invalid("zg_x: what is wrong");
inline int invalid(const std::string &msg) {
    set_error(msg);
    return ZG_ERR_INVALID;
}
inline int invalid(const char *who, const char *what) { return invalid(std::string(who) + ": " + what); }

// Every entry point that needs device scratch reads: validate, stage inputs, launch, fetch outputs, finish. Staging owns the scratch buffers
// AND the wait: they go back to the shared cache only after `st` has been synchronised, on every return path. The first failure sticks
// (ZG_ERR_NOMEM, ZG_ERR_HIP with the failing expression as the error text, or the code of a nested enqueue), later steps do nothing,
// finish() reports it — so a caller checks ok() once, before it launches on the pointers it was given. Whatever else must outlive the
// wait (a pinned block, a stream group) is declared BEFORE the Staging, so that it is destroyed after it.
#define ZG_STAGE(sg, expr) (sg).check((expr), #expr)  // a HIP call that in / fetch do not cover: a memset, a device copy, an event
struct Staging {
    hipStream_t st;
    std::vector<void *> bufs;
    int rc = ZG_OK;
    bool synced = false;
    explicit Staging(hipStream_t s) : st(s) {}
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() {
        if (!synced) (void)hipStreamSynchronize(st);
        for (void *p : bufs) scratch_put(p);
    }
    bool ok() const { return rc == ZG_OK; }
    bool check(hipError_t e, const char *expr) {
        if (e != hipSuccess && ok()) {
            set_error(std::string(expr) + ": " + hipGetErrorString(e));
            rc = ZG_ERR_HIP;
        }
        return ok();
    }
    // the return code of a nested enqueue that reports its own error text (eq_table_enqueue, launch_fold, an MSM launch set, ...)
    bool adopt(int r) {
        if (r != ZG_OK && ok()) rc = r;
        return ok();
    }
    // device scratch of `bytes` (an output, or working memory of the launch set)
    template <class T = void> T *out(size_t bytes) {
        void *p = ok() ? scratch_get(bytes) : nullptr;
        if (p) bufs.push_back(p);
        else if (ok()) rc = ZG_ERR_NOMEM;
        return reinterpret_cast<T *>(p);
    }
    // optional scratch: nullptr when the pool has none, and the call goes on without it (HIP's last error cleared, rc untouched)
    template <class T = void> T *try_out(size_t bytes) {
        void *p = ok() ? scratch_get(bytes) : nullptr;
        if (p) bufs.push_back(p);
        else (void)hipGetLastError();
        return reinterpret_cast<T *>(p);
    }
    // a device copy of host[0, bytes); an absent optional array (host == nullptr) stays absent
    template <class T> T *in(const T *host, size_t bytes) {
        if (!host) return nullptr;
        T *d = out<T>(bytes);
        if (d && !ZG_STAGE(*this, hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st))) return nullptr;
        return d;
    }
    bool launched() { return ZG_STAGE(*this, hipGetLastError()); }  // after the launches
    void fetch(void *host, const void *dev, size_t bytes) {
        if (host && ok()) ZG_STAGE(*this, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    }
    int finish() {
        hipError_t e = hipStreamSynchronize(st);
        synced = true;
        check(e, "hipStreamSynchronize(st)");
        return rc;
    }
    // for a caller that has SEEN the stream's last work complete (the mailbox flag of the last kernel, a callee's own wait): no second
    // wait when all went well
    int finish_drained() {
        if (!ok()) return finish();
        synced = true;
        return rc;
    }
};

// set-up phase split for the bench (include/zolt_gpu_internal.h: zg_last_setup_times); phases are only separated by synchronisations
// when ZG_SETUP_TIMES is set
struct SetupTimes { double alloc_ms = 0, h2d_ms = 0, kernel_ms = 0, other_ms = 0; };
SetupTimes &setup_times();   // the calling thread's record
bool setup_times_enabled();
double now_ms();

static inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// r = a + b mod the BN254 scalar modulus on the host, canonical inputs (src/field/mod.zig:782-798)
static inline void fr_add_host(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
    static const uint64_t M[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    uint64_t t[4];
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a[i] + b[i];
        t[i] = (uint64_t)c;
        c >>= 64;
    }
    uint64_t carry = (uint64_t)c, d[4];
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; i++) {
        unsigned __int128 x = (unsigned __int128)t[i] - M[i] - (uint64_t)br;
        d[i] = (uint64_t)x;
        br = (x >> 64) & 1;
    }
    bool ge = carry || !br;
    for (int i = 0; i < 4; i++) r[i] = ge ? d[i] : t[i];
}

// The host side of a round that ended inside its kernel: spin on the sequence word of the session's pinned mailbox (word `flag_off` of
// `pin`, written by the GPU after the values: system-scope stores, drained in between) until it shows `seq`; fall back to a
// synchronisation of `st` if it does not arrive promptly. Then out[0, words) = pin[0, words). The caller holds the session's mutex.
static inline int mailbox_wait(const uint64_t *pin, size_t flag_off, uint64_t seq, hipStream_t st, uint64_t *out, int words) {
    ZG_HIP(hipGetLastError());
    const volatile uint64_t *flag = pin + flag_off;
    bool got = false;
    for (uint64_t spin = 0; spin < (1ull << 22); spin++) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) { got = true; break; }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (!got) ZG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < words; i++) out[i] = pin[i];
    return ZG_OK;
}

int bound_devices();      // devices 0..n-1 bound by zg_init_devices (1 in the one-GPU-per-process model)
void sharded_shutdown();  // sharded.hip: drop communicators / exchange buffers (called by zg_shutdown)

// msm.hip: zg_msm_g1_batch_dev that also fuses zero-padded rows on wide-window handles (HyperKZG.open's long levels)
// row_len (optional, k entries): row j holds zeros from row_len[j] on — the digit and sort kernels then walk the live entries only
int msm_batch_dev_wide(zg_bases_t b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out9, const size_t *row_len = nullptr);
// msm.hip, for sharded.hip: k un-normalised Jacobian partials of this device's shard; the combine of gathered partials
int msm_batch_partials_dev(zg_bases_t b, size_t n, const uint64_t *d_scalars, size_t k, hipStream_t st, uint64_t *d_out12);
int msm_combine_batch_enqueue(const uint64_t *d_partials, size_t ranks, size_t rank_stride, size_t k, hipStream_t st, uint64_t *d_out9);
int bases_device(zg_bases_t b);
// ingest.hip: host columns widened into the cycle-major matrix at d_rows on st (synchronous: zg_fr_rows_from_columns, zg_sumcheck_open_column)
int rows_from_host_columns(const zg_col_t *cols, size_t n_cols, size_t n_rows, uint64_t *d_rows, hipStream_t st);
// ingest.hip: d_out[i] = F.fromU64(d_vals[i]) as canonical Montgomery elements, one launch on st (zg_msm_g1_u64's widening step)
int ingest_u64_to_fr(const uint64_t *d_vals, size_t n, uint64_t *d_out, hipStream_t st);
// poly.hip, for sharded.hip: enqueue a session's round-sums pass without waiting for its mailbox
int sc_round_sums_start(zg_sc_t s);
// poly.hip: out_host[i] = d_table[idx_host[i]] (32-byte elements; every index < len) through one gather launch on st, synchronous
int gather_to_host(const uint64_t *d_table, size_t len, const uint64_t *idx_host, size_t n, uint64_t *out_host, hipStream_t st);
// poly.hip: an unsigned environment switch clamped to [lo, hi], dflt when unset or empty (read at every call)
unsigned env_uint(const char *name, unsigned dflt, unsigned lo, unsigned hi);
// poly.hip: the workgroup cap of a sumcheck-family grid, dflt unless ZG_SC_MAX_BLOCKS overrides it; the 256-thread pair-sum grid over `half`
unsigned sc_block_cap(unsigned dflt);
unsigned sc_blocks(size_t half);
// poly.hip: the eq(r, .) table of v challenges (host pointers, optional scale) into d_out in one asynchronous launch on st
int eq_table_enqueue(const uint64_t *r_host, size_t v, const uint64_t *scale_host, uint64_t *d_out, hipStream_t st);
// hyperkzg.hip, for poly_launch_shape: the workgroups of one level of HyperKZG.open over `half` pairs (ZG_SHAPE_HK_FOLD)
unsigned hk_fold_grid(size_t half);
// zg_selftest_launch_shape's families, each answered by the unit whose launches choose that shape (poly.hip: ZG_SHAPE_EQ_*, ZG_SHAPE_SC_*;
// msm.hip: ZG_SHAPE_FB; rrw.hip: ZG_SHAPE_RRW; psc.hip: ZG_SHAPE_PSC); arguments already validated, out[4] zeroed
void poly_launch_shape(int family, size_t a, size_t b, uint32_t *out);
void fb_launch_shape(size_t n, uint32_t *out);
void rrw_launch_shape(size_t inner, uint32_t outer, uint32_t *out);
void psc_launch_shape(size_t pairs, uint32_t *out);
// pairing.hip: the ZG_OP_FP12_* self-test hooks of zg_field_op — n_elems Fp12 elements (12 Fp each) at device pointers, one launch on st
int fp12_selftest_enqueue(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n_elems, hipStream_t st);
// pairing.hip: the product launch and the final-exponentiation launch of every pair set (the Miller launch is pair_set.hip.h's) —
// pair_product_kernel over k > 0 segments [d_seg[j], d_seg[j + 1]) of the n Miller values at d_miller into d_prod (k * 48 words); the
// final exponentiations of n values, by the kernel that `engine` (ZG_PAIRING_ENGINE_*, read once by the entry point) names; and the
// two in a row, the k products through d_prod into d_out
void pair_product_enqueue(const uint64_t *d_miller, size_t n, const size_t *d_seg, size_t k, hipStream_t st, uint64_t *d_prod);
void pair_final_exp_enqueue(const uint64_t *d_in, size_t n, hipStream_t st, uint64_t *d_out, int engine);
void pair_product_final_enqueue(const uint64_t *d_miller, size_t n, const size_t *d_seg, size_t k, hipStream_t st, uint64_t *d_prod, uint64_t *d_out, int engine);
// pairing_wave.hip: the process-wide engine setting (zg_pairing_engine_get without the C linkage); the wave engine's final
// exponentiations (a wave per value; nothing is launched for n == 0); the ZG_OP_FP12W_* hooks, a wave per element
int pairing_engine();
void pairw_final_exp_enqueue(const uint64_t *d_in, size_t n, hipStream_t st, uint64_t *d_out);
int fp12w_selftest_enqueue(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n_elems, hipStream_t st);
// g2.hip, for dory.hip: zg_g2_fixed_base_mul_batch's launch set over device pointers (n > 0, the base not the identity); the window table
// is scratch of sg
void g2_fixed_base_enqueue(Staging &sg, const uint64_t *d_base, const uint64_t *d_sc, size_t n, uint64_t *d_out, uint8_t *d_inf);
// dory.hip: the ZG_OP_DORY_* self-test hooks of zg_field_op — the state of an opening session as host records (synchronous)
int dory_state_read(int field, int op, const uint64_t *handle_word, const uint64_t *b, uint64_t *out, size_t n);
// dory_commit.hip: the ZG_OP_DORY_COMMIT_SPLIT hook of zg_field_op — the stage times of the calling thread's last commitment batch
int dory_commit_split_read(int field, uint64_t *out, size_t n);
// dory_commit.hip, for point_bytes.hip: zg_dory_key_create from DEVICE generators — a key with its blocks taken (1 <= n_g1 <= 2^16,
// n_g2 <= 2^24, on the current device); the digit table and the MSM handle over what the caller wrote into key->g1 .. key->g2_inf on
// sg.st, which the caller finishes (it also sets key->g2_0_inf); and the way back, with the key's work synchronised
int dory_key_alloc(size_t n_g1, size_t n_g2, zg_dory_key_s **out);
int dory_key_tables(zg_dory_key_s *key, Staging &sg);
void dory_key_drop(zg_dory_key_s *key);

}  // namespace zg

// dory_commit.hip's resident key (created and freed there), read in place by dory_vsetup.hip and by the opening sessions dory.hip
// begins over it: both generator vectors with their flags (never null), on `device`; a call that launches over them holds `mu`, an
// opening session counts in `sessions` (under `mu`) from its begin to its close and only reads
struct zg_dory_key_s {
    int device = 0;
    size_t n_g1 = 0, n_g2 = 0;
    uint64_t *g1 = nullptr, *g2 = nullptr;
    uint8_t *g1_inf = nullptr, *g2_inf = nullptr;
    char *table = nullptr;         // 255 * n_g1 rows of 64 bytes
    zg_bases_t bases = nullptr;    // over g1_vec: the rows of Montgomery Fr polynomials, e1_beta of an opening
    bool g2_0_inf = false;         // g2_vec[0] is the identity (the host's flag at create)
    int sessions = 0;              // open zg_dory_t over this key: zg_dory_key_free refuses while there are any
    std::vector<void *> blocks;
    std::mutex mu;
};
