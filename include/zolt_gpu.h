/*
 * zolt_gpu.h — C ABI of libzolt_gpu.so, the MI355X (gfx950) backend for Zolt's
 * data-parallel prover inner loops.
 *
 * The reference (MatteoMer/zolt) has no FFI boundary; the seam is a set of Zig
 * generic functions. Each entry point below names the reference
 * function it replaces (paths relative to the reference root). A Zig shim keeps the
 * `src/msm`, `src/poly`, `src/subprotocols` module APIs and forwards here — see
 * INTEGRATION.md for the `extern fn` declarations.
 *
 * Conventions
 *   - field element  : uint64_t[4], little-endian limbs, Montgomery form (R = 2^256),
 *                      canonical (< modulus) — src/field/mod.zig:131,583-584.
 *                      "fr" = BN254 scalar field (:16-41), "fp" = base field (:51-75).
 *   - affine G1 point: uint64_t[8] = x limbs then y limbs (Fp), plus an out-of-band
 *                      uint8_t infinity flag (the Zig struct layout {x,y,infinity} is not
 *                      ABI-stable, src/msm/mod.zig:19-21). Identity is written as
 *                      x = y = 0, inf = 1 like AffinePoint.identity() (:24-30).
 *   - affine G2 point: uint64_t[16] = x.c0, x.c1, y.c0, y.c1 (Fp2 = Fp[u]/(u^2+1), each component four limbs as above), plus an
 *                      out-of-band uint8_t infinity flag. An identity is WRITTEN as G2Point.identity() does — x = 0, y = (one, 0),
 *                      inf = 1 (src/field/pairing.zig:754-760); on INPUT only the flag is looked at. inf pointers may be NULL as
 *                      for G1 (no identity inputs / flags not wanted).
 *   - Jacobian record: uint64_t[12] = X,Y,Z (Fp); identity = (1,1,0) (:154-160).
 *   - every function returns 0 on success or a ZG_ERR_* code, never throws, and is
 *     re-entrant (MSM.compute is called from std.Thread workers, src/msm/mod.zig:637,732).
 *     zg_last_error() gives the calling thread's last message.
 *   - "_dev" variants take DEVICE pointers (hipMalloc'ed / torch tensors' data_ptr) and a
 *     hipStream_t passed as void* (NULL = the library's own non-blocking stream, which is NOT ordered
 *     with the legacy default stream: pass your stream explicitly when other work consumes the
 *     result); work is enqueued asynchronously unless the function returns a host value.
 *   - No CPU fallback exists: without a usable gfx950 device every compute entry point
 *     fails with ZG_ERR_NO_DEVICE.
 */
#ifndef ZOLT_GPU_H
#define ZOLT_GPU_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define ZG_API __attribute__((visibility("default")))
#else
#define ZG_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ZG_OK 0
#define ZG_ERR_INVALID 1   /* bad argument */
#define ZG_ERR_HIP 2       /* HIP runtime error (see zg_last_error) */
#define ZG_ERR_NOMEM 3
#define ZG_ERR_NO_DEVICE 4
#define ZG_ERR_VERIFY 5    /* error.SumcheckVerificationFailed (src/subprotocols/mod.zig:175-178) */

#define ZG_FIELD_FR 0
#define ZG_FIELD_FP 1

/* elementwise ops for zg_field_op */
#define ZG_OP_MUL 0        /* montgomeryMul, src/field/mod.zig:269-308 / :735-779 */
#define ZG_OP_ADD 1        /* :402-417 / :782-798 */
#define ZG_OP_SUB 2        /* :420-435 / :801-816 */
#define ZG_OP_NEG 3        /* :494-497 / :944-947 (b ignored) */
#define ZG_OP_SQR 4        /* :443-445 / :866-941 (b ignored) */
#define ZG_OP_INV 5        /* :500-518 / :955-983; inverse(0) -> 0 (b ignored) */
#define ZG_OP_FROM_MONT 6  /* :187-189 / :642-645 (b ignored) */
#define ZG_OP_TO_MONT 7    /* fromBytes' reduction :171-184 / :625-639: raw 256-bit LE -> Montgomery (b ignored) */
/* op codes 9..24 are self-test hooks for the device arithmetic: include/zolt_gpu_internal.h */

/* ------------------------------------------------------------------ ABI version and sections
 * MAJOR changes when an existing signature or layout changes, MINOR when entry points are added. A host binds against the header it was
 * built with and checks zg_abi_version() >> 16 == ZG_ABI_MAJOR (and the minor it needs) after loading the library.
 *
 * Sections of this header:
 *   CORE      lifecycle, device memory, field vectors, G1 bases / MSM / HyperKZG, poly tables, sumcheck sessions, product-form
 *             sessions, several GPUs in one process — the path BASELINE.json's north_star names.
 *   OPTIONAL  protocol-specific device sessions for two of the reference's stage provers (zg_rrw_*: RegistersReadWriteChecking,
 *             zg_rwc_*: RamReadWriteChecking). A host that only re-points MSM / poly / sumcheck call sites never touches them:
 *             compile with -DZG_NO_PROTOCOL_SESSIONS to leave them out of the binding; zg_abi_features() reports whether the loaded
 *             library carries them.
 * 1.10 (round 6): NO entry point added — the boundary is frozen; zg_hyperkzg_setup accepts the reference's largest key (2^24 + 256 powers,
 * formerly at most 2^24) and keeps the identity flags of tau = 0.
 * 1.11: the section "G2 (Dory)" — a missing GROUP at the level of zg_g1_*, not another prover mirror: seven zg_g2_* / zg_msm_g2* entry
 * points and zg_g1_axpy_batch; ZG_FEATURE_G2.
 * Still 1.11: the section "Pairings (Dory)" — five entry points, zg_miller_loop_batch .. zg_multi_pairing_dev — is announced by
 * ZG_FEATURE_PAIRING alone. The minor did not move because hosts and tests pin 1.11 as the G2 boundary; ask zg_abi_features().
 * Still 1.11: the section "Dory opening (session)" — zg_dory_open_begin .. zg_dory_open_close, the whole of openWithTranscript's device side
 * on top of the two sections above — is announced by ZG_FEATURE_DORY_OPEN alone, for the same reason.
 * Still 1.11: the section "Dory commitments (key and batch)" — zg_dory_key_create .. zg_dory_commit_batch_dev, every commitment of a proof
 * in one call over a resident key — is announced by ZG_FEATURE_DORY_COMMIT alone, for the same reason.
 * Still 1.11: the section "Dory verifier setup" — zg_dory_verifier_setup_levels, zg_dory_verifier_setup, zg_dory_verifier_setup_points, every
 * chi and delta of a key in one launch set — is announced by ZG_FEATURE_DORY_VSETUP alone, for the same reason.
 * Still 1.11: the section "Pairings (engine)" — zg_pairing_engine_set, zg_pairing_engine_get, a second engine behind every pairing above —
 * is announced by ZG_FEATURE_PAIRING_WAVE alone, for the same reason.
 * Still 1.11: the section "Dory opening (over a key, `open`)" — zg_dory_open_key_begin and zg_dory_open_run, the opening the prover
 * calls, over a resident key and in one call — is announced by ZG_FEATURE_DORY_OPEN_KEY alone, for the same reason.
 * Still 1.11: the section "Points from bytes" — zg_g1_points_from_bytes, zg_g2_points_from_bytes, zg_g1_bases_from_bytes,
 * zg_dory_key_from_bytes, the byte formats of key and proof files decoded on the device — is announced by ZG_FEATURE_POINT_BYTES alone,
 * for the same reason.
 * Still 1.11: the section "field vectors (device)" — zg_field_op_dev .. zg_fr_dense_evaluate_dev, field.BatchOps on resident tables with
 * Montgomery's trick for the inverses — is announced by ZG_FEATURE_FIELD_VECTORS alone, for the same reason. */
#define ZG_ABI_MAJOR 1
#define ZG_ABI_MINOR 11
#define ZG_FEATURE_PROTOCOL_SESSIONS 1u /* zg_rrw_* and zg_rwc_* are exported */
#define ZG_FEATURE_RCCL 2u              /* the several-GPU entry points can exchange partials over RCCL */
#define ZG_FEATURE_COLUMN_INGEST 4u     /* zg_fr_rows_from_columns[_dev] */
#define ZG_FEATURE_G2 8u                /* the section "G2 (Dory)" */
#define ZG_FEATURE_PAIRING 16u          /* the section "Pairings (Dory)" */
#define ZG_FEATURE_DORY_OPEN 32u        /* the section "Dory opening (session)" */
#define ZG_FEATURE_DORY_COMMIT 64u      /* the section "Dory commitments (key and batch)" */
#define ZG_FEATURE_DORY_VSETUP 128u     /* the section "Dory verifier setup" */
#define ZG_FEATURE_PAIRING_WAVE 256u
#define ZG_FEATURE_DORY_OPEN_KEY 512u   /* the section "Dory opening (over a key, `open`)" */
#define ZG_FEATURE_POINT_BYTES 1024u    /* the section "Points from bytes" */
#define ZG_FEATURE_FIELD_VECTORS 2048u  /* the section "field vectors (device)" */
ZG_API uint32_t zg_abi_version(void);  /* (ZG_ABI_MAJOR << 16) | ZG_ABI_MINOR of the library that was loaded */
ZG_API uint32_t zg_abi_features(void); /* ZG_FEATURE_* bits */

/* ------------------------------------------------------------------ lifecycle */
/* Binds the calling process to one GPU (device < 0: keep the current HIP device) and
 * creates the library stream. Idempotent. */
ZG_API int zg_init(int device);
/* ONE process driving several GPUs — the reference's own process model: `zolt prove` is a single process (src/main.zig:271-696)
 * and ParallelMSM.compute runs threads inside it (src/msm/mod.zig:588-653). Binds devices 0..n_devices-1 (n_devices <= 0: every
 * visible device); device 0 stays the primary for the single-device entry points. May follow zg_init(0) / zg_init(-1) on
 * device 0. The sharded entry points below ("several GPUs in one process") then spread their work over the bound devices. */
ZG_API int zg_init_devices(int n_devices);
ZG_API int zg_n_devices(void); /* devices bound: 1 after zg_init, n after zg_init_devices(n), 0 before either */
ZG_API void zg_shutdown(void);
ZG_API const char *zg_last_error(void);
ZG_API const char *zg_version(void);
ZG_API int zg_device_count(void);

/* raw device memory, for hosts without their own HIP binding (the Zig shim). The two copies run on the library's stream and return when
 * they are done: ordered after every earlier call that was given stream = NULL (e.g. the asynchronous zg_fr_eq_table_dev).
 * zg_dev_free returns when the device is idle (hipFree's own guarantee) and keeps the block in the library's device pool for the next
 * allocation of its size class — by zg_dev_alloc or by the library itself (scratch buffers, session tables): a prover that allocates
 * its tables per proof does not pay hipMalloc / hipFree each time, whatever their size. The pool keeps up to a quarter of the device's
 * memory (ZG_DEV_ALLOC_CACHE_MB overrides; 0 = no caching); an allocation that fails returns the idle blocks to the driver and tries
 * again; zg_dev_trim does so on request, zg_shutdown at the end. */
ZG_API int zg_dev_alloc(size_t bytes, void **dptr);
ZG_API int zg_dev_free(void *dptr);
ZG_API int zg_dev_trim(void);
/* pinned host memory (hipHostMalloc) for callers that fill large inputs in place — trace columns, scalar vectors: copies from it run by
 * DMA at link rate whatever the page state of the process. Not pooled: the caller owns the lifetime. */
ZG_API int zg_host_alloc(size_t bytes, void **ptr);
ZG_API int zg_host_free(void *ptr);
ZG_API int zg_dev_memset(void *dst_dev, int byte_value, size_t bytes); /* on the library's stream, returns when done (as the copies do) */
ZG_API int zg_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
ZG_API int zg_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
ZG_API int zg_sync(void);

/* ------------------------------------------------------------------ field vectors */
/* out[i] = op(a[i], b[i]) over n elements; host pointers. Replaces the scalar loops of
 * field.BatchOps (src/field/mod.zig:1164-1280) and backs the device-arithmetic unit tests. */
ZG_API int zg_field_op(int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);

/* DensePolynomial.scale (src/poly/mod.zig:112-126): out[i] = a[i] * s. (DensePolynomial.add, :94-110, is zg_field_op ZG_OP_ADD.) */
ZG_API int zg_fr_scale(const uint64_t *a, size_t n, const uint64_t s[4], uint64_t *out);

/* ------------------------------------------------------------------ field vectors (device) */
/* field.BatchOps (src/field/mod.zig:1164-1280) on tables that live in HBM, and its three routines zg_field_op never had: the inner
 * product, Horner's rule and the batch inverse. `field` is ZG_FIELD_FR or ZG_FIELD_FP; an element is four uint64_t words, canonical
 * Montgomery form. ZG_FEATURE_FIELD_VECTORS.
 *   Streams: a _dev form takes `stream` (a hipStream_t; NULL = the library's stream). It is asynchronous — enqueued, not waited for —
 *   unless it returns a scalar to host memory: then it returns when the scalar is there.
 *   Degenerate and bad arguments: n == 0 is ZG_OK (a scalar output is then zero); null data with n > 0, a scalar pointer that is null,
 *   an unknown field or op: ZG_ERR_INVALID; no device: ZG_ERR_NO_DEVICE.
 *   Overlap: `out` may be exactly `a` (in place). Any other overlap of the output's n elements with an input's is ZG_ERR_INVALID. */

/* zg_field_op on device pointers: the public ops ZG_OP_MUL .. ZG_OP_TO_MONT only (the self-test codes are refused); d_b may be NULL for
 * the ops that ignore b. batchAdd / batchSub / batchMul / batchSquare (:1166-1203). */
ZG_API int zg_field_op_dev(int field, int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n, void *stream);
/* d_out[i] = d_a[i] * s: batchMulScalar (:1190-1195) and DensePolynomial.scale on a resident table. s is read before the call returns. */
ZG_API int zg_field_scale_dev(int field, const uint64_t *d_a, size_t n, const uint64_t s_host[4], uint64_t *d_out, void *stream);
/* batchInverse (:1232-1273), Montgomery's trick: out[i] = a[i]^-1, and out[i] = 0 where a[i] = 0 — the words of ZG_OP_INV, one
 * inversion per group of elements instead of one per element.
 * Divergence from the reference, on purpose: BatchOps.batchInverse seeds products[0] = a[0] without the zero guard it applies to every
 * later element (:1241), so with a[0] = 0 EVERY output of the reference is zero. These entry points compute the element-wise value: zero
 * only where the input is zero. They equal the reference on every input whose first element is non-zero, zeros elsewhere included. */
ZG_API int zg_field_batch_inverse(int field, const uint64_t *a, uint64_t *out, size_t n);
ZG_API int zg_field_batch_inverse_dev(int field, const uint64_t *d_a, uint64_t *d_out, size_t n, void *stream);
/* innerProduct / multiScalarMulLinear (:1206-1213, :1277-1279): out = sum of a[i] * b[i] */
ZG_API int zg_field_inner_product(int field, const uint64_t *a, const uint64_t *b, size_t n, uint64_t out[4]);
ZG_API int zg_field_inner_product_dev(int field, const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream, uint64_t out_host[4]);
/* hornerEval (:1217-1227): out = sum of coeffs[i] * x^i */
ZG_API int zg_field_horner(int field, const uint64_t *coeffs, size_t n, const uint64_t x[4], uint64_t out[4]);
ZG_API int zg_field_horner_dev(int field, const uint64_t *d_coeffs, size_t n, const uint64_t x_host[4], void *stream, uint64_t out_host[4]);
/* zg_fr_dense_evaluate ("poly tables") on a resident table of 2^num_vars evaluations (num_vars <= 30): the eq table of the point, then
 * the inner product above */
ZG_API int zg_fr_dense_evaluate_dev(const uint64_t *d_evals, size_t num_vars, const uint64_t *point_host, void *stream, uint64_t out_host[4]);

/* ------------------------------------------------------------------ G1 bases (SRS) */
typedef struct zg_bases_s *zg_bases_t;

/* MSM tuning. window_bits 0 = auto from n; precompute_levels: 1 = none, 0 = auto,
 * k>1 = store 2^(c*G*l)*P for l<k at upload so k windows share one bucket set
 * (HBM cost k*64 B per base). expected_uses: how many MSMs the handle is expected to serve — 0 = many (an SRS that lives for
 * the whole run: the full table, 64*W bytes per base and a one-time build — 1 GB and ~13 ms at 2^20 bases, 4 GB and ~47 ms at 2^22 —
 * which pays back after ~12 MSMs issued one at a time, ~35 when several are kept in flight: bench.py reports table_build_ms,
 * table_bytes and breakeven_msms in its config); 1..15 = an ad-hoc bases slice (MSM.compute on a temporary): auto picks
 * precompute_levels = 1, no table build. Results do not depend on these. */
typedef struct {
    int window_bits;
    int precompute_levels;
    int expected_uses;
} zg_msm_config;

/* Upload n affine bases once and keep them resident in HBM for any number of MSMs —
 * the device-side image of HyperKZG SetupParams.powers_of_tau_g1
 * (src/poly/commitment/mod.zig:122-140), which lives for the whole prover run.
 * inf may be NULL (no infinity bases). cfg may be NULL (auto). Bases must be on the
 * curve y^2 = x^3 + 3 (src/msm/mod.zig:106-115). */
ZG_API int zg_g1_bases_upload(const uint64_t *xy, const uint8_t *inf, size_t n, const zg_msm_config *cfg, zg_bases_t *out);
ZG_API int zg_g1_bases_upload_dev(const uint64_t *d_xy, const uint8_t *d_inf, size_t n, const zg_msm_config *cfg, void *stream,
                           zg_bases_t *out);
ZG_API int zg_g1_bases_free(zg_bases_t b);
ZG_API size_t zg_g1_bases_len(zg_bases_t b);
/* the plan the handle was built with: window bits c (optimalWindowSize's role, src/msm/mod.zig:475-484, chosen for the GPU),
 * windows per scalar ceil(255 / c), table levels stored per base. Any pointer may be NULL. */
ZG_API int zg_g1_bases_plan(zg_bases_t b, int *window_bits, int *windows, int *precompute_levels);
/* bytes of HBM the handle holds for its bases: the table of precomputed multiples (levels * 64 B per base) or the plain bases */
ZG_API size_t zg_g1_bases_table_bytes(zg_bases_t b);

/* ------------------------------------------------------------------ MSM */
/* MSM(F,G).compute(bases[off..off+n], scalars) -> Affine   (src/msm/mod.zig:355-438)
 * = HyperKZG.commit when bases is the SRS (src/poly/commitment/mod.zig:239-255).
 * n = 0 -> identity (:361-363). Scalars: n x 4 Montgomery Fr limbs on the host. */
ZG_API int zg_msm_g1(zg_bases_t b, size_t off, size_t n, const uint64_t *scalars_mont, uint64_t out_xy[8], uint8_t *out_inf);
/* The same MSM for scalars that are F.fromU64 of machine words, handed over as the words: what `zolt prove` commits to — program bytes,
 * memory values, rd_value per cycle (commitBytecode / commitMemory / commitRegisters, src/zkvm/mod.zig:1518-1617) — is such a vector.
 * 8 instead of 32 bytes per scalar cross PCIe, the conversion runs on the device, and a 64-bit scalar has digits in 4 of the 15 windows
 * only. out = MSM.compute(bases[off..off+n], values.map(F.fromU64)), bit for bit. */
ZG_API int zg_msm_g1_u64(zg_bases_t b, size_t off, size_t n, const uint64_t *values_u64, uint64_t out_xy[8], uint8_t *out_inf);
/* same, scalars already resident in HBM */
ZG_API int zg_msm_g1_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars_mont, void *stream, uint64_t out_xy[8],
                  uint8_t *out_inf);
/* asynchronous form: the affine result (8 limbs) and the flag are written to DEVICE memory */
ZG_API int zg_msm_g1_dev_async(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars_mont, void *stream,
                        uint64_t *d_out_xy, uint8_t *d_out_inf);
/* BatchMSM / ParallelBatchMSM.compute (src/msm/mod.zig:545-565,683-748) = HyperKZG.batchCommit
 * (src/poly/commitment/mod.zig:558-570): k scalar vectors of length n over bases[0..n]. */
ZG_API int zg_msm_g1_batch(zg_bases_t b, size_t n, const uint64_t *const *scalar_batches, size_t k, uint64_t *out_xy /* k*8 */,
                    uint8_t *out_inf /* k */);
/* same with the k vectors resident in HBM back to back (k*n*4 limbs); asynchronous: record i = d_out9[9*i .. 9*i+9) =
 * affine xy[8] followed by a flag word (low byte 1 = identity). Short vectors (Dory row commitments,
 * src/poly/commitment/dory.zig:646-670; commitments of <= 2^14-entry polynomials) are FUSED: the k MSMs run as one
 * sort / accumulate / reduce pass with k times the bucket groups, instead of k latency-bound launch sets; long vectors
 * rotate over three streams so their tails overlap. Results are identical to k separate zg_msm_g1 calls. */
ZG_API int zg_msm_g1_batch_dev(zg_bases_t b, size_t n, const uint64_t *d_scalars_mont, size_t k, void *stream, uint64_t *d_out9);
/* ParallelMSM's per-chunk result (src/msm/mod.zig:656-665): this GPU's partial sum as the
 * reference's Jacobian record fromAffine(SingleMSM.compute(chunk)) = (x,y,1) or (1,1,0),
 * written to DEVICE memory so it can be all-gathered over RCCL without a host round trip. */
ZG_API int zg_msm_g1_partial_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars_mont, void *stream,
                          uint64_t *d_out_jac /* 12 */);
/* Same partial without the normalisation: some Jacobian representative (X, Y, Z) of the shard's sum (identity:
 * Z = 0). It exists only to be fed to zg_g1_combine_partials_dev*, whose result is identical; skipping the
 * per-GPU inversion shortens every rank's step in a sharded MSM. */
ZG_API int zg_msm_g1_partial_fast_dev(zg_bases_t b, size_t off, size_t n, const uint64_t *d_scalars_mont, void *stream,
                               uint64_t *d_out_jac /* 12 */);
/* ParallelMSM's serial combine + toAffine (src/msm/mod.zig:647-652) over k gathered
 * Jacobian partials resident on the device. */
ZG_API int zg_g1_combine_partials_dev(const uint64_t *d_partials_jac /* k*12 */, size_t k, void *stream, uint64_t out_xy[8],
                               uint8_t *out_inf);
/* asynchronous form: result (8 limbs) and flag land in DEVICE memory, ordered on `stream` */
ZG_API int zg_g1_combine_partials_dev_async(const uint64_t *d_partials_jac /* k*12 */, size_t k, void *stream, uint64_t *d_out_xy,
                                     uint8_t *d_out_inf);
/* The same combine for a BATCH of m MSMs behind ONE exchange (ParallelBatchMSM's per-thread partial lists, src/msm/mod.zig:683-748): the
 * gathered buffer holds, for every rank r, that rank's m records back to back at d_partials_jac + r * rank_stride (u64 words,
 * rank_stride >= 12 * m — the layout of one all-gather of m * 96 bytes per rank); result j (xy[8] + flag word, 9 words) goes to
 * d_out9 + 9 * j. One launch of m workgroups, stream-ordered. */
ZG_API int zg_g1_combine_partials_batch_dev_async(const uint64_t *d_partials_jac, size_t ranks, size_t rank_stride, size_t m, void *stream,
                                           uint64_t *d_out9);
/* AffinePoint.isOnCurve (src/msm/mod.zig:106-115) for n points: out[i] = 1 iff infinity or y^2 == x^3 + 3
 * (what parseG1Uncompressed checks per SRS point, src/poly/commitment/srs.zig:93-96). */
ZG_API int zg_g1_is_on_curve_batch(const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out);
/* AffinePoint.add for n independent pairs (src/msm/mod.zig:74-103): the lambda formulas with one field inversion per pair,
 * x1 == x2 resolved as the reference does (:79-88: y1 == -y2 -> identity, y1 == y2 -> double, :118-138); identity operands pass
 * the other point through. AffinePoint.double(p) = add(p, p). Flags may be NULL (no identity inputs / flags not wanted). */
ZG_API int zg_g1_affine_add_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n,
                           uint64_t *out_xy, uint8_t *out_inf);
/* MSM(F,G).scalarMul(base, scalar).toAffine() for n independent (base, scalar) pairs
 * (src/msm/mod.zig:503-540) — the primitive of HyperKZG.setup (commitment/mod.zig:194-199). */
ZG_API int zg_g1_scalar_mul_batch(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars_mont, size_t n,
                           uint64_t *out_xy, uint8_t *out_inf);

/* The same for n scalars over ONE base — HyperKZG.setup's loop powers[i] = MSM.scalarMul(g1, tau^i).toAffine()
 * (src/poly/commitment/mod.zig:194-199; generateMockSRS, srs.zig:326-355): a shared table of the 255 multiples of 2^(8w) * base
 * per 8-bit window, so an output is at most 32 mixed additions and one toAffine instead of 254 doublings + ~127 additions. */
ZG_API int zg_g1_fixed_base_mul_batch(const uint64_t base_xy[8], uint8_t base_inf, const uint64_t *scalars_mont, size_t n, uint64_t *out_xy,
                               uint8_t *out_inf);

/* HyperKZG.setup's G1 side with nothing leaving the device (generateMockSRS, src/poly/commitment/mod.zig:174-213: powers[i] =
 * scalarMul(g1, tau^i), i < n < 2^27 — the reference's largest key is 2^24 + 256 powers, src/host/mod.zig:384-387): powers of tau,
 * fixed-base batch and the handle (with its table of multiples) are built in HBM.
 * out_xy / out_inf (n*8 words / n bytes, host) may be NULL when the caller does not need the points themselves. The handle equals
 * zg_g1_bases_upload of zg_g1_fixed_base_mul_batch's output for the scalars tau^i, infinity flags included (tau = 0: every power
 * but the first is the identity). */
ZG_API int zg_hyperkzg_setup(const uint64_t base_xy[8], const uint64_t tau[4], size_t n, const zg_msm_config *cfg, uint64_t *out_xy, uint8_t *out_inf,
                             zg_bases_t *out);
/* HyperKZG.open (src/poly/commitment/mod.zig:261-324), resident on the device: per variable i the quotient
 * q[j] = cur[j+half] - cur[j] is committed (MSM over srs[0..min(half, srs_len))), then cur is folded by point[i]
 * (high half). Writes num_vars quotient commitments (rounds that the reference skips when the table runs out are
 * reported as the identity) and the final evaluation; num_vars == 0 returns `value` like the reference. */
ZG_API int zg_hyperkzg_open(zg_bases_t srs, const uint64_t *evals, size_t n_evals, const uint64_t *point, size_t num_vars,
                     const uint64_t value[4], uint64_t *q_xy /* num_vars*8 */, uint8_t *q_inf /* num_vars */,
                     uint64_t final_eval[4]);
/* same with the evaluation table already resident in HBM (a prover that has just committed the polynomial from device memory):
 * no 32*n-byte upload; the table is copied on the device (the loop folds in place, the caller's polynomial stays intact) */
ZG_API int zg_hyperkzg_open_dev(zg_bases_t srs, const uint64_t *d_evals, size_t n_evals, const uint64_t *point, size_t num_vars,
                         const uint64_t value[4], void *stream, uint64_t *q_xy /* num_vars*8 */, uint8_t *q_inf /* num_vars */,
                         uint64_t final_eval[4]);
/* HyperKZG.batchOpen (src/poly/commitment/mod.zig:607-732): k polynomials opened at one point through the random linear
 * combination P = sum_i gamma^i p_i, gamma = fromU64(0x9a8b7c6d) * prod_j (point[j] + 11) (the reference's deterministic
 * stand-in for a transcript challenge, :633-640). Outputs: evaluations[k] = evaluateMultilinear(p_i, point) EXACTLY as the
 * reference computes it (:788-817 — the direct sum for point.len <= 10 and len <= 1024, evals[0] otherwise); the quotient
 * commitments of P (*n_quot of them; fewer than num_vars when the fold runs out of elements, :686,714-720; the unused
 * slots are reported as identity); final_eval (combined_eval when num_vars == 0, :665-673) and gamma. Polynomials shorter
 * than polys[0] are zero-extended, longer ones truncated (:649-651). */
ZG_API int zg_hyperkzg_batch_open(zg_bases_t srs, const uint64_t *const *polys, const size_t *lens, size_t k, const uint64_t *point,
                           size_t num_vars, uint64_t *q_xy /* num_vars*8 */, uint8_t *q_inf /* num_vars */, size_t *n_quot,
                           uint64_t *evaluations /* k*4 */, uint64_t final_eval[4], uint64_t gamma[4]);

/* ------------------------------------------------------------------ G2 (Dory) */
/* What the Dory prover does with G2Point in its reduce-and-fold rounds (src/poly/commitment/dory.zig:1545-1635; the same loop at
 * :1240-1340): the twist y^2 = x^3 + 3/(9+u) over Fp2, in the layout of the convention block above. Host pointers unless "_dev".
 * Scalars are Montgomery Fr elements, taken out of Montgomery form once on the device and used as the integers they are (0 <= s < r);
 * a zero scalar or an identity point gives the identity. Results are the reference's affine values, bit for bit. The multi-pairings
 * of the same rounds are the next section; GT exponentiation and the verifier's GT algebra stay the host's. No handle: these vectors
 * are short and change every round. */
/* out[i] = 1 iff infinity or y^2 == x^3 + 3/(9+u) (computeG2YSquared, dory.zig:348-355) */
ZG_API int zg_g2_is_on_curve_batch(const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out);
/* G2Point.add for n independent pairs (src/field/pairing.zig:839-875): an identity operand passes the other point through, x1 == x2
 * with y1 == -y2 gives the identity, x1 == x2 otherwise doubles (:861-875; y == 0 -> identity). One Fp2 inversion per pair. */
ZG_API int zg_g2_affine_add_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n,
                           uint64_t *out_xy, uint8_t *out_inf);
/* G2Point.scalarMul for n independent (point, scalar) pairs (pairing.zig:880-919) */
ZG_API int zg_g2_scalar_mul_batch(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars_mont, size_t n, uint64_t *out_xy,
                           uint8_t *out_inf);
/* The same for n scalars over ONE base — setup's g2_vec[i] = generator.scalarMul(hash_i) (dory.zig:963-966, 1695-1712) and the opening's
 * v2[i] = g2_vec[0].scalarMul(v_vec[i]) (:1513-1519): a shared window table, at most 64 (n <= 256) or 32 mixed additions per output. */
ZG_API int zg_g2_fixed_base_mul_batch(const uint64_t base_xy[16], uint8_t base_inf, const uint64_t *scalars_mont, size_t n, uint64_t *out_xy,
                               uint8_t *out_inf);
/* out[i] = s * a[i] + b[i] with one scalar s for the whole vector — a round's two vector updates: v2[i] += beta_inv * g2_vec[i]
 * (dory.zig:1582-1583: a = g2_vec, b = v2) and v2[i] = alpha_inv * v2[i] + v2[i + n2] (:1621-1624: a = v2[0..n2), b = v2[n2..)).
 * = G2Point.add(a[i].scalarMul(s), b[i]), one inversion per output. out may alias neither input. */
ZG_API int zg_g2_axpy_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const uint64_t s[4], size_t n,
                     uint64_t *out_xy, uint8_t *out_inf);
/* the G1 halves of the same updates, G1 layouts: v1[i] += beta * g1_vec[i] (dory.zig:1579-1580), v1[i] = alpha * v1[i] + v1[i + n2]
 * (:1616-1619) = AffinePoint.add(MSM.scalarMul(a[i], s).toAffine(), b[i]) */
ZG_API int zg_g1_axpy_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const uint64_t s[4], size_t n,
                     uint64_t *out_xy, uint8_t *out_inf);
/* msmG2 (dory.zig:693-703: sum_i g2_vec[i].scalarMul(scalars[i]), n scalar multiplications in the reference) as one bucket MSM sized for
 * n <= 2^13 (at most 2^24). Nothing is tabled or kept: e2_plus / e2_minus run over v2, which changes every round. n = 0 -> identity. */
ZG_API int zg_msm_g2(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars_mont, size_t n, uint64_t out_xy[16], uint8_t *out_inf);
/* same with device pointers: the launch set runs on `stream`, ordered after the work already enqueued there; d_out17 = affine xy[16]
 * followed by a flag word (low byte 1 = identity). The call returns once the record is written (its scratch is pooled). */
ZG_API int zg_msm_g2_dev(const uint64_t *d_xy, const uint8_t *d_inf, const uint64_t *d_scalars_mont, size_t n, void *stream, uint64_t *d_out17);

/* ------------------------------------------------------------------ Pairings (Dory) */
/* The multi-pairings of the PROVER: multiPairG1G2 (src/poly/commitment/dory.zig:673-690) — six of them in every reduce-and-fold round
 * (:1549-1552, :1587-1588), one per commit (:1029-1037), and preprocessing's chi / delta_* (src/zkvm/preprocessing.zig:833-935) — as the
 * optimal ate pairing of src/field/pairing.zig: millerLoopArkworks (:1561-1628) and finalExponentiation (:1653-1681, the hard part
 * :1812-1880, i.e. the power 2x(6x^2 + 3x + 1) (p^12 - 1) / r). Host pointers unless "_dev".
 *   - G1 operands: affine xy[8] + flag byte, as zg_g1_axpy_batch takes them; G2 operands: the layout of zg_g2_*. A NULL flag array
 *     means "no identities". Operands are expected to be points ON their curves (zg_g1_is_on_curve_batch / zg_g2_is_on_curve_batch);
 *     for other inputs the formulas still run and the result is unspecified but never a fault.
 *   - a GT element: uint64_t[48] = twelve Montgomery Fp elements in the order of Fp12.toBytes (pairing.zig:632-633): c0.c0.c0, c0.c0.c1,
 *     c0.c1.c0, ... c1.c2.c1 (Fp12 = Fp6[w]/(w^2 - v), Fp6 = Fp2[v]/(v^3 - (9 + u))). Canonical: the reference's bits.
 *   - a multi-pairing is ONE Miller loop per pair, one product and ONE final exponentiation; the reference exponentiates per pair and
 *     multiplies. Same bits: the final exponentiation is a homomorphism and values are canonical. A Miller value of ZERO cannot arise
 *     from points of the curves; a lane that computes one stores ONE instead, which is what the per-pair finalExponentiation answers
 *     for it (:1654-1664) — so zg_miller_loop_batch never returns zero.
 * GT exponentiation and the verifier's GT algebra are not here. */
/* n unreduced Miller values (millerLoopArkworks); an identity on either side -> one */
ZG_API int zg_miller_loop_batch(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n,
                         uint64_t *out_gt /* n*48 */);
/* finalExponentiation for n independent inputs; zero (the only non-invertible element) -> one */
ZG_API int zg_final_exponentiation_batch(const uint64_t *in_gt, size_t n, uint64_t *out_gt /* n*48 */);
/* pairingFp for n independent pairs (pairing.zig:1276-1286) */
ZG_API int zg_pairing_batch(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n,
                     uint64_t *out_gt /* n*48 */);
/* k multi-pairings in ONE launch set: out[j] = prod_{seg[j] <= i < seg[j+1]} e(P_i, Q_i); seg = k + 1 ascending offsets, seg[k] <= n
 * (ZG_ERR_INVALID otherwise); an empty segment gives one. = multiPairG1G2 (dory.zig:673-690) per segment: a round's six products, or
 * commit's row product, are one call. */
ZG_API int zg_multi_pairing(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n,
                     const size_t *seg /* k+1 */, size_t k, uint64_t *out_gt /* k*48 */);
/* same with device pointers (d_seg too): the launch set runs on `stream`, ordered after the work already enqueued there. The offsets
 * cannot be validated by the host: each end is clamped to n and an inverted range counts as empty. The call returns once the outputs
 * are written (its scratch is pooled), as zg_msm_g2_dev does. */
ZG_API int zg_multi_pairing_dev(const uint64_t *d_g1_xy, const uint8_t *d_g1_inf, const uint64_t *d_g2_xy, const uint8_t *d_g2_inf, size_t n,
                         const size_t *d_seg /* k+1 */, size_t k, void *stream, uint64_t *d_out_gt /* k*48 */);

/* ------------------------------------------------------------------ Dory opening (session) */
/* DoryCommitmentScheme.openWithTranscript (src/poly/commitment/dory.zig:1404-1669) resident on the device: begin uploads the generators,
 * the row commitments and the three scalar vectors once and builds v1, v2, s1, s2 in HBM (:1438-1533); every reduce-and-fold round is
 * then first message -> (host: transcript, beta) -> second message -> (host: transcript, alpha) -> fold, and final closes the proof.
 * The MESSAGES are all that crosses to the host in a round and the challenge scalars all that crosses to the device: no vector is
 * uploaded or downloaded and no zg_bases_t is built after begin; a round costs two host synchronisations, one per message (the fold is
 * enqueued and rides in front of the next first message). The transcript, the `inverse() orelse one` rule for the challenges' inverses
 * and the proof's serialisation are the host's. Host pointers throughout.
 *   - layouts: G1 points and flags as zg_g1_axpy_batch takes them, G2 as zg_g2_*, scalars Montgomery Fr, a GT value uint64_t[48] as in
 *     the pairing section; a G1 RESULT is xy[8] followed by a flag word (1 = identity, written x = y = 0), a G2 result xy[16] followed
 *     by a flag word (identity written as G2Point.identity()), as zg_msm_g1_batch_dev / zg_msm_g2_dev write them.
 *   - every value is the reference's, bit for bit, under zg_multi_pairing's argument (one final exponentiation per product).
 *   - the calls of one session must come in the order begin, { first, second, fold } x sigma, final; anything else returns ZG_ERR_INVALID
 *     and changes nothing. zg_dory_open_close may come at any point. A session belongs to one host thread at a time. */
typedef struct zg_dory_s *zg_dory_t;
#define ZG_DORY_VMV_WORDS 105    /* c[48], d2[48], e1[9] */
#define ZG_DORY_FIRST_WORDS 218  /* d1_left[48], d1_right[48], d2_left[48], d2_right[48], e1_beta[9], e2_beta[17] */
#define ZG_DORY_SECOND_WORDS 148 /* c_plus[48], c_minus[48], e1_plus[9], e1_minus[9], e2_plus[17], e2_minus[17] */
#define ZG_DORY_FINAL_WORDS 26   /* final_e1[9], final_e2[17] */
/* g1_vec / g2_vec: n_gens >= 2^sigma entries each, the first 2^sigma are used (flags may be NULL); rows: n_rows row commitments (flags may
 * be NULL; truncated, or padded with identities, to 2^sigma for v1 and to 2^nu for e1); v_vec: n_v <= 2^sigma scalars; right_vec: 2^sigma,
 * left_vec: 2^nu scalars. nu <= sigma <= 20 (the reference's setup only makes sigma >= nu and indexes the generators up to 2^sigma; the
 * session runs sigma rounds), ZG_ERR_INVALID otherwise, as for short generator vectors and missing data. Writes the VMV message (:1456-1495):
 * c = e(MSM(v1, v_vec), g2_vec[0]), d2 = e(MSM(g1_vec[0..n_v], v_vec), g2_vec[0]), e1 = MSM(rows to 2^nu, left_vec). */
ZG_API int zg_dory_open_begin(const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n_gens,
                              const uint64_t *rows_xy, const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec, size_t n_v,
                              const uint64_t *right_vec, const uint64_t *left_vec, uint32_t nu, uint32_t sigma,
                              uint64_t *out_vmv /* ZG_DORY_VMV_WORDS */, zg_dory_t *out);
/* the current round's first reduce message (:1549-1554) over the live length cur = 2^(sigma - round) */
ZG_API int zg_dory_open_first_message(zg_dory_t s, uint64_t *out /* ZG_DORY_FIRST_WORDS */);
/* applies the first challenge — v1[i] += beta * g1_vec[i], v2[i] += beta_inv * g2_vec[i] (:1578-1584), both scalars exactly as given —
 * and returns the second reduce message (:1587-1592) */
ZG_API int zg_dory_open_second_message(zg_dory_t s, const uint64_t beta[4], const uint64_t beta_inv[4], uint64_t *out /* ZG_DORY_SECOND_WORDS */);
/* folds v1 and s1 by alpha, v2 and s2 by alpha_inv and halves the length (:1615-1634). ASYNCHRONOUS: one launch is enqueued */
ZG_API int zg_dory_open_fold(zg_dory_t s, const uint64_t alpha[4], const uint64_t alpha_inv[4]);
/* the scalar-product message (:1641-1655): final_e1 = v1[0] + (gamma * s1[0]) G, final_e2 = v2[0] + (gamma_inv * s2[0]) H with the two
 * generators of the reference; the products with s1[0] / s2[0] are formed on the device, which alone holds them */
ZG_API int zg_dory_open_final(zg_dory_t s, const uint64_t gamma[4], const uint64_t gamma_inv[4], uint64_t *out /* ZG_DORY_FINAL_WORDS */);
ZG_API size_t zg_dory_open_len(zg_dory_t s); /* the live length: 2^sigma after begin, halved by every fold; 0 for NULL */
ZG_API int zg_dory_open_close(zg_dory_t s);  /* waits for the session's work and returns its buffers to the device pool; NULL is fine */

/* ------------------------------------------------------------------ Dory commitments (key and batch) */
/* DoryCommitmentScheme.commit (src/poly/commitment/dory.zig:989-1042) for ALL the polynomials of a proof in one call
 * (proveJoltCompatibleWithDoryAndSrsAtAddress commits about forty, src/zkvm/mod.zig:847-961), over a key that stays in HBM. What is
 * committed there is mostly small integers — 4-bit chunks of one column per cycle, two columns of signed 64-bit increments — so the
 * row commitments of those kinds are not MSMs over 255-bit scalars but SUMS OF TABLE ENTRIES: the key holds T[c][d] = d * g1_vec[c]
 * for d = 1..255, and row r of an 8-bit polynomial is sum_c T[c][digit(r, c)]; a 64-bit polynomial is eight such sums and
 * 56 doublings. Every row of every polynomial then goes through ONE pairing launch set against the key's g2_vec.
 *   - layout of a polynomial of `len` entries (the reference derives it from the length): num_vars = floor(log2 len), 1 for len <= 1;
 *     sigma = (num_vars + 1) / 2 columns bits, nu = num_vars - sigma row bits; the first 2^num_vars entries are read (one entry for
 *     len = 1); len = 0 gives GT one; rows >= n_g2 are left out of the product (:1030); 2^sigma > n_g1 is ZG_ERR_INVALID.
 *   - values are the reference's, bit for bit: GT canonical as in the pairing section, rows as zg_msm_g1_batch_dev writes them. */
typedef struct zg_dory_key_s *zg_dory_key_t;
#define ZG_DORY_POLY_FR 0        /* Montgomery Fr elements, 4 words each: rows through the fused batch MSM over the key's own handle */
#define ZG_DORY_POLY_U64 1       /* F.fromU64(word); aux (optional) one byte per entry, 1 = the entry is F.fromU64(word).neg() */
#define ZG_DORY_POLY_CHUNK64 2   /* F.fromU64((entry >> shift) & (2^bits - 1)) of a column of 64-bit integers, 1 <= bits <= 8 */
#define ZG_DORY_POLY_CHUNK128 3  /* the same of a column of 128-bit little-endian integers (2 words each); a field may straddle the words */
/* uploads both generator vectors (flags may be NULL) and builds the digit table in HBM: 255 * n_g1 * 64 bytes (16 MB at n_g1 = 2^10),
 * plus an MSM handle over g1_vec for ZG_DORY_POLY_FR. 1 <= n_g1 <= 2^16; n_g2 may be 0. An identity generator contributes nothing. */
ZG_API int zg_dory_key_create(const uint64_t *g1_xy, const uint8_t *g1_inf, size_t n_g1, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n_g2,
                              zg_dory_key_t *out);
ZG_API int zg_dory_key_free(zg_dory_key_t key); /* waits for the device; NULL is fine; ZG_ERR_INVALID while an opening session over it is open */
ZG_API int zg_dory_key_len(zg_dory_key_t key, size_t *n_g1, size_t *n_g2); /* either pointer may be NULL */
/* k polynomials: kinds[j], data[j] (lens[j] entries of 4 / 1 / 1 / 2 words), aux[j] (ZG_DORY_POLY_U64 only; aux or aux[j] may be NULL),
 * shifts[j] / bits[j] (the CHUNK kinds only; both arrays may be NULL when there is none; shift + bits beyond the width is
 * ZG_ERR_INVALID). Polynomials that name the same data pointer, kind width and length are uploaded once. out_gt: k GT elements.
 * out_rows (may be NULL): the row commitments of all polynomials back to back as 9-word records (xy[8], flag word: 1 = identity, written
 * x = y = 0), polynomial j's 2^nu_j records (none for len = 0) from record out_rows_off[j] on; out_rows_off (may be NULL): k + 1 offsets.
 * These are the rows openWithRowCommitments / zg_dory_open_begin take. On an error nothing is written. */
ZG_API int zg_dory_commit_batch(zg_dory_key_t key, size_t k, const uint32_t *kinds, const uint64_t *const *data, const uint8_t *const *aux,
                                const size_t *lens, const uint32_t *shifts, const uint32_t *bits, uint64_t *out_gt /* k*48 */,
                                uint64_t *out_rows, uint64_t *out_rows_off /* k+1 */);
/* same with data[j], aux[j], d_out_gt and d_out_rows in DEVICE memory (the arrays kinds .. bits and out_rows_off stay the host's); the
 * launch set runs on `stream`, ordered after the work already enqueued there, and the call returns once the outputs are written. */
ZG_API int zg_dory_commit_batch_dev(zg_dory_key_t key, size_t k, const uint32_t *kinds, const uint64_t *const *data, const uint8_t *const *aux,
                                    const size_t *lens, const uint32_t *shifts, const uint32_t *bits, void *stream, uint64_t *d_out_gt /* k*48 */,
                                    uint64_t *d_out_rows, uint64_t *out_rows_off /* k+1 */);

/* ------------------------------------------------------------------ Dory verifier setup */
/* DoryVerifierSetup.fromSRS (src/zkvm/preprocessing.zig:889-973), which `zolt prove` runs whenever it exports its preprocessing
 * (src/main.zig:431-489, :630-692), for ALL levels at once: with K = floor(log2 n_g1) and h = 2^(k-1),
 *   chi[0]      = e(g1_vec[0], g2_vec[0])                                   (:914)
 *   chi[k]      = chi[k-1] * multiPair(g1_vec[h..2h), g2_vec[h..2h))        (:935)
 *   delta_1r[k] = multiPair(g1_vec[h..2h), g2_vec[0..h))                    (:929)       delta_1r[0] = one (:906)
 *   delta_2r[k] = multiPair(g1_vec[0..h), g2_vec[h..2h))                    (:932)       delta_2r[0] = one (:907)
 * for k = 1..K — 3 * 2^K - 2 pairings, which the reference runs one after another with a final exponentiation each (multiPair, :833-850).
 * Here they are ONE launch set over the generators where they lie: a Miller lane per pair, one segmented product, the running product
 * of the chi values, and 3K + 1 final exponentiations. delta_1l = delta_2l = (one, chi[0..K-1]) (:905, :926, :940-945) and ht = chi[0]
 * (:950-957) are copies of these values: the host mirrors make them, the library does not write them.
 *   - out_gt: three arrays of `levels` = K + 1 GT elements back to back — chi[0..K], delta_1r[0..K], delta_2r[0..K] — in the GT layout of
 *     the pairing section. Values are the reference's, bit for bit, under zg_multi_pairing's argument; a pair with an identity on
 *     either side contributes one (multiPair's `continue`, :839; pairingFp's own rule for chi[0]), a Miller value of zero is stored as one.
 *   - only the first 2^K generators of either vector are read; n_g1 need not be a power of two and n_g2 may exceed 2^K.
 *   - ZG_ERR_INVALID, with nothing written: a NULL key or NULL points; n_g1 = 0 or n_g1 > 2^16; n_g2 < 2^K (the reference would slice
 *     g2_vec out of bounds); levels_cap < K + 1; a NULL out_gt.
 * The calls return once the outputs are written (their scratch is pooled), as zg_dory_commit_batch does. */
/* levels = K + 1, K = floor(log2 n_g1): what fromSRS calls max_num_rounds + 1 (:890, :902); 0 for n_g1 = 0. Pure host arithmetic. */
ZG_API size_t zg_dory_verifier_setup_levels(size_t n_g1);
/* fromSRS (:889-973) over a resident key (zg_dory_key_create): nothing is uploaded but the segment table, the key is only read.
 * out_levels (may be NULL) receives K + 1. */
ZG_API int zg_dory_verifier_setup(zg_dory_key_t key, uint64_t *out_gt /* 3 * levels * 48 */, size_t levels_cap, size_t *out_levels);
/* the same from host points (flags may be NULL), for a caller that builds the SRS only for this, as src/main.zig:431-489 does: no digit
 * table and no MSM handle are built; the first 2^K points of either vector cross once. */
ZG_API int zg_dory_verifier_setup_points(const uint64_t *g1_xy, const uint8_t *g1_inf, size_t n_g1, const uint64_t *g2_xy, const uint8_t *g2_inf,
                                         size_t n_g2, uint64_t *out_gt /* 3 * levels * 48 */, size_t levels_cap, size_t *out_levels);

/* ------------------------------------------------------------------ Dory opening (over a key, `open`) */
/* DoryCommitmentScheme.open -> openWithRowCommitments (src/poly/commitment/dory.zig:1052-1378): the opening `zolt prove` runs, called
 * from serializeJoltProof / serializeJoltProofWithDory (src/zkvm/mod.zig:1374, :1485) over setup(log_size). It differs from
 * openWithTranscript, which the session section above restates, in its SHAPES: setup makes 2^sigma G1 and only 2^nu G2 generators
 * (nu = sigma - 1 for every odd log_size) and open carries two live lengths, current_col_len and current_row_len (:1211-1214,
 * :1236-1252, :1279-1304, :1321-1344). With nu <= sigma, round t has cur = 2^(sigma - t), n2 = cur / 2, row = max(2^nu >> t, 1),
 * h = min(n2, row) and
 *   first message (:1245-1261)  d1_left = <v1[0..h), g2[0..h)>, d1_right = <v1[n2..n2+h), g2[0..h)>, d2_left = <g1[0..n2), v2[0..n2)>,
 *                               d2_right = <g1[0..n2), v2[n2..cur)>, e1_beta = MSM(g1[0..cur), s2[0..cur)), e2_beta = msmG2(g2[0..row), s1[0..row))
 *   update (:1279-1286)         v1[i] += beta g1[i] for i < cur; v2[i] += beta_inv g2[i] for i < row only
 *   second message (:1291-1304) c_plus = <v1[0..h), v2[n2..n2+h)>, c_minus = <v1[n2..n2+h), v2[0..h)> (multiPairG1G2's own @min rule,
 *                               :673-690), e1_plus = MSM(v1[0..n2), s2[n2..cur)), e1_minus = MSM(v1[n2..cur), s2[0..n2)),
 *                               e2_plus = msmG2(v2[n2..n2+h), s1[0..h)), e2_minus = msmG2(v2[0..h), s1[n2..n2+h))
 *   fold (:1321-1344)           v1 and s2 over n2 entries by alpha / alpha_inv, v2 and s1 over h entries by alpha_inv / alpha; row
 *                               halves while it is above 1
 * (one function, dory_round_shape of zolt_amd/csrc/dory_shape.h, holds these lengths). The VMV message, v1, v2, s1, s2 and the final
 * message are the session section's. open's challenges are constants — beta = round + 1, alpha = round + 100, gamma = 999 (:1274,
 * :1316, :1349) — so no transcript sits between the messages and zg_dory_open_run enqueues the whole proof at once. */
/* Begins a session over a resident key (zg_dory_key_create): the generators and the MSM handle are read where the key holds them —
 * nothing of them is uploaded or copied, no handle is built. Requires key.n_g1 >= 2^sigma, key.n_g2 >= 2^nu and nu <= sigma <= 20
 * (nu > sigma: the reference would index v1_work past 2^sigma); ZG_ERR_INVALID otherwise, with nothing written. The other arguments
 * and the VMV message are zg_dory_open_begin's. The session runs the schedule above through zg_dory_open_first_message ..
 * zg_dory_open_close. It holds a reference on the key: zg_dory_key_free of a key with an open session returns ZG_ERR_INVALID and frees
 * nothing. The key is only read; several sessions may be open over one key. */
ZG_API int zg_dory_open_key_begin(zg_dory_key_t key, const uint64_t *rows_xy, const uint8_t *rows_inf, size_t n_rows, const uint64_t *v_vec,
                                  size_t n_v, const uint64_t *right_vec, const uint64_t *left_vec, uint32_t nu, uint32_t sigma,
                                  uint64_t *out_vmv /* ZG_DORY_VMV_WORDS */, zg_dory_t *out);
/* All sigma rounds and the final message of a session begun either way, in one call: every round's launches go onto the session's
 * stream back to back, the messages are staged on the device in per-message areas allocated at begin, and ONE copy and ONE host
 * synchronisation end the call. challenges: (beta, beta_inv, alpha, alpha_inv) per round, then (gamma, gamma_inv) — 16 sigma + 8 words,
 * Montgomery Fr, each taken exactly as given. Callable only right after begin (ZG_ERR_INVALID at any other point, with nothing
 * changed); the session is finished afterwards (zg_dory_open_len = 1) and only zg_dory_open_close remains. sigma = 0: only the final
 * message is written; out_first / out_second may then be NULL. The records are those of the stepwise calls, bit for bit. */
ZG_API int zg_dory_open_run(zg_dory_t s, const uint64_t *challenges, uint64_t *out_first /* sigma * ZG_DORY_FIRST_WORDS */,
                            uint64_t *out_second /* sigma * ZG_DORY_SECOND_WORDS */, uint64_t *out_final /* ZG_DORY_FINAL_WORDS */);

/* ------------------------------------------------------------------ Pairings (engine) */
/* Which kernels compute the Miller loops and the final exponentiations of every section above. Both engines give the same bits: every
 * value is a canonical field element. The setting is process-wide, one atomic integer without a device behind it: it can be set before
 * zg_init and after zg_shutdown. It starts as LANE, or as WAVE where the environment has ZG_PAIRING_ENGINE=wave when the library first
 * reads it. Every call reads it once, at entry; a Dory opening session reads it at zg_dory_open_begin and keeps that engine until it is
 * closed. Honoured by zg_miller_loop_batch, zg_pairing_batch, zg_final_exponentiation_batch, zg_multi_pairing[_dev], the opening
 * session, zg_dory_commit_batch[_dev] and zg_dory_verifier_setup[_points]. */
#define ZG_PAIRING_ENGINE_LANE 0   /* a lane per pair / per product: the kernels of "Pairings (Dory)", unchanged; the default */
#define ZG_PAIRING_ENGINE_WAVE 1   /* a wavefront per pair / per product */
ZG_API int zg_pairing_engine_set(int engine);   /* ZG_OK, or ZG_ERR_INVALID for any other value (the engine is then unchanged) */
ZG_API int zg_pairing_engine_get(void);

/* ------------------------------------------------------------------ Points from bytes */
/* Keys, proofs and preprocessing files hold points as BYTES: the HyperKZG key of `zolt srs` / loadFromRawBinary / loadFromPtau
 * (src/poly/commitment/srs.zig:264-306, :733-900), the Jolt-exported Dory SRS of `zolt prove --srs FILE`
 * (DoryCommitmentScheme.loadFromFile, src/poly/commitment/dory.zig:752-924), the compressed points of proofs (compressG1 / compressG2,
 * dory.zig:51-76, :179-210; serializeG1 / serializeG2, src/zkvm/preprocessing.zig:1061-1127). These calls decode them on the device,
 * one lane per record: the bytes cross once, byte order, identity rule, Montgomery conversion, the on-curve check and — for compressed
 * records — the square root in Fp or Fp2 run in one launch, and the handle calls build their handle from what lies in HBM: no point
 * returns to the host. Record sizes G1 / G2:
 *   ZG_POINT_BYTES_BE              64 / 128   G1: x, y big-endian. G2: x.c1, x.c0, y.c1, y.c0, each big-endian. Identity = every byte zero
 *                                             (parseG1Uncompressed / parseG2Uncompressed, srs.zig:65-99, :165-203)
 *   ZG_POINT_BYTES_LE              64 / 128   G1: x, y little-endian. G2: x.c0, x.c1, y.c0, y.c1 little-endian. Identity = every byte zero
 *                                             (parseG1LE / parseG2LE, srs.zig:616-712)
 *   ZG_POINT_BYTES_ARK             64 / 128   as LE, with the two top bits of the record's last byte cleared first; identity = every byte
 *                                             zero after that (dory.zig:828-924)
 *   ZG_POINT_BYTES_ARK_COMPRESSED  32 / 64    x little-endian (G2: x.c0, x.c1); flag = last byte & 0xC0: 0x40 exactly is the identity, the
 *                                             stored sign is positive iff flag == 0 (y is positive when y <= -y as canonical integers, Fp2
 *                                             comparing c1 first), x is taken with the two bits cleared (decompressG1 / decompressG2,
 *                                             dory.zig:81-120, :214-261)
 * A coordinate is reduced and converted as ZG_OP_TO_MONT does it, so a coordinate >= p gives the words zg_field_op gives. An identity is
 * written as the group's identity (G1 x = y = 0; G2 x = 0, y = one) with its flag byte 1. ZG_POINT_BYTES_CHECK: a non-identity
 * uncompressed point that is not on its curve is a bad record (PointNotOnCurve) — the reference checks G1 in BE and LE, never G2, never
 * ARK. A compressed record whose x has no y is a bad record (DecompressionFailed) with or without the flag. G2 subgroup membership is
 * not checked (the reference has no such check).
 * Deviations from the reference: its ARK G2 parser has no identity rule (an all-zero record becomes (0, 0), on no curve) — here it is the
 * identity; parseG1Compressed (srs.zig:102-162) is left out: its 48-byte layout is another curve's, its square root's exponent is not
 * (p + 1) / 4 and nothing calls it.
 *   - all pointers are HOST pointers. On success *first_bad (may be NULL) = n. On a bad record the call returns ZG_ERR_INVALID, *first_bad
 *     is the SMALLEST bad index, zg_last_error() names index and reason, nothing else is written and no handle is made; the launch is not
 *     cut short and the library stays usable.
 *   - n = 0: ZG_OK and nothing written for the two point calls, ZG_ERR_INVALID for the two handle calls. ZG_ERR_INVALID also for an
 *     unknown encoding, unknown flag bits, NULL data with n > 0, more than 2^28 records. */
#define ZG_POINT_BYTES_BE 0
#define ZG_POINT_BYTES_LE 1
#define ZG_POINT_BYTES_ARK 2
#define ZG_POINT_BYTES_ARK_COMPRESSED 3
#define ZG_POINT_BYTES_CHECK 1u
ZG_API int zg_g1_points_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy /* n*8 */,
                                   uint8_t *out_inf /* n, may be NULL */, size_t *first_bad /* may be NULL */);
ZG_API int zg_g2_points_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, uint64_t *out_xy /* n*16 */,
                                   uint8_t *out_inf /* n, may be NULL */, size_t *first_bad /* may be NULL */);
/* zg_g1_bases_upload over the decoded points, which stay in HBM: the handle is the one zg_g1_bases_upload builds from them */
ZG_API int zg_g1_bases_from_bytes(const uint8_t *bytes, size_t n, uint32_t encoding, uint32_t flags, const zg_msm_config *cfg, zg_bases_t *out,
                                  size_t *first_bad);
/* zg_dory_key_create over both decoded vectors (its bounds: 1 <= n_g1 <= 2^16, n_g2 <= 2^24; g2_bytes may be NULL for n_g2 = 0); flags
 * apply to both. *first_bad: a G1 index, or n_g1 + a G2 index; n_g1 + n_g2 on success. */
ZG_API int zg_dory_key_from_bytes(const uint8_t *g1_bytes, size_t n_g1, uint32_t g1_encoding, const uint8_t *g2_bytes, size_t n_g2,
                                  uint32_t g2_encoding, uint32_t flags, zg_dory_key_t *out, size_t *first_bad);

/* ------------------------------------------------------------------ poly tables */
/* EqPolynomial.evals / evalsSliceWithScaling (src/poly/mod.zig:240-290): out[2^v], index MSB <-> r[0];
 * scale may be NULL (= one). Identical values to GruenSplitEqPolynomial's tables
 * (src/poly/split_eq.zig:122-171). */
ZG_API int zg_fr_eq_table(const uint64_t *r, size_t v, const uint64_t *scale, uint64_t *out);
/* device output; ASYNCHRONOUS: one launch on `stream`, r and scale travel as kernel arguments (nothing of the caller's is read
 * after the call returns, no upload precedes the kernel). v <= 34. */
ZG_API int zg_fr_eq_table_dev(const uint64_t *r_host, size_t v, const uint64_t *scale_host, uint64_t *d_out, void *stream);
/* The eq+1 evaluation table of EqPlusOnePrefixSuffixPoly (src/poly/mod.zig:462-560, computeEqPlusOneEvals :530-548; the same helper in
 * src/zkvm/spartan/stage3_prover.zig:1878-1894): out[j] = EqPlusOnePolynomial.mle(r, bits(j)), r[0] <-> MSB, 2^v entries. Over the
 * boolean cube eq+1(r, j) = eq(r, j - 1) and out[0] = 0, so this is the eq table moved up by one entry (the reference evaluates the
 * general formula, v^2 products per entry). */
ZG_API int zg_fr_eq_plus_one_table(const uint64_t *r, size_t v, uint64_t *out);
ZG_API int zg_fr_eq_plus_one_table_dev(const uint64_t *r_host, size_t v, uint64_t *d_out, void *stream);
/* GruenSplitEqPolynomial.initWithScaling's prefix-table set in one launch (src/poly/split_eq.zig:122-171: E_out_vec / E_in_vec,
 * "append the new variable as LSB" and KEEP every level): out holds the v+1 tables eq(tau[0..k), .), k = 0..v, back to back —
 * table k has 2^k entries and starts at element 2^k - 1 (so out has 2^(v+1) - 1 elements; table 0 is [1]); within a table
 * tau[0] <-> MSB of the index. The caller passes tau[0..m) for E_out_vec and tau[m..n-1) for E_in_vec (:91-93). v <= 24. */
ZG_API int zg_fr_eq_prefix_tables(const uint64_t *tau, size_t v, uint64_t *out /* (2^(v+1)-1)*4 */);
ZG_API int zg_fr_eq_prefix_tables_dev(const uint64_t *tau_host, size_t v, uint64_t *d_out, void *stream);
/* DensePolynomial.evaluate (src/poly/mod.zig:73-92): sum_i evals[i] * prod_j (bit_j(i) ? point[j] : 1 - point[j]),
 * index bit j <-> point[j] (LSB first). The reference expands every term (O(n*v) multiplications); here the
 * weights are one eq table (point reversed) and the sum is a device dot product — same field value. */
ZG_API int zg_fr_dense_evaluate(const uint64_t *evals, size_t num_vars, const uint64_t *point, uint64_t out[4]);
/* R1CSInputEvaluator.computeClaimedInputs (src/zkvm/r1cs/evaluation.zig:55-122) and the factor claims of
 * ProductVirtualRemainderProver.computeOpeningClaims (src/zkvm/spartan/product_remainder.zig:396-425): the MLE evaluation of k <= 64
 * column polynomials at one point from a CYCLE-MAJOR matrix (rows[t*k + i] = column i at cycle t, the layout of R1CSCycleInputs.values):
 * out[i] = sum_{t < min(n_rows, 2^v)} eq(r, t) * rows[t*k + i], eq = EqPolynomial(r).evals (r[0] <-> MSB of t). */
ZG_API int zg_fr_rows_mle(const uint64_t *rows, size_t n_rows, size_t k, const uint64_t *r, size_t v, uint64_t *out /* k*4 */);
ZG_API int zg_fr_rows_mle_dev(const uint64_t *d_rows, size_t n_rows, size_t k, const uint64_t *r_host, size_t v, void *stream,
                       uint64_t *out /* host, k*4 */);
/* StreamingOuterProver.materializeLinearPhasePolynomials (src/zkvm/spartan/streaming_outer.zig:258-372): per cycle, Az and Bz of the two
 * constraint groups are Lagrange-weighted sums of the 19 uniform constraints' linear combinations (src/zkvm/r1cs/constraints.zig:248-531)
 * — AFFINE maps of the cycle's R1CS inputs. Generic form, over the same cycle-major matrix zg_fr_rows_mle reads (k <= 64 columns):
 *     table t, element i * g + j  =  C[t*g + j][k] + sum_{col < k} C[t*g + j][col] * rows[i*stride + col] i < n_rows
 *                                 =  0                                                                     n_rows <= i < n_pad
 * coeffs: (ntab * g) rows of k + 1 elements (the last one the constant), host memory; ntab * g <= 16. For the outer prover ntab = 2
 * (Az, Bz), g = 2 (the group selector is the lowest variable), coefficient rows (az0, az1, bz0, bz1), n_pad = the padded trace length.
 * stride: elements between the starts of consecutive rows, 0 = k. With stride < k a map is a SLIDING WINDOW over the matrix — row i's
 * columns stride .. k-1 are the first columns of the rows after it, the matrix must hold (n_rows - 1) * stride + k elements — which is how
 * ProductVirtualRemainderProver's fused right factor reads the NEXT cycle's IsNoop flag (src/zkvm/spartan/product_remainder.zig:436-476). */
ZG_API int zg_fr_rows_affine(const uint64_t *rows, size_t n_rows, size_t k, size_t stride, const uint64_t *coeffs, size_t ntab, size_t g, size_t n_pad,
                      uint64_t *const *tables /* ntab host pointers, n_pad * g elements each */);
ZG_API int zg_fr_rows_affine_dev(const uint64_t *d_rows, size_t n_rows, size_t k, size_t stride, const uint64_t *coeffs_host, size_t ntab, size_t g,
                          size_t n_pad, uint64_t *const *d_tables /* host array of ntab DEVICE pointers */, void *stream);
/* The same affine maps written as RECORDS: d_out[(i * record + first + c) * 4 ..] = map_c(row_i) for c < nout <= 16 consecutive positions of a
 * record of `record` elements per row. JoltR1CS.computeAz / computeBz (src/zkvm/r1cs/jolt_r1cs.zig:143-190) lay the 19 uniform constraints
 * of a cycle out this way (constraint_idx = cycle * 19 + i): two calls per vector (constraints 0..15, 16..18) fill it in place; the zero
 * padding up to the power of two is the caller's (a cleared buffer). coeffs_host: nout x (k + 1) elements, the constant last. */
ZG_API int zg_fr_rows_affine_records_dev(const uint64_t *d_rows, size_t n_rows, size_t k, size_t stride, const uint64_t *coeffs_host, size_t nout,
                                         size_t record, size_t first, uint64_t *d_out, void *stream);
/* LtPolynomial over the cube (src/zkvm/ram/val_evaluation.zig:289-330), the third factor of ValEvaluationProver's inc * wa * lt:
 * out[j] = sum over the ZERO bits i of j of r[i] * prod_{k > i} (bit_k(j) ? r[k] : 1 - r[k]); index bit i <-> r[i]. v <= 30. */
/* The witness matrix of a stage built ON THE DEVICE from integer columns. The reference derives every R1CS input of a cycle from machine
 * integers — F.fromU64 of a register / memory / pc value, signedI64ToField of an immediate, a 0/1 flag, the field product of two inputs
 * (R1CSCycleInputs.fromTraceStep, src/zkvm/r1cs/constraints.zig:929-1223, signedI64ToField :868-876) — and the provers then read the
 * 32-byte elements (R1CSInputEvaluator.computeClaimedInputs, src/zkvm/r1cs/evaluation.zig:55-122; StreamingOuterProver,
 * src/zkvm/spartan/streaming_outer.zig:258-372). A host hands the columns over as they are (~180 instead of 1376 bytes per cycle
 * across PCIe) and d_rows[row * n_cols + c] = the column's value at `row` as a canonical Montgomery Fr element, bit for bit what the
 * reference's conversions produce. One array per column, n_rows values each:
 *   ZG_COL_ZERO  no data: the column is zero              ZG_COL_U8 / U32 / U64  unsigned integers -> F.fromU64
 *   ZG_COL_I64   int64_t: v < 0 -> r - |v|                ZG_COL_I128 / U128     16 bytes per row (lo, hi), two's complement / unsigned
 *   ZG_COL_FR    a Montgomery element per row, copied     ZG_COL_BIT             bit `a` of a packed flag word of `b` = 1, 4 or 8 bytes
 *   ZG_COL_MUL   the product of columns a and b of the same row, plus — when data is given — a           per row -> 0 or F.one()
 *                128-bit two's-complement addend per row. A factor may itself be a ZG_COL_MUL column whose factors are plain columns
 *                (RightLookupOperand = Product * FlagMultiplyOperands + the sum / difference of the other rows), no deeper.
 *   ZG_COL_LUT   data = an index per row (a = 1, 2 or 4 bytes each), aux = a table of b Montgomery elements: the value is table[index]
 *                (an index >= b reads as zero) — eq_evals[j] = table[rd(j)] of proveStage5, src/zkvm/prover.zig:880-900
 * Several ZG_COL_BIT columns may name the same word array (it crosses once). n_cols <= 64. */
#define ZG_COL_ZERO 0
#define ZG_COL_U8 1
#define ZG_COL_U32 2
#define ZG_COL_U64 3
#define ZG_COL_I64 4
#define ZG_COL_I128 5
#define ZG_COL_U128 6
#define ZG_COL_FR 7
#define ZG_COL_BIT 8
#define ZG_COL_MUL 9
#define ZG_COL_LUT 10
typedef struct {
    uint32_t kind; /* ZG_COL_* */
    uint32_t a, b; /* ZG_COL_BIT: bit index, bytes per word; ZG_COL_MUL: the two factor columns (data: optional addend); ZG_COL_LUT: bytes per index, table length */
    const void *data;
    const void *aux; /* ZG_COL_LUT: the table (b elements); NULL otherwise */
} zg_col_t;
/* host columns (pageable, or pinned from zg_host_alloc); returns when the matrix is complete */
ZG_API int zg_fr_rows_from_columns(const zg_col_t *cols, size_t n_cols, size_t n_rows, uint64_t *d_rows /* device, n_rows*n_cols*4 */);
/* columns already in HBM (data = device addresses); one asynchronous launch */
ZG_API int zg_fr_rows_from_columns_dev(const zg_col_t *cols, size_t n_cols, size_t n_rows, uint64_t *d_rows, void *stream);

ZG_API int zg_fr_lt_table(const uint64_t *r, size_t v, uint64_t *out /* 2^v * 4 */);
ZG_API int zg_fr_lt_table_dev(const uint64_t *r_host, size_t v, uint64_t *d_out, void *stream);
/* ValEvaluation's other two tables from the LIST OF WRITES (the prover's stage 4, src/zkvm/prover.zig:760-800 over
 * ram/val_evaluation.zig:298-345): d_inc[cycle[i]] = F.fromU64(post[i]) - F.fromU64(pre[i]) and d_wa[cycle[i]] = eq(r_eq, word[i] mod 2^log_k)
 * for the m writes, zero elsewhere (n entries each, DEVICE). r_eq is the point in EqPolynomial order (the reference passes r_address
 * reversed). The cycles must be distinct — a repeated or out-of-range cycle is refused (ZG_ERR_INVALID); the caller keeps the last write of a
 * cycle, as the reference's loop does by overwriting.
 * Returns after the work has completed: 24 bytes per write cross the boundary instead of two n-element tables. */
ZG_API int zg_fr_write_tables_dev(size_t n, size_t m, const uint32_t *cycle, const uint32_t *word, const uint64_t *pre, const uint64_t *post,
                           const uint64_t *r_eq, size_t log_k, uint64_t *d_inc, uint64_t *d_wa, void *stream);
/* The Q tables of Stage 3's prefix / suffix provers (ShiftPrefixSuffixProver.init, src/zkvm/spartan/stage3_prover.zig:1066-1112;
 * RegistersPrefixSuffixProver.init, :2232-2290): Q[x_lo] = sum over x_hi of witness(x_lo + x_hi * 2^prefix_vars) * suffix[x_hi] — column
 * sums of the cycle-length table read as a (rows = 2^suffix_vars) x (cols = 2^prefix_vars) matrix, under up to four weight vectors at
 * once (eq and eq+1 suffixes share the pass):   out[k * cols + c] = sum_r weights[k * rows + r] * table[r * cols + c],  k < m <= 4.
 * The _dev form is enqueued on `stream`; when the rows are cut into slabs (more than one) it also waits for the stream, because the
 * slab partials live in the library's scratch cache. */
ZG_API int zg_fr_weighted_colsum(const uint64_t *table, size_t rows, size_t cols, const uint64_t *weights, size_t m, uint64_t *out);
ZG_API int zg_fr_weighted_colsum_dev(const uint64_t *d_table, size_t rows, size_t cols, const uint64_t *d_weights, size_t m, uint64_t *d_out,
                              void *stream);
/* StreamingOuterProver.computeFirstRoundPoly's extended evaluations (src/zkvm/spartan/streaming_outer.zig:523-597, evaluateAzBzAtTargetY
 * :599-671): for each UniSkip target Y_j and constraint group, Az(x, Y_j) and Bz(x, Y_j) are Lagrange extrapolations (COEFFS_PER_J,
 * src/zkvm/r1cs/univariate_skip.zig:469-476) of the group's constraint values — affine maps of the cycle's inputs — and
 * t1(Y_j) = sum_{cycle, group} eq(tau_low, (cycle, group)) * Az * Bz. Generic form over the cycle-major matrix:
 *     out[p] = sum_{i < n_rows} W[i * g + p % g] * A_p(rows[i]) * B_p(rows[i]),     p < npairs <= 32,
 * A_p / B_p = coefficient rows 2p / 2p + 1 (k + 1 elements each, the constant last; host memory); W: DEVICE table of n_rows * g weights
 * (for the outer prover g = 2 and W = zg_fr_eq_table_dev(tau_low): index = cycle * 2 + group; pairs ordered (target, group)). */
ZG_API int zg_fr_rows_affine_prodsum_dev(const uint64_t *d_rows, size_t n_rows, size_t k, size_t stride, const uint64_t *coeffs_host, size_t npairs,
                                  const uint64_t *d_weights, size_t g, uint64_t *out /* host, npairs * 4 */, void *stream);
/* DensePolynomial.bindLow, in place: t[i] = t[2i] + r*(t[2i+1]-t[2i]), len -> len/2 (src/poly/mod.zig:160-175) */
ZG_API int zg_fr_bind_low(uint64_t *table, size_t len, const uint64_t r[4]);
/* DensePolynomial.bindFirst: out[i] = (1-r)*t[i] + r*t[i+len/2] (src/poly/mod.zig:128-149) */
ZG_API int zg_fr_bind_high(const uint64_t *table, size_t len, const uint64_t r[4], uint64_t *out);
/* Spartan combine f[i] = eq[i]*(Az[i]*Bz[i] - Cz[i]) (src/zkvm/spartan/mod.zig:191-199) */
ZG_API int zg_fr_spartan_combine(const uint64_t *eq, const uint64_t *az, const uint64_t *bz, const uint64_t *cz, size_t n,
                          uint64_t *out);
ZG_API int zg_fr_spartan_combine_dev(const uint64_t *d_eq, const uint64_t *d_az, const uint64_t *d_bz, const uint64_t *d_cz,
                              size_t n, uint64_t *d_out, void *stream);

/* ------------------------------------------------------------------ sumcheck session */
/* A device-resident Sumcheck(F).Prover (src/subprotocols/mod.zig:50-134): the table stays in
 * HBM across rounds; per round only two field elements come back and one goes in.
 * layout ZG_SC_HIGH_HALF = bindFirst order (the generic prover, :112-122);
 *        ZG_SC_LOW_PAIR  = bindLow order (src/poly/mod.zig:160-175; zkvm/r1cs/jolt_r1cs.zig:470-477). */
#define ZG_SC_HIGH_HALF 0
#define ZG_SC_LOW_PAIR 1
typedef struct zg_sc_s *zg_sc_t;
ZG_API int zg_sumcheck_open(const uint64_t *evals, size_t len, int layout, zg_sc_t *s);
ZG_API int zg_sumcheck_open_dev(const uint64_t *d_evals, size_t len, int layout, void *stream, zg_sc_t *s); /* copies */
/* The same session WITHOUT the copy: the session reads the caller's table (never writes it) until its first bind has run — the caller
 * keeps d_evals alive and unchanged until a later call on the session has returned round sums or a final value (or zg_sync). Its own
 * buffers hold the folds only (len/2 + len/4 entries instead of len + len/2): Az and Bz of an outer sumcheck, 1 GB each at 2^20 cycles,
 * are bound alongside without a second copy in HBM. zg_sumcheck_bit_bind (an in-place bind) is refused before the first zg_sumcheck_bind. */
ZG_API int zg_sumcheck_open_dev_borrowed(const uint64_t *d_evals, size_t len, int layout, void *stream, zg_sc_t *out);
/* A session whose table is ONE integer column widened on the device (zg_fr_rows_from_columns' kinds; host data): entries [0, n_rows) from
 * the column, [n_rows, len) zero. The tables of proveStage5 (eq_evals[j] = table[rd of cycle j]: a ZG_COL_LUT over one byte per cycle) and
 * proveStage6 (all zero: ZG_COL_ZERO) are built this way without a 32-byte-per-cycle upload (src/zkvm/prover.zig:880-944, 1024-1097). */
ZG_API int zg_sumcheck_open_column(const zg_col_t *col, size_t n_rows, size_t len, int layout, zg_sc_t *s);
/* Spartan's first sumcheck instance in ONE pass (src/zkvm/spartan/mod.zig:182-206, then Sumcheck.Prover.init): opens a session
 * whose table is f[i] = eq(r, i) * (Az[i]*Bz[i] - Cz[i]) (eq as zg_fr_eq_table: r[0] <-> MSB, optional scale; Az, Bz, Cz: 2^v
 * device-resident elements; d_cz = NULL: Cz is identically zero, as JoltR1CS.computeCz leaves it, src/zkvm/r1cs/jolt_r1cs.zig:193-200)
 * with round 0's sums already computed; the eq table is never materialised, nothing is copied. */
ZG_API int zg_sumcheck_open_spartan_dev(const uint64_t *r /* host, v*4 */, size_t v, const uint64_t *scale /* host 4 or NULL */,
                                 const uint64_t *d_az, const uint64_t *d_bz, const uint64_t *d_cz, int layout, void *stream,
                                 zg_sc_t *s);
/* Prover.nextRound's two sums (:79-93): HIGH_HALF g0 = sum first half, g1 = sum second half;
 * LOW_PAIR g0 = sum even, g1 = sum odd (jolt_r1cs.zig:436-444). */
ZG_API int zg_sumcheck_round_sums(zg_sc_t s, uint64_t g0[4], uint64_t g1[4]);
/* Prover.receiveChallenge (:112-122): fold by r. The next round's sums are produced by the
 * same kernel and returned by the following zg_sumcheck_round_sums without another pass. */
ZG_API int zg_sumcheck_bind(zg_sc_t s, const uint64_t r[4]);
ZG_API size_t zg_sumcheck_len(zg_sc_t s);
ZG_API int zg_sumcheck_final(zg_sc_t s, uint64_t out[4]); /* getFinalEval (:130-133), needs len == 1 */
ZG_API int zg_sumcheck_read(zg_sc_t s, uint64_t *out_table); /* copy the current table to the host (tests) */
/* out[i] = table[idx[i]], i < n (every idx < the current length): what a SPARSE-entry prover reads of a dense table —
 * RamReadWriteCheckingProver's val_init checkpoints of the column pairs its entries touch (src/zkvm/ram/read_write_checking.zig:591-602,
 * 985-996) — instead of copying the table back every round. */
ZG_API int zg_sumcheck_gather(zg_sc_t s, const uint64_t *idx, size_t n, uint64_t *out /* n*4 */);
/* Sharded tables: the LOCAL pair g0||g1 (8 limbs) / the current local table, written to device
 * memory in stream order on the session's stream (the one given to zg_sumcheck_open_dev) with no host
 * synchronisation, so an RCCL all-gather enqueued on that stream can follow directly. */
ZG_API int zg_sumcheck_round_sums_dev(zg_sc_t s, uint64_t *d_out8);
ZG_API int zg_sumcheck_read_dev(zg_sc_t s, uint64_t *d_out_table);
ZG_API int zg_sumcheck_close(zg_sc_t s);
/* Prover fold sites beyond the generic Sumcheck.Prover. On a LOW_PAIR session holding RaPolynomial's table:
 * RafEvaluationProver.computeRoundPolynomialCubic's two sums (src/zkvm/ram/raf_checking.zig:335-410)
 *   s(0) = sum_i ra[2i] * u0(i),  s(2) = sum_i (2 ra[2i+1] - ra[2i]) * (u0(i) + 2 * current_power),
 *   u0(i) = base + 2 * current_power * i   (as field elements; `base` = start_address + 8 * sum_j bound_j 2^j, Montgomery),
 * in one pass over the table; s(1) = claim - s(0) and s(3) = s(0) - 3 s(1) + 3 s(2) are host scalar code, the fold of the round
 * (RaPolynomial.bind, :162-174) is zg_sumcheck_bind. */
ZG_API int zg_sumcheck_raf_round(zg_sc_t s, const uint64_t base[4], uint64_t current_power, uint64_t s0[4], uint64_t s2[4]);
/* RafEvaluationProver.computeInitialClaim (src/zkvm/ram/raf_checking.zig:312-321): claim = sum_k t[k] * F.fromU64(base + step * k) over the
 * session's current table (base = start_address, step = 8 for UnmapPolynomial :207-209); base + step * (len - 1) must fit 64 bits. */
ZG_API int zg_sumcheck_raf_claim(zg_sc_t s, uint64_t base, uint64_t step, uint64_t claim[4]);
/* LassoProver's eq_evals path on ONE session (src/zkvm/lasso/prover.zig:262-453): open the session with layout ZG_SC_HIGH_HALF over
 * the padded eq_evals (:153-171); the log_K address rounds use the two calls below, the log_T cycle rounds are the session's
 * ordinary round_sums / bind (:313-340,411-441). d_idx128: the u128 lookup indices in DEVICE memory (two little-endian u64 words
 * each; zg_dev_alloc + zg_memcpy_h2d), n_idx <= the session's length.
 *   bit_round = computeAddressRoundPoly's sum_0 / sum_1 (:283-293) over the first n_idx entries;
 *   bit_bind  = receiveChallenge's address branch (:375-399): entry j *= (bit of idx[j]) ? r : 1 - r, claim = sum of ALL entries.
 * bit_bind also leaves the next round's sums (bit + 1) behind, so the following bit_round costs no pass over the table (they are
 * keyed by d_idx128, n_idx and the bit: the index buffer's CONTENTS must stay unchanged between the two calls, as a prover's do). */
ZG_API int zg_sumcheck_bit_round(zg_sc_t s, const uint64_t *d_idx128, size_t n_idx, unsigned bit, uint64_t sum0[4], uint64_t sum1[4]);
ZG_API int zg_sumcheck_bit_bind(zg_sc_t s, const uint64_t *d_idx128, size_t n_idx, unsigned bit, const uint64_t r[4], uint64_t claim[4]);
/* LassoProver.computeAddressRoundPoly's two sums (src/zkvm/lasso/prover.zig:283-293): sum0 / sum1 = the sum of vals[j] over the
 * entries whose u128 lookup index (idx128: n x 2 little-endian u64 words) has bit `bit` clear / set. The _dev form keeps eq_evals
 * and the indices resident across the LOG_K address rounds. */
ZG_API int zg_fr_bit_split_sums(const uint64_t *vals, const uint64_t *idx128, size_t n, unsigned bit, uint64_t sum0[4], uint64_t sum1[4]);
ZG_API int zg_fr_bit_split_sums_dev(const uint64_t *d_vals, const uint64_t *d_idx128, size_t n, unsigned bit, void *stream, uint64_t sum0[4],
                             uint64_t sum1[4]);

/* Self-test of the round-ending hand-off every sumcheck-family kernel uses (block partials -> the workgroup that arrives last; the
 * reference's serial sums of src/subprotocols/mod.zig:79-93 have no counterpart): `iters` launches of `blocks` workgroups of `threads`
 * threads on the library's stream. Each workgroup first reads every partial line with PLAIN loads (its L1 then holds the previous
 * launch's bytes), waits an uneven, launch-dependent time, and hands in a pattern unique to (launch, workgroup); the last arriver
 * checks EVERY word it reads against the pattern. With busy != 0 a second stream streams through a 256 MiB buffer meanwhile.
 * Outputs: words that differed (must be 0) and launches that elected exactly one last arriver (must be iters). */
ZG_API int zg_selftest_handoff(unsigned blocks, unsigned threads, unsigned iters, int busy, uint64_t *mismatches, uint64_t *completed);

/* runSumcheck (src/subprotocols/mod.zig:302-354) with the WHOLE protocol on the device: the prover's sums and folds
 * (bindFirst order) and the reference's toy verifier (verifyRound / deriveChallenge, :165-243: the deterministic
 * 64-bit mixer, F.fromU64, claim <- p(challenge)) — the verifier step runs at the end of the kernel that produced the
 * round's sums, so no round crosses PCIe. len = 2^v (v >= 0). Outputs (host): claim[4]; rounds: v x (c0 || c1) =
 * Round.poly.coeffs [g(0), g(1) - g(0)]; challenges: v x 4 (= Proof.final_point); final_eval[4]; *result =
 * verifier.claim == final_eval. Returns ZG_ERR_VERIFY where the reference returns error.SumcheckVerificationFailed.
 * The input table is not modified. Provers driven by a host transcript (Keccak/Blake2b) use the session API above. */
ZG_API int zg_run_sumcheck_dev(const uint64_t *d_evals, size_t len, void *stream, uint64_t claim[4], uint64_t *rounds,
                               uint64_t *challenges, uint64_t final_eval[4], uint8_t *result);
ZG_API int zg_run_sumcheck(const uint64_t *evals, size_t len, uint64_t claim[4], uint64_t *rounds, uint64_t *challenges,
                           uint64_t final_eval[4], uint8_t *result);

/* ------------------------------------------------------------------ product-form sumcheck sessions */
/* The zkVM provers whose round polynomial is a sum over adjacent pairs of a PRODUCT of multilinear tables, all folded LowToHigh by
 * the same challenge — ValEvaluationProver (src/zkvm/ram/val_evaluation.zig:554-628: inc * wa * lt), ValFinalProver
 * (ram/val_final.zig:149-200: inc * wa), OutputSumcheckProver (ram/output_check.zig:375-470: eq * io * (vf - vio)),
 * InstructionLookupsClaimReduction (claim_reductions/instruction_lookups.zig:146-240: eq * (out + gamma left + gamma^2 right)) and the
 * Gruen-form ProductVirtualRemainderProver (spartan/product_remainder.zig:269-420: left * right under split-eq weights). A session keeps
 * k <= 12 tables of `len` entries (a power of two) resident in HBM; the transcript, the claim update and the Gruen scalar algebra stay
 * on the host. */
typedef struct zg_psc_s *zg_psc_t;
ZG_API int zg_psc_open(const uint64_t *const *tables /* k host pointers, len*4 words each */, size_t k, size_t len, zg_psc_t *s);
ZG_API int zg_psc_open_dev(const uint64_t *const *d_tables /* host array of k device pointers */, size_t k, size_t len, void *stream,
                    zg_psc_t *s); /* copies. stream = NULL: the session runs on its own stream; the copies follow the work already on the
                                   * library stream (the *_dev builders' default) and are complete on return. Otherwise the session
                                   * lives on `stream` and the copies are only enqueued there. */
ZG_API size_t zg_psc_len(zg_psc_t s);
ZG_API size_t zg_psc_tables(zg_psc_t s);
/* out[t] (t = 0..3, 4 words each) = sum over the pairs g of  prod_{j<p} T[prod_idx[j]](t) * L(t), where T(t) = T[2g] + t (T[2g+1] - T[2g])
 * and L(t) = sum_{m<q} lin_coeff[m] * T[lin_idx[m]](t) (q = 0: L = 1). p, q <= 4, p + q >= 1. These are the reference's
 * [p(0), p(1), p(2), p(3)] (val_evaluation.zig:554-603); provers that send fewer values drop the rest. */
ZG_API int zg_psc_round_evals(zg_psc_t s, const int *prod_idx, size_t p, const int *lin_idx, const uint64_t *lin_coeff /* q*4 */, size_t q,
                       uint64_t out[16]);
/* A SUM of up to four such product terms in one pass — the round polynomials of stage3_prover.zig: ShiftSumcheck phase 1 (four P*Q
 * pairs, :1351-1392) and phase 2 (:1399-1455), InstructionInput ((eq_out + g^2 eq_prod) * (is_rs2*rs2 + is_imm*imm + g (is_rs1*rs1 +
 * is_pc*pc)), :2029-2100: four terms of two plain factors and a two-table combination). out as zg_psc_round_evals; provers that
 * derive p(1) from the claim drop it. */
#define ZG_PSC_PAIR_SUM 256 /* n_prod = 4 | ZG_PSC_PAIR_SUM: the term is (T[prod[0]]*T[prod[1]] + T[prod[2]]*T[prod[3]]) * L (L = 1 when
                             * n_lin = 0) — two terms with the same weight as one (InstructionInput: is_rs2*rs2 + is_imm*imm under one
                             * weight; ShiftSumcheck phase 1: P_0*Q_0 + P_1*Q_1): three field products per evaluation point, not four */
typedef struct {
    int n_prod;
    int prod[4];
    int n_lin;
    int lin[4];
    uint64_t lin_coeff[16]; /* n_lin x 4 words, Montgomery */
} zg_psc_term;
ZG_API int zg_psc_round_expr(zg_psc_t s, const zg_psc_term *terms, size_t n_terms /* 1..4 */, uint64_t out[16]);
/* The evaluation points the following zg_psc_round_evals / zg_psc_round_expr calls (and the evaluations fused into zg_psc_bind)
 * compute: bit t of `points` = p(t) is wanted; the other slots of out[] come back as zero and their field products are not spent.
 * Several reference provers read p(0) and p(2) only and derive p(1) = claim - p(0), p(3) = p(0) - 3 p(1) + 3 p(2)
 * (claim_reductions/instruction_lookups.zig:146-200; stage3_prover.zig:1399-1455, 2334-2389) or all but p(1) (:2029-2100).
 * Default 0xF (all four); a session handed out again by zg_psc_open starts at 0xF. */
ZG_API int zg_psc_set_points(zg_psc_t s, unsigned points /* 1..15 */);
/* Gruen's pair (product_remainder.zig:281-330): t0 = sum_g w(g) prod_j T_j[2g], t_inf = sum_g w(g) prod_j (T_j[2g+1] - T_j[2g]),
 * w(g) = E_out[g >> log2|E_in|] * E_in[g & (|E_in| - 1)], pairs with g >> log2|E_in| >= |E_out| skipped. d_e_out / d_e_in: DEVICE
 * pointers (e.g. into the buffer zg_fr_eq_prefix_tables_dev filled: table k starts at element 2^k - 1). */
ZG_API int zg_psc_round_gruen(zg_psc_t s, const int *prod_idx, size_t p, const uint64_t *d_e_out, size_t n_out, const uint64_t *d_e_in,
                       size_t n_in, uint64_t t0[4], uint64_t t_inf[4]);
/* every table folded: T'[i] = (1 - r) T[2i] + r T[2i+1]; len -> len / 2 (val_evaluation.zig:609-628) */
ZG_API int zg_psc_bind(zg_psc_t s, const uint64_t r[4]);
ZG_API int zg_psc_read(zg_psc_t s, size_t table, uint64_t *out /* len*4 */);
/* the table where it lies in HBM (zg_psc_len(s) * 4 words), after the session's pending folds have completed: valid until the next
 * bind / close of this session. For handing folded tables to another session or kernel without a host round trip (Stage 3's phase
 * transitions, src/zkvm/spartan/stage3_prover.zig:1506-1700, 2427-2466, re-open their provers over the folded witness columns). */
ZG_API int zg_psc_table_dev(zg_psc_t s, size_t table, const uint64_t **d_ptr);
/* out[i] = T[table][idx[i]], i < n: the inc values of the row pairs a sparse prover's entries touch (read_write_checking.zig:431-446) */
ZG_API int zg_psc_gather(zg_psc_t s, size_t table, const uint64_t *idx, size_t n, uint64_t *out /* n*4 */);
ZG_API int zg_psc_final(zg_psc_t s, uint64_t *out /* k*4: each table's single remaining entry */);
ZG_API int zg_psc_close(zg_psc_t s);

/* ================================================================== OPTIONAL section: protocol-specific sessions */
#ifndef ZG_NO_PROTOCOL_SESSIONS
/* ------------------------------------------------------------------ registers read/write checking (Stage 4) */
/* Stage4GruenProver (src/zkvm/spartan/stage4_gruen_prover.zig:65-1240) and the original Stage4Prover (stage4_prover.zig:74-865: the same
 * tables, every cycle variable first under a dense eq table set at the start, all four evaluations computed directly), the
 * RegistersReadWriteChecking sumcheck: five DENSE tables of
 * K = 128 registers x T = 2^log_t cycles — val, rd_wa, ra = gamma rs1_ra + gamma^2 rs2_ra, rs1_ra, rs2_ra, indexed [k * T + j] — plus
 * inc[T], LOG_K + log_t rounds in three phases (cycle variables in Gruen form, the seven register variables, the remaining cycle
 * variables under the merged dense eq table). The session builds the tables on the device from the per-cycle trace columns and keeps
 * them in HBM — the 32 rows that can be non-zero (register indices are 5-bit fields; rows 32..127 are zero in the reference's tables
 * and are neither stored nor visited here); every round is one pass (sums) + one pass (folds). The eq structure, Gruen's cubic, the claim and the transcript stay on
 * the host. Values are the reference's, exactly.
 *   rs1 / rs2 / rd [T]: the register a cycle reads / writes, 0xFF = none — decided as initWithPhaseConfig does (:199-246: by opcode; rd
 *                        only when it is used and non-zero); padding cycles are 0xFF;
 *   reg_vals [32 * T] : value of register k before cycle j at [k * T + j] (:186-192, 249-258);  inc [T * 4]: F.fromU64(post) - F.fromU64(pre)
 *                        of the written register, zero elsewhere (:240-243);  gamma: the batching challenge. */
typedef struct zg_rrw_s *zg_rrw_t;
ZG_API int zg_rrw_open(size_t log_t, const uint8_t *rs1, const uint8_t *rs2, const uint8_t *rd, const uint64_t *reg_vals, const uint64_t *inc,
                const uint64_t gamma[4], zg_rrw_t *s);
/* the same session from the write column alone: rd_value [T] = what cycle j writes to register rd[j] (ignored where rd[j] = 0xFF). The
 * register file before every cycle (the last write to each register at an earlier cycle, zero before the first) and inc are rebuilt on
 * the device — 11 bytes per cycle cross the boundary instead of 291, and the host keeps no 32 x T table (stage4_gruen_prover.zig:183-258). */
ZG_API int zg_rrw_open_trace(size_t log_t, const uint8_t *rs1, const uint8_t *rs2, const uint8_t *rd, const uint64_t *rd_value,
                      const uint64_t gamma[4], zg_rrw_t *s);
ZG_API size_t zg_rrw_cycles(zg_rrw_t s);    /* current_T */
ZG_API size_t zg_rrw_registers(zg_rrw_t s); /* current_K */
/* phase1ComputeMessage's pair (:561-741): q0 = sum_i E_out[i >> log2|E_in|] E_in[i & (|E_in| - 1)] sum_k C_0(k, i), qX2 likewise with the
 * slopes; C = ra val + wa (val + inc) over the cycle pair (2i, 2i + 1). d_e_out / d_e_in: DEVICE tables (zg_fr_eq_prefix_tables_dev). */
ZG_API int zg_rrw_round_cycle_gruen(zg_rrw_t s, const uint64_t *d_e_out, size_t n_out, const uint64_t *d_e_in, size_t n_in, uint64_t q0[4], uint64_t qx2[4]);
/* the merged eq table of gruen_eq.merge (gruen_eq.zig:119-146) after the last phase-1 bind: n = zg_rrw_cycles(s) entries (host) */
ZG_API int zg_rrw_set_eq(zg_rrw_t s, const uint64_t *eq, size_t n);
/* phase2ComputeMessage's (eval_0, eval_2) (:764-852; also the register rounds once a single cycle is left, :955-1013). e1 != NULL: the value
 * at t = 1 as well, computed from the odd rows — Stage4Prover.computeRoundEvalsInternal's register rounds evaluate it directly
 * (src/zkvm/spartan/stage4_prover.zig:666-706) instead of taking it from the claim. */
ZG_API int zg_rrw_round_address(zg_rrw_t s, uint64_t e0[4], uint64_t *e1 /* 4 words, or NULL */, uint64_t e2[4]);
/* phase3ComputeMessage's (eval_0, eval_2, eval_3) (:854-953); e1 != NULL: p(1) too, as Stage4Prover's cycle rounds compute all four
 * (stage4_prover.zig:617-664) */
ZG_API int zg_rrw_round_cycle(zg_rrw_t s, uint64_t e0[4], uint64_t *e1 /* 4 words, or NULL */, uint64_t e2[4], uint64_t e3[4]);
/* bindPolynomials (:1047-1163): fold the cycle variable (five tables, inc, and the merged eq table once it is set) / the register variable */
ZG_API int zg_rrw_bind_cycle(zg_rrw_t s, const uint64_t r[4]);
ZG_API int zg_rrw_bind_address(zg_rrw_t s, const uint64_t r[4]);
/* entry [0][0] of val, rd_wa, ra, rs1_ra, rs2_ra, then inc[0] and merged_eq[0] (7 x 4 words): getFinalClaims (:1219-1236) */
ZG_API int zg_rrw_final(zg_rrw_t s, uint64_t *out /* 28 */);
ZG_API int zg_rrw_close(zg_rrw_t s);

/* ------------------------------------------------------------------ RAM read/write checking (Stage 2, the sparse instance) */
/* RamReadWriteCheckingProver (src/zkvm/ram/read_write_checking.zig:160-1323): a list of access entries {cycle, address, ra_coeff, val_coeff,
 * prev_val, next_val} (:91-157) beside three dense tables — eq_evals = eq(r_cycle, .) and inc over 2^log_t cycles, val_init over 2^log_k
 * words — and log_t + log_k rounds in three phases: phase1_num_rounds cycle variables, the address variables, the remaining cycle
 * variables. The session owns everything: the reference's walks over the integer fields of the list (who pairs with whom, which
 * checkpoint a lone entry meets) run once per round inside the library — the cycle phases' neighbour rule on the device, the address
 * phase's sequential column walk on the host; ra_coeff, val_coeff and the dense tables live in HBM, where one kernel turns a round's
 * walk into its two sums and one into the bound list. The caller keeps what the
 * reference's struct keeps besides: the GruenSplitEqPolynomial (its prefix tables as device buffers), the cubic, the claim.
 *   entries: sorted by (cycle, address) as init leaves them (:333-340); val_coeff as u64 (F.fromU64 of prev_val for a write, of the value
 *   for a read, :300-330), ra_coeff = 1; inc / val_init: field elements (:253-330); r_cycle: the eq point, r_cycle[0] <-> MSB (:345-348). */
typedef struct zg_rwc_s *zg_rwc_t;
ZG_API int zg_rwc_open(size_t log_k, size_t log_t, size_t n, const uint32_t *cycle, const uint32_t *address, const uint64_t *val_coeff,
                const uint64_t *prev_val, const uint64_t *next_val, const uint64_t *inc /* 2^log_t * 4 */, const uint64_t *val_init /* 2^log_k * 4 */,
                const uint64_t *r_cycle /* log_t * 4 */, zg_rwc_t *s);
/* the same session without the dense inc table crossing the boundary: is_write [n] marks the entries that are writes, and the device
 * forms inc[cycle] = F.fromU64(next_val) - F.fromU64(prev_val) for them (zero elsewhere) — what init's loop assigns (:283-291). A list
 * with two writes in one cycle is refused (ZG_ERR_INVALID): the reference keeps the later one in ACCESS order; use zg_rwc_open then. */
ZG_API int zg_rwc_open_writes(size_t log_k, size_t log_t, size_t n, const uint32_t *cycle, const uint32_t *address, const uint64_t *val_coeff,
                       const uint64_t *prev_val, const uint64_t *next_val, const uint8_t *is_write, const uint64_t *val_init /* 2^log_k * 4 */,
                       const uint64_t *r_cycle /* log_t * 4 */, zg_rwc_t *s);
ZG_API size_t zg_rwc_entries(zg_rwc_t s); /* current length of the list */
ZG_API size_t zg_rwc_cycles(zg_rwc_t s);  /* current length of eq_evals / inc */
/* computePhase1Polynomial's (q_constant, q_quadratic) (:410-536) under the split-eq weights E_out x E_in (DEVICE tables, as
 * zg_psc_round_gruen takes them); cycle phases 1 and 3 */
ZG_API int zg_rwc_round_cycle(zg_rwc_t s, const uint64_t *d_e_out, size_t n_out, const uint64_t *d_e_in, size_t n_in, const uint64_t gamma[4],
                       uint64_t q_constant[4], uint64_t q_quadratic[4]);
/* bindChallenge in a cycle phase (:919-938, 1139-1185): eq_evals and inc LowToHigh, the entry list pairwise. Needs zg_rwc_cycles(s) >= 2
 * (the reference skips the whole bind otherwise, :915). */
ZG_API int zg_rwc_bind_cycle(zg_rwc_t s, const uint64_t r[4]);
/* computePhase2Polynomial's (s(0), s(2)) (:538-769) in address round addr_round = round - phase1_num_rounds; challenges: the address
 * challenges bound so far (addr_round elements, host). The first call sorts the list address-major (:553-558). */
ZG_API int zg_rwc_round_address(zg_rwc_t s, size_t addr_round, const uint64_t *challenges, const uint64_t gamma[4], uint64_t s0[4], uint64_t s2[4]);
/* bindChallenge in the address phase (:953-970, 973-1137): val_init LowToHigh, then the entry list by column pairs */
ZG_API int zg_rwc_bind_address(zg_rwc_t s, size_t addr_round, const uint64_t r[4]);
/* getOpeningClaims (:1210-1322): ra_claim, val_claim, inc_claim (3 x 4 words) at r_address (log_k, [0] <-> MSB) and r_cycle (log_t) */
ZG_API int zg_rwc_opening(zg_rwc_t s, const uint64_t *r_address, const uint64_t *r_cycle, uint64_t out[12]);
/* eq_evals[0] and inc[0] as they stand (the two scalars the address phase works with, :543-552) */
ZG_API int zg_rwc_cycle_scalars(zg_rwc_t s, uint64_t eq0[4], uint64_t inc0[4]);
/* the current list (any pointer may be NULL); the coefficient columns come from the device */
ZG_API int zg_rwc_read_entries(zg_rwc_t s, uint32_t *cycle, uint32_t *address, uint64_t *ra_coeff, uint64_t *val_coeff, uint64_t *prev_val, uint64_t *next_val);
ZG_API int zg_rwc_close(zg_rwc_t s);

#endif /* ZG_NO_PROTOCOL_SESSIONS */
/* ================================================================== end of the OPTIONAL section */

/* ------------------------------------------------------------------ several GPUs in one process */
/* The bases (SRS) sharded over the bound devices in ParallelMSM's contiguous chunks of ceil(n / S) points
 * (src/msm/mod.zig:609,619-639), one resident table per device. */
typedef struct zg_sbases_s *zg_sbases_t;
/* the partition itself — chunk `shard` of `shards` over n points: start = min(shard * ceil(n / shards), n), end = min(start +
 * ceil(n / shards), n) (src/msm/mod.zig:609,619-621). Pure host arithmetic, needs no device. */
ZG_API int zg_shard_bounds(size_t n, int shards, int shard, size_t *start, size_t *len);
ZG_API int zg_g1_bases_upload_sharded(const uint64_t *xy, const uint8_t *inf, size_t n, const zg_msm_config *cfg, zg_sbases_t *out);
ZG_API int zg_g1_sbases_free(zg_sbases_t sb);
ZG_API size_t zg_g1_sbases_len(zg_sbases_t sb);
ZG_API int zg_g1_sbases_shards(zg_sbases_t sb);   /* number of shards S */
ZG_API int zg_g1_sbases_exchange(zg_sbases_t sb); /* how partials meet: 0 = single shard, 1 = RCCL all-gather, 2 = peer copies */
ZG_API int zg_g1_sbases_shard(zg_sbases_t sb, int shard, int *device, size_t *start, size_t *len);
/* ParallelMSM.compute(bases[0..n), scalars) (src/msm/mod.zig:588-653) over the devices: every device runs the Pippenger pipeline
 * on its chunk (one host worker thread per device issues its launches), the S Jacobian partials (96 B each, un-normalised) are
 * exchanged with ONE ncclAllGather over xGMI (RCCL has no user-defined reduction for group elements) and device 0 performs the
 * serial combine + the single toAffine (:647-652). Result bytes equal zg_msm_g1's. Scalars: n x 4 limbs on the host. */
ZG_API int zg_msm_g1_sharded(zg_sbases_t sb, size_t n, const uint64_t *scalars_mont, uint64_t out_xy[8], uint8_t *out_inf);
/* same with the scalars resident: d_scalars_per_shard[i] points into device memory of shard i's device and holds the scalars of
 * that shard's chunk (zg_g1_sbases_shard tells which). The buffers are read on the handle's own streams, which are not ordered
 * with the streams of the caller: their contents must be complete (synchronised) when the call is made. */
ZG_API int zg_msm_g1_sharded_dev(zg_sbases_t sb, size_t n, const uint64_t *const *d_scalars_per_shard, uint64_t out_xy[8],
                          uint8_t *out_inf);
/* ParallelBatchMSM.compute / HyperKZG.batchCommit (src/msm/mod.zig:683-748, src/poly/commitment/mod.zig:558-570) sharded: k scalar
 * vectors over bases[0..n) -> k partials per device, ONE all-gather of k x 96 B per device, k combines. */
ZG_API int zg_msm_g1_batch_sharded(zg_sbases_t sb, size_t n, const uint64_t *const *scalar_batches, size_t k, uint64_t *out_xy /* k*8 */,
                            uint8_t *out_inf /* k */);
/* Pipelined forms: the call returns a ticket as soon as every device's launch set, the exchange and the combine are ENQUEUED;
 * zg_sharded_wait(ticket) blocks until that call's result records have reached the host and hands them out (out_xy: k*8 words,
 * out_inf: k bytes or NULL; k = 1 for zg_msm_g1_sharded_dev_async). A handle keeps zg_g1_sbases_inflight() calls in flight (3 by
 * default; ZG_SHARDED_INFLIGHT = 1..8 at upload), each on its own stream per device, so the latency-bound tail and the exchange of
 * one MSM run under the accumulation of the next — HyperKZG.batchCommit over long vectors (src/poly/commitment/mod.zig:558-570)
 * and `zolt prove`'s three commitments (src/zkvm/mod.zig:1538,1572,1607) overlap this way. One more call than that without a wait
 * returns ZG_ERR_INVALID. Tickets may be waited for in any order, each exactly once. The synchronous entry points above are
 * these + zg_sharded_wait.
 * Scalars: the host vectors of zg_msm_g1_batch_sharded_async must stay valid until the ticket is waited for. The device buffers
 * of zg_msm_g1_sharded_dev[_async] are read on the handle's own streams: they must be COMPLETE when the call is made, unless
 * ready_streams (S stream handles, shard order; NULL or NULL entries = complete) names for every shard the stream whose enqueued
 * work fills that shard's buffer — the shard's launch set is then ordered behind it with an event. */
ZG_API int zg_msm_g1_sharded_dev_async(zg_sbases_t sb, size_t n, const uint64_t *const *d_scalars_per_shard, void *const *ready_streams,
                                uint64_t *ticket);
ZG_API int zg_msm_g1_batch_sharded_async(zg_sbases_t sb, size_t n, const uint64_t *const *scalar_batches, size_t k /* >= 1 */,
                                  uint64_t *ticket);
ZG_API int zg_sharded_wait(zg_sbases_t sb, uint64_t ticket, uint64_t *out_xy, uint8_t *out_inf);
ZG_API int zg_g1_sbases_inflight(zg_sbases_t sb); /* calls the handle keeps in flight */

/* Sumcheck(F).Prover over a table sharded across the bound devices (S = the largest power of two <= devices and <= len):
 * LOW_PAIR tables by contiguous chunks, HIGH_HALF tables by residue class i mod S, so that every fold of the first
 * log2(len / S) rounds is local to a device; a round's sums are the modular sum of the per-device pairs (64 B per device, read
 * from each session's pinned mailbox); the last log2(S) rounds run on the S gathered residuals on device 0. Same messages as
 * the single-device session, bit for bit. */
typedef struct zg_ssc_s *zg_ssc_t;
ZG_API int zg_sumcheck_open_sharded(const uint64_t *evals, size_t len, int layout, zg_ssc_t *s);
ZG_API int zg_sumcheck_shards(zg_ssc_t s);
ZG_API size_t zg_sumcheck_len_sharded(zg_ssc_t s);
ZG_API int zg_sumcheck_round_sums_sharded(zg_ssc_t s, uint64_t g0[4], uint64_t g1[4]);
ZG_API int zg_sumcheck_bind_sharded(zg_ssc_t s, const uint64_t r[4]);
ZG_API int zg_sumcheck_final_sharded(zg_ssc_t s, uint64_t out[4]);
ZG_API int zg_sumcheck_close_sharded(zg_ssc_t s);

#ifdef __cplusplus
}
#endif
#endif /* ZOLT_GPU_H */
