/*
 * zolt_gpu_internal.h — test and bench scaffolding exported by libzolt_gpu.so that is NOT part of the drop-in boundary
 * (include/zolt_gpu.h). tests/ and bench.py bind these through zolt_amd/lib.py; a Zig host never needs them.
 */
#ifndef ZOLT_GPU_INTERNAL_H
#define ZOLT_GPU_INTERNAL_H

#include "zolt_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zg_field_op self-test hooks for the device arithmetic (results always come back canonical, Montgomery-2^256) */
#define ZG_OP_MUL29 9        /* Fp only: a*b through the MSM's 9x29-bit lazy representation (csrc/fp29.hip.h) */
#define ZG_OP_SQR29 10       /* Fp only: a^2 through the lazy representation (b ignored) */
#define ZG_OP_X3_29 11       /* Fp only: a chain through f29_x3, f29_sub2/4/7, f29_neg2, f29_times2/3 and the zero test on f29_from_fp outputs (runtime.hip) */
#define ZG_OP_INV_XGCD 12    /* same value as ZG_OP_INV via plain binary extended Euclid (cross-check) */
#define ZG_OP_INV_SAFEGCD 13 /* same value via batched Bernstein-Yang division steps (the device's toAffine path) */
/* Fp only, n even: elements (2i, 2i + 1) of a (and b) are the components (c0, c1) of one Fp2 element (csrc/fp2.hip.h) */
#define ZG_OP_FP2_MUL 14     /* src/field/pairing.zig:212-223 */
#define ZG_OP_FP2_SQR 15     /* :225-237 (b ignored) */
#define ZG_OP_FP2_INV 16     /* :255-263, one Fp inversion of the norm; inverse(0) -> 0 (b ignored) */
/* Fp only, n a multiple of 12: elements 12i .. 12i + 11 of a (and b) are one Fp12 element in the order of a GT element (zolt_gpu.h,
 * "Pairings (Dory)"): the tower of csrc/fp12.hip.h, src/field/pairing.zig:279-620 */
#define ZG_OP_FP12_MUL 17
#define ZG_OP_FP12_SQR 18    /* b ignored, as for every code below */
#define ZG_OP_FP12_INV 19    /* inverse(0) -> 0 */
#define ZG_OP_FP12_CONJ 20
#define ZG_OP_FP12_FROB1 21  /* a^p */
#define ZG_OP_FP12_FROB2 22  /* a^(p^2) */
#define ZG_OP_FP12_FROB3 23  /* a^(p^3) */
#define ZG_OP_FP12_EXP_X 24  /* expByX (:1786-1800): a^4965661367192848881 */

/* The state of a Dory opening session (zolt_gpu.h, "Dory opening (session)") for tests, through zg_field_op like the hooks above (codes
 * 25..31 stay invalid): field = ZG_FIELD_FR, a = ONE word holding the zg_dory_t handle, b = NULL, n = the entries `out` has room for. The
 * word is looked up among the sessions that are open before anything is read through it: a word that is no open session's handle (field
 * data under a stray op code, a closed session) gets ZG_ERR_INVALID. The call waits for the session's enqueued work (a fold included)
 * and writes the first min(zg_dory_open_len(s), n) entries; n = 0 only waits. */
#define ZG_OP_DORY_V1 32     /* v1: records of 9 words, xy[8] then a flag word (1 = identity) */
#define ZG_OP_DORY_V2 33     /* v2: records of 17 words, xy[16] then a flag word */
#define ZG_OP_DORY_S1 34     /* s1: 4 words per scalar */
#define ZG_OP_DORY_S2 35     /* s2 */
/* Where the calling thread's last zg_dory_commit_batch spent its time (zolt_gpu.h, "Dory commitments (key and batch)"), for
 * tools/bench_dory_commit.py: field = ZG_FIELD_FR, a = b = NULL, n = 5, out = five words holding doubles, milliseconds of a host clock:
 * upload, row sums (the table sums and the MSMs of Montgomery polynomials), Horner and affine, Miller loops, products and final
 * exponentiations. Measured only while ZG_DORY_COMMIT_TIMES=1 is in the environment — the stages are then separated by stream
 * synchronisations, which the untimed call does not pay — and zero otherwise. */
#define ZG_OP_DORY_COMMIT_SPLIT 36
/* The tower of the wave pairing engine (csrc/fp12_wave.hip.h; zolt_gpu.h, "Pairings (engine)"): a wavefront per element, the conventions
 * and the refusals of ZG_OP_FP12_* (Fp, n a multiple of 12; codes 37..39 stay invalid). Every code has the bits of its ZG_OP_FP12_*
 * counterpart. There is no cyclotomic square: ZG_OP_FP12W_EXP_X squares plainly and accepts any input, like expByX. */
#define ZG_OP_FP12W_MUL 40
#define ZG_OP_FP12W_SQR 41     /* b ignored, as for every code below but the last */
#define ZG_OP_FP12W_INV 42     /* inverse(0) -> 0 */
#define ZG_OP_FP12W_CONJ 43
#define ZG_OP_FP12W_FROB1 44
#define ZG_OP_FP12W_FROB2 45
#define ZG_OP_FP12W_FROB3 46
#define ZG_OP_FP12W_EXP_X 47
#define ZG_OP_FP12W_MUL_034 48 /* fp12MulBy034: a times the sparse c0 + c3 w + c4 v w; the first three Fp2 of each element of b are c0, c3, c4 */

/* The MSM's lazy 29-bit-limb field forms and group law (csrc/fp29.hip.h, g1_29.hip.h, g1_29x4.hip.h) on RAW limbs: the caller chooses
 * the representative and the limb encoding of every operand, which no whole MSM can. n records of 91 u32 in (ten operands of 9 limbs, one
 * flags word), n records of 146 u32 out (sixteen results, a status word, an aux word); host pointers. The ops and the record layout are
 * csrc/lazy_selftest.hip.h; tests/lazy_model.py is the model and the checker. ZG_ERR_INVALID for an unknown op, n == 0 or a null pointer. */
ZG_API int zg_selftest_lazy_g1(int op, const uint32_t *in, size_t n, uint32_t *out);

/* The same for the sumcheck kernels' lazy Fr arithmetic (the Fr side of csrc/fp29.hip.h: the lazy products and their short forms, the
 * prescaled and narrow factors, the 64- and 32-bit limb sums) and their lazy 288-bit sums (csrc/acc9.hip.h, csrc/sc_common.hip.h) on RAW
 * limbs. Ops 0..7: n records of 146 u32 in (sixteen slots of 9 words, a flags word, a length word) and 146 u32 out (sixteen slots, a
 * status word, an aux word), threads = 0. Op 8 (the block reduction block_sum_pair9): n workgroups of `threads` threads (a multiple of 64,
 * at most 1024); in = 18 u32 per thread (two raw nine-word sums), out = 16 u32 per workgroup (the two canonical totals). Host pointers.
 * The ops and the record layout are csrc/lazy_fr_selftest.hip.h; tests/lazy_fr_model.py is the model and the checker. ZG_ERR_INVALID for
 * an unknown op, n == 0 or n > 4096, a null pointer, or a thread count the op does not take. */
ZG_API int zg_selftest_lazy_fr(int op, const uint32_t *in, size_t n, uint32_t *out, int threads);

/* The canonical XYZZ group law (csrc/xyzz.hip.h: the law of everything but the G1 MSM's inner loop) on RAW coordinates, over Fp (group 0:
 * G1) and over Fp2 (group 1: G2): the caller chooses the representative (l^2 x, l^3 y, l^2, l^3) of every XYZZ operand, which no entry point
 * that takes affine points can. With W = 4 (group 0) or 8 (group 1) words per coordinate, canonical Montgomery form: n records of 8 W + 6
 * u64 in (two XYZZ operands, a scalar as a canonical integer, a flags word, a pad) and of 4 W + 2 u64 out (four coordinates or an affine
 * pair, a status word, a pad); host pointers. The ops (doubling, mixed and full addition, negation, conversion to affine, scalar
 * multiplication, one index of xyzz_axpy_at, fe_inv_safegcd) and the record layout are csrc/xyzz_selftest.hip.h; tests/xyzz_model.py is
 * the model and the checker. ZG_ERR_INVALID for an unknown group or op, n == 0 or n > 2^16, a null pointer. */
ZG_API int zg_selftest_xyzz(int group, int op, const uint64_t *in, size_t n, uint64_t *out);

/* The short-vector bucket MSM (csrc/small_msm.hip.h) on its own: ONE launch set of n_jobs MSMs (1..4) over G1 (group 0) or G2 (group 1),
 * job j over n[j] affine points xy[j] (8 or 16 u64 each), flags inf[j] (inf or inf[j] may be null) and Montgomery Fr scalars scalars[j];
 * the jobs may differ in length, and a length may be 0. One SmallMsmScratch sized for the longest job. out: n_jobs records of the
 * affine result (8 or 16 u64, an identity as the group's reference writes it) followed by a flag word (1 = identity). Host pointers.
 * ZG_ERR_INVALID for an unknown group, n_jobs outside 1..4, a length above 2^16, a null array, or a null xy[j] / scalars[j] with n[j] > 0. */
ZG_API int zg_selftest_small_msm(int group, int n_jobs, const size_t *n, const uint64_t *const *xy, const uint8_t *const *inf, const uint64_t *const *scalars,
                                 uint64_t *out);

/* The launch shape the library would choose for a kernel family at a size, under the environment switches this process was started with
 * (docs/design/08_switches.md): host code only, nothing is launched and no device is needed. It calls the functions the launches call
 * (eq_table_shape, eq_spartan_shape, fold_grid, sums_grid, sc_blocks, hk_fold_grid, fb_plan, rrw_chunks, psc_blocks / psc_spread), so a test that forces
 * a shape through a switch can assert that the switch took effect before it compares results. out: four words, unused ones zero.
 *   family                  a                      b                                      out
 *   ZG_SHAPE_EQ_TABLE       v (entries = 2^v)      1: r[v-11 .. v-8) are 128-bit          groups of 256 threads per workgroup (the kernel's
 *                                                  challenges [0, 0, lo, hi], 0: wide     template argument), rows per workgroup, workgroups,
 *                                                                                         1 if the expanding kernel is taken
 *   ZG_SHAPE_EQ_SPARTAN     v                      0                                      the same; out[3] = 0
 *   ZG_SHAPE_SC_FOLD        pairs (entries / 2)    1: zg_run_sumcheck's launches, 0: a    threads per workgroup, workgroups
 *   ZG_SHAPE_SC_SUMS                               session's
 *   ZG_SHAPE_SC_PAIRSUM     elements               0                                      256, workgroups (the raf / bit-split / range / dot kernels)
 *   ZG_SHAPE_FB             outputs n              0                                      window bits c, windows W, rows per window
 *   ZG_SHAPE_RRW            inner (pairs, cycles)  outer (registers a chunk may split)    register chunks of a Stage-4 round launch
 *   ZG_SHAPE_PSC            pairs                  0                                      workgroups of an expression round, 1 if one lane per
 *                                                                                         (pair, term, point) (psc_expr_spread_kernel)
 *   ZG_SHAPE_HK_FOLD        pairs of a level       0                                      256, workgroups (HyperKZG.open's quotient-fold)
 * ZG_ERR_INVALID for an unknown family, out == NULL, v > 34, a or b beyond 2^40, or b outside what the family takes. */
#define ZG_SHAPE_EQ_TABLE 0
#define ZG_SHAPE_EQ_SPARTAN 1
#define ZG_SHAPE_SC_FOLD 2
#define ZG_SHAPE_SC_SUMS 3
#define ZG_SHAPE_SC_PAIRSUM 4
#define ZG_SHAPE_FB 5
#define ZG_SHAPE_RRW 6
#define ZG_SHAPE_PSC 7
#define ZG_SHAPE_HK_FOLD 8
ZG_API int zg_selftest_launch_shape(int family, size_t a, size_t b, uint32_t out[4]);

/* The geometry of the batch inverse and of Horner's rule (csrc/field_vec.hip.h; zolt_gpu.h, "field vectors (device)"): a lane owns
 * ZG_FV_E elements, a workgroup of 256 lanes a tile of ZG_FV_TILE = 256 * ZG_FV_E. The tests take their sizes from here. ZG_FV_BLOCKS in the
 * environment caps the grid of these kernels and of the inner product (docs/design/08_switches.md). */
#define ZG_FV_E 8
#define ZG_FV_TILE 2048

/* ------------------------------------------------------------------ profiling */
/* Per-kernel timing with HIP events recorded on the stream each kernel is launched on
 * (bench.py's roofline figure). zg_profile_begin enables recording of up to max_records
 * kernel intervals; zg_profile_end synchronises, adds the elapsed times up per kernel id
 * (milliseconds, launch counts) and disables recording. Not thread-safe; bench use only. */
#define ZG_PROF_MSM_DIGITS 0
#define ZG_PROF_MSM_SORT 1       /* scan + scatter */
#define ZG_PROF_MSM_ACCUMULATE 2 /* bucket accumulation: the dominant MSM kernel */
#define ZG_PROF_MSM_REDUCE 3     /* bucket reduction levels + final */
#define ZG_PROF_EQ_TABLE 4
#define ZG_PROF_SC_FOLD 5        /* fold + fused next-round sums */
#define ZG_PROF_SC_SUMS 6
#define ZG_PROF_COMBINE 7        /* Spartan combine */
#define ZG_PROF_NKERNELS 8
ZG_API int zg_profile_begin(int max_records);
ZG_API int zg_profile_end(double ms_out[ZG_PROF_NKERNELS], uint64_t count_out[ZG_PROF_NKERNELS]);

/* Set-up phase split (tools/bench_sumcheck: "time set-up phases separately"). With ZG_SETUP_TIMES=1 in the environment the two entry points
 * that build large device state from host inputs — zg_fr_rows_from_columns and zg_rrw_open / zg_rrw_open_trace — synchronise between
 * their phases and record, for the calling thread's last call: out[0] = device allocation (pool), out[1] = host-to-device copies,
 * out[2] = kernels, out[3] = everything else inside the call, in milliseconds. Without the variable the calls run unsplit and this
 * returns zeros. */
ZG_API int zg_last_setup_times(double out[4]);

/* RCCL communicator sets (ncclCommInitAll) created so far by the one-process / several-GPU path: a set is shared by the sharded
 * handles made while the same number of devices is bound; tests check that re-binding creates a new set instead of failing. */
ZG_API int zg_sharded_comm_sets_created(void);

/* ZG_POOL_DEBUG (csrc/runtime.hip): the device pool's "a freed block is idle" contract, checked. With ZG_POOL_DEBUG=1 in the environment
 * freed (and fresh) blocks are filled with 0xDBDBDBDB and verified before they are handed out again; a block written after its free is
 * refused and counted (=2: the process aborts). zg_pool_debug_stats: out[0] = hits, out[1] = frees made while the device's library stream
 * was busy (information only), out[2] = blocks verified, out[3] = bytes poisoned; returns the mode (0 = off).
 * zg_pool_debug_selftest breaks the contract on purpose: 1 = the mode caught it, 0 = mode off (nothing checked), < 0 = error. */
ZG_API int zg_pool_debug_stats(uint64_t out[4]);
ZG_API int zg_pool_debug_selftest(void);

#ifdef __cplusplus
}
#endif
#endif /* ZOLT_GPU_INTERNAL_H */
