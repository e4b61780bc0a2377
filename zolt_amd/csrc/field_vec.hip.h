// field_vec.hip.h — what one lane does in the kernels of field_vec.hip (zolt_gpu.h, "field vectors (device)"): Montgomery's trick over the
// E elements a lane owns, Horner's rule over E consecutive coefficients, the weight of a chunk from the power ladder. Plain functions
// of field.hip.h's arithmetic, without a lane movement, so that tests/cpp/field_vec_host.cpp compiles the same text for the CPU (the
// function qualifiers are the only things replaced). The batch-inverse kernel is here as well — a template over E, so that a sweep can
// instantiate other group sizes than the library's — because it needs nothing but these functions.
#pragma once
#include "../../include/zolt_gpu_internal.h"
#include "field.hip.h"

#ifndef ZG_DEV_CALL
#define ZG_DEV_CALL static __device__ __noinline__
#endif

namespace zg {

constexpr int FV_E = ZG_FV_E;            // elements per lane
constexpr int FV_THREADS = 256;          // lanes per workgroup
constexpr int FV_TILE = ZG_FV_TILE;      // elements per workgroup and grid-stride trip
constexpr int FV_LADDER = 64;            // entries of Horner's power ladder: x^(E * 2^k), k < 64
static_assert(FV_TILE == FV_THREADS * FV_E, "ZG_FV_TILE is 256 * ZG_FV_E");

// The product as a REAL function: with fe_mul inlined 3 (E - 1) + E times the loops below are too large to unroll, and the arrays they
// index then live in scratch memory instead of registers
template <class P>
ZG_DEV_CALL Fe<P> fv_mul_call(Fe<P> a, Fe<P> b) {
    return fe_mul(a, b);
}

// take ? a : b, limb by limb (v_cndmask): the zero handling below must not split a wave around a product
template <class P>
ZG_DEV Fe<P> fe_select(bool take, const Fe<P> &a, const Fe<P> &b) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = take ? a.l[i] : b.l[i];
    return r;
}

// Montgomery's trick (BatchOps.batchInverse, src/field/mod.zig:1232-1273) over a[0, E): a[k] <- a[k]^-1, and 0 where a[k] = 0. A zero
// enters the running products as one — the first element included, which the reference forgets (:1241) — so the product is never zero
// and ONE inversion serves the group: 3 (E - 1) products and fe_inv_safegcd. The prefix products stay in registers.
template <class P, int E>
ZG_DEV void fv_inv_group(Fe<P> (&a)[E]) {
    Fe<P> pre[E];  // pre[k] = a'[0] * ... * a'[k], a' = a with its zeros replaced by one
    bool z[E];
    const Fe<P> one = Fe<P>::one(), zero = Fe<P>::zero();
#pragma unroll
    for (int k = 0; k < E; k++) {
        z[k] = a[k].is_zero();
        a[k] = fe_select(z[k], one, a[k]);
        pre[k] = k ? fv_mul_call(pre[k - 1], a[k]) : a[k];
    }
    Fe<P> run = fe_inv_safegcd(pre[E - 1]);  // 1 / (a'[0] ... a'[k]) on the way down
#pragma unroll
    for (int k = E - 1; k > 0; k--) {
        const Fe<P> inv = fv_mul_call(run, pre[k - 1]);
        run = fv_mul_call(run, a[k]);
        a[k] = fe_select(z[k], zero, inv);
    }
    a[0] = fe_select(z[0], zero, run);
}

// c[0] + x (c[1] + x (... + x c[E - 1])): hornerEval (:1217-1227) over one chunk
template <class P, int E>
ZG_DEV Fe<P> fv_horner_chunk(const Fe<P> (&c)[E], const Fe<P> &x) {
    Fe<P> r = c[E - 1];
#pragma unroll
    for (int k = E - 1; k > 0; k--) r = fe_add(fv_mul_call(r, x), c[k - 1]);
    return r;
}

// ladder[k] = x^(E * 2^k), k < nbits <= FV_LADDER: E - 1 products, then a squaring per entry (one lane, one dependent chain: only the
// entries the chunk indices can name are made)
template <class P, int E>
ZG_DEV void fv_ladder_fill(const Fe<P> &x, Fe<P> *ladder, int nbits) {
    Fe<P> p = x;
    for (int k = 1; k < E; k++) p = fe_mul(p, x);
    for (int k = 0; k < nbits; k++) {
        ladder[k] = p;
        if (k + 1 < nbits) p = fe_sqr(p);
    }
}
// x^(E * j) for chunk j < 2^nbits: the ladder entries the bits of j name, by select (a clear bit multiplies by one)
template <class P>
ZG_DEV Fe<P> fv_chunk_weight(const Fe<P> *ladder, uint64_t j, int nbits) {
    const Fe<P> one = Fe<P>::one();
    Fe<P> w = fe_select((j & 1u) != 0, ladder[0], one);
    for (int k = 1; k < nbits; k++) w = fe_mul(w, fe_select(((j >> k) & 1u) != 0, ladder[k], one));
    return w;
}
// bits needed to write every chunk index below `chunks` (at least 1)
static inline int fv_index_bits(uint64_t chunks) {
    int b = 1;
    while (b < 64 && (chunks - 1) >> b) b++;
    return b;
}

// The batch inverse over n elements. A workgroup takes tiles of 256 * E elements, grid-stride; inside a tile lane t owns elements
// t, t + 256, ..., so a wave's loads and stores are contiguous. Elements past n count as one and are never written; a lane without a
// single element skips the inversion (in the last tile whole waves do). A lane writes only what it read: out == a is safe.
template <class P, int E>
__global__ void __launch_bounds__(FV_THREADS) fv_batch_inv_kernel(const uint64_t *a, uint64_t *out, size_t n) {
    const size_t tile = (size_t)FV_THREADS * E;
    for (size_t base = (size_t)blockIdx.x * tile; base < n; base += (size_t)gridDim.x * tile) {
        const size_t first = base + threadIdx.x;
        if (first >= n) continue;
        Fe<P> v[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const size_t i = first + (size_t)k * FV_THREADS;
            v[k] = i < n ? fe_load<P>(a + 4 * i) : Fe<P>::one();
        }
        fv_inv_group<P, E>(v);
#pragma unroll
        for (int k = 0; k < E; k++) {
            const size_t i = first + (size_t)k * FV_THREADS;
            if (i < n) fe_store(out + 4 * i, v[k]);
        }
    }
}

}  // namespace zg
