// points.hip — the per-element point batches of both groups: on-curve, affine add, scalar multiplication per pair, and the vector
// update out[i] = s * a[i] + b[i] of Dory's reduce-and-fold rounds (src/poly/commitment/dory.zig:1578-1584, 1615-1624).
//
// One lane per output, host pointers in and out, one inversion per output. The kernels are templated on the group; only the affine
// additions are two bodies, because they restate two reference functions that differ (below). G1 launches in workgroups of 256; G2 —
// short vectors, ~380 group operations with out-of-line Fp2 products per output — and both axpy kernels in workgroups of 64, so that
// every wave lands on its own SIMD; the axpy scalar is uniform over the launch, its double-and-add runs without divergence.
#include "common.hip.h"
#include "g1.hip.h"
#include "g2.hip.h"

namespace zg {

struct G1 {
    using F = Fp;
    static constexpr int BLOCK = 256, WORDS = 8;  // 64-bit words of an affine point
    ZG_DEV static bool on_curve(const Affine &p) { return g1_is_on_curve(p); }
};
struct G2 {
    using F = Fp2;
    static constexpr int BLOCK = 64, WORDS = 16;
    ZG_DEV static bool on_curve(const G2Affine &p) { return g2_is_on_curve(p); }
};

// AffinePoint.isOnCurve (msm/mod.zig:106-115), dory.zig computeG2YSquared; the identity counts as on the curve
template <class G>
__global__ void __launch_bounds__(G::BLOCK) on_curve_kernel(const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = ((inf && inf[i]) || G::on_curve(affine_load<typename G::F>(xy + G::WORDS * i))) ? 1 : 0;
}

// MSM.scalarMul(base, scalar).toAffine() (msm/mod.zig:503-540), G2Point.scalarMul (pairing.zig:880-919), one pair per thread
template <class G>
__global__ void __launch_bounds__(G::BLOCK) scalar_mul_kernel(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars, size_t n, uint64_t *out_xy,
                                                              uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fe_from_mont(fe_load<FrParams>(scalars + 4 * i));
    const XyzzT<typename G::F> acc = xyzz_scalar_mul(affine_load<typename G::F>(xy + G::WORDS * i), inf && inf[i], s);
    AffineT<typename G::F> r;
    const bool isinf = xyzz_to_affine(acc, r);
    affine_store(out_xy + G::WORDS * i, r);
    if (out_inf) out_inf[i] = isinf ? 1 : 0;
}

// out[i] = s * a[i] + b[i] with ONE scalar for the launch: v1[i] += beta * g1_vec[i], v2[i] += beta_inv * g2_vec[i] (dory.zig:1579-1583,
// a = the generators, b = v) and v[i] = alpha * v[i] + v[i + n2] (:1616-1624) — scalarMul(..) followed by the group's affine add, in one
// launch with one inversion per output
template <class G>
__global__ void __launch_bounds__(64) axpy_kernel(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, FeArg s_mont, size_t n,
                                                  uint64_t *out_xy, uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyzz_axpy_at<typename G::F>(a_xy, a_inf, b_xy, b_inf, fe_from_mont(fe_from_arg<FrParams>(s_mont)), i, out_xy, out_inf);
}

// The two affine additions stay apart: for equal x with y neither equal nor opposite (no such pair on the curve, but the ABI cannot
// rule it out) AffinePoint.add falls through to the chord and returns the identity, G2Point.add doubles its first operand.

// AffinePoint.add (msm/mod.zig:74-103) and, through add(p, p), AffinePoint.double (:118-138): the lambda formulas on canonical
// Montgomery values, one inversion per pair (safegcd, the value of the reference's Fermat inverse)
__global__ void __launch_bounds__(256) g1_affine_add_kernel(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy,
                                                            const uint8_t *b_inf, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine a = affine_load(a_xy + 8 * i), b = affine_load(b_xy + 8 * i), r;
    bool ai = a_inf && a_inf[i], bi = b_inf && b_inf[i], ri = false;
    if (ai) {  // :75-76
        r = b;
        ri = bi;
    } else if (bi) {
        r = a;
    } else {
        Fp num, den;
        bool dbl = false;
        if (a.x.eq(b.x)) {  // :79-88
            if (a.y.eq(fe_neg(b.y))) ri = true;
            else if (a.y.eq(b.y)) dbl = true;
        }
        if (!ri) {
            if (dbl) {  // :118-138: lambda = 3 x^2 / 2 y; y == 0 -> identity
                Fp xx = fe_sqr(a.x);
                num = fe_add(fe_add(xx, xx), xx);
                den = fe_add(a.y, a.y);
                if (a.y.is_zero()) ri = true;
            } else {  // :90-93: lambda = (y2 - y1) / (x2 - x1)
                num = fe_sub(b.y, a.y);
                den = fe_sub(b.x, a.x);
            }
        }
        if (!ri && den.is_zero()) ri = true;  // dx.inverse() orelse return identity() (:93,:129)
        if (!ri) {
            Fp lam = fe_mul(num, fe_inv_safegcd(den));
            Fp x2 = dbl ? a.x : b.x;
            r.x = fe_sub(fe_sub(fe_sqr(lam), a.x), x2);
            r.y = fe_sub(fe_mul(lam, fe_sub(a.x, r.x)), a.y);
        }
    }
    if (ri) r = Affine::identity();
    affine_store(out_xy + 8 * i, r);
    if (out_inf) out_inf[i] = ri ? 1 : 0;
}

// G2Point.add per pair (pairing.zig:839-875): the affine lambda formulas on canonical values, one Fp2 inversion per pair
__global__ void __launch_bounds__(64) g2_affine_add_kernel(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf,
                                                           size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G2Affine a = affine_load<Fp2>(a_xy + 16 * i), b = affine_load<Fp2>(b_xy + 16 * i), r;
    bool ai = a_inf && a_inf[i], bi = b_inf && b_inf[i], ri = false;
    if (ai) {  // :840-841
        r = b;
        ri = bi;
    } else if (bi) {
        r = a;
    } else {
        Fp2 num, den;
        const bool same_x = a.x.eq(b.x);
        if (same_x && a.y.eq(fe_neg(b.y))) {  // :843-846
            ri = true;
        } else if (same_x) {  // self.double() (:861-875): lambda = 3 x^2 / 2 y; y == 0 -> identity
            num = fp2_mul3(fe_sqr(a.x));
            den = fe_dbl(a.y);
            if (a.y.is_zero()) ri = true;
        } else {  // :851-853
            num = fe_sub(b.y, a.y);
            den = fe_sub(b.x, a.x);
        }
        if (!ri) {
            Fp2 lam = fe_mul(num, fe_inv_safegcd(den));
            Fp2 x2 = same_x ? a.x : b.x;
            r.x = fe_sub(fe_sub(fe_sqr(lam), a.x), x2);
            r.y = fe_sub(fe_mul(lam, fe_sub(a.x, r.x)), a.y);
        }
    }
    if (ri) r = G2Affine::identity();
    affine_store(out_xy + 16 * i, r);
    if (out_inf) out_inf[i] = ri ? 1 : 0;
}

// ---- the entry points: validate, stage inputs, launch, fetch outputs

template <class G>
static int on_curve_batch(const char *who, const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out) {
    ZG_INIT();
    if (n && (!xy || !out)) return invalid(who, "invalid argument");
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const uint64_t *d_xy = sg.in(xy, n * G::WORDS * 8);
    const uint8_t *d_inf = sg.in(inf, n);
    uint8_t *d_out = sg.out<uint8_t>(n);
    if (sg.ok()) {
        hipLaunchKernelGGL(on_curve_kernel<G>, dim3(div_up(n, G::BLOCK)), dim3(G::BLOCK), 0, sg.st, d_xy, d_inf, n, d_out);
        sg.launched();
    }
    sg.fetch(out, d_out, n);
    return sg.finish();
}

// the six arrays of out = f(a, b) per pair on the device: the affine additions and axpy
struct PairArrays {
    const uint64_t *a, *b;
    const uint8_t *a_inf, *b_inf;
    uint64_t *out;
    uint8_t *out_inf;
};
static PairArrays stage_pairs(Staging &sg, size_t point_bytes, const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n) {
    PairArrays d;
    d.a = sg.in(a_xy, n * point_bytes); d.b = sg.in(b_xy, n * point_bytes);
    d.a_inf = sg.in(a_inf, n); d.b_inf = sg.in(b_inf, n);
    d.out = sg.out<uint64_t>(n * point_bytes);
    d.out_inf = sg.out<uint8_t>(n);
    return d;
}
static int fetch_pairs(Staging &sg, const PairArrays &d, size_t point_bytes, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    sg.fetch(out_xy, d.out, n * point_bytes);
    sg.fetch(out_inf, d.out_inf, n);
    return sg.finish();
}

template <class G, class Kernel>
static int affine_add_batch(const char *who, Kernel kernel, const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n,
                            uint64_t *out_xy, uint8_t *out_inf) {
    ZG_INIT();
    if (n && (!a_xy || !b_xy || !out_xy)) return invalid(who, "invalid argument");
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const PairArrays d = stage_pairs(sg, G::WORDS * 8, a_xy, a_inf, b_xy, b_inf, n);
    if (sg.ok()) {
        hipLaunchKernelGGL(kernel, dim3(div_up(n, G::BLOCK)), dim3(G::BLOCK), 0, sg.st, d.a, d.a_inf, d.b, d.b_inf, n, d.out, d.out_inf);
        sg.launched();
    }
    return fetch_pairs(sg, d, G::WORDS * 8, n, out_xy, out_inf);
}

template <class G>
static int axpy_batch(const char *who, const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const uint64_t s[4], size_t n,
                      uint64_t *out_xy, uint8_t *out_inf) {
    ZG_INIT();
    if (!s || (n && (!a_xy || !b_xy || !out_xy))) return invalid(who, "invalid argument");
    if (n == 0) return ZG_OK;
    Staging sg(lib_stream());
    const PairArrays d = stage_pairs(sg, G::WORDS * 8, a_xy, a_inf, b_xy, b_inf, n);
    if (sg.ok()) {
        hipLaunchKernelGGL(axpy_kernel<G>, dim3(div_up(n, 64)), dim3(64), 0, sg.st, d.a, d.a_inf, d.b, d.b_inf, fe_arg(s), n, d.out, d.out_inf);
        sg.launched();
    }
    return fetch_pairs(sg, d, G::WORDS * 8, n, out_xy, out_inf);
}

template <class G>
static int scalar_mul_batch(const char *who, const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    ZG_INIT();
    if (n && (!xy || !scalars || !out_xy || !out_inf)) return invalid(who, "invalid argument");
    if (n == 0) return ZG_OK;
    const size_t pb = (size_t)G::WORDS * 8;
    Staging sg(lib_stream());
    const uint64_t *d_xy = sg.in(xy, n * pb), *d_sc = sg.in(scalars, n * 32);
    const uint8_t *d_inf = sg.in(inf, n);
    uint64_t *d_o = sg.out<uint64_t>(n * pb);
    uint8_t *d_oi = sg.out<uint8_t>(n);
    if (sg.ok()) {
        hipLaunchKernelGGL(scalar_mul_kernel<G>, dim3(div_up(n, G::BLOCK)), dim3(G::BLOCK), 0, sg.st, d_xy, d_inf, d_sc, n, d_o, d_oi);
        sg.launched();
    }
    sg.fetch(out_xy, d_o, n * pb);
    sg.fetch(out_inf, d_oi, n);
    return sg.finish();
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_g1_is_on_curve_batch(const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out) {
    return on_curve_batch<G1>("zg_g1_is_on_curve_batch", xy, inf, n, out);
}
int zg_g2_is_on_curve_batch(const uint64_t *xy, const uint8_t *inf, size_t n, uint8_t *out) {
    return on_curve_batch<G2>("zg_g2_is_on_curve_batch", xy, inf, n, out);
}

int zg_g1_affine_add_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n, uint64_t *out_xy,
                           uint8_t *out_inf) {
    return affine_add_batch<G1>("zg_g1_affine_add_batch", g1_affine_add_kernel, a_xy, a_inf, b_xy, b_inf, n, out_xy, out_inf);
}
int zg_g2_affine_add_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n, uint64_t *out_xy,
                           uint8_t *out_inf) {
    return affine_add_batch<G2>("zg_g2_affine_add_batch", g2_affine_add_kernel, a_xy, a_inf, b_xy, b_inf, n, out_xy, out_inf);
}

int zg_g1_scalar_mul_batch(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    return scalar_mul_batch<G1>("zg_g1_scalar_mul_batch", xy, inf, scalars, n, out_xy, out_inf);
}
int zg_g2_scalar_mul_batch(const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars, size_t n, uint64_t *out_xy, uint8_t *out_inf) {
    return scalar_mul_batch<G2>("zg_g2_scalar_mul_batch", xy, inf, scalars, n, out_xy, out_inf);
}

int zg_g1_axpy_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const uint64_t s[4], size_t n, uint64_t *out_xy,
                     uint8_t *out_inf) {
    return axpy_batch<G1>("zg_g1_axpy_batch", a_xy, a_inf, b_xy, b_inf, s, n, out_xy, out_inf);
}
int zg_g2_axpy_batch(const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, const uint64_t s[4], size_t n, uint64_t *out_xy,
                     uint8_t *out_inf) {
    return axpy_batch<G2>("zg_g2_axpy_batch", a_xy, a_inf, b_xy, b_inf, s, n, out_xy, out_inf);
}

}  // extern "C"
