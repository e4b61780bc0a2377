// field_vectors.hpp — zolt.field.BatchOps (src/field/mod.zig:1164-1280) over the device: the section "field vectors (device)" of zolt_gpu.h.
// Part of zolt_host.hpp (the C++ host mirror over include/zolt_gpu.h); included by it, after the parts it depends on.
#pragma once
#ifndef ZOLT_HOST_UMBRELLA
#error "include zolt_host.hpp"
#endif
namespace zolt {

// The reference's names and argument order (`results` first; its allocator argument has no use here). Slices are pointer + length of
// host Fr; a table that already lives in HBM goes through BatchOps::Dev, the same operations over device pointers and a stream.
struct BatchOps {
    static const uint64_t *w(const Fr *p) { return reinterpret_cast<const uint64_t *>(p); }
    static uint64_t *w(Fr *p) { return reinterpret_cast<uint64_t *>(p); }

    static void batchAdd(Fr *results, const Fr *a, const Fr *b, size_t n) { check(zg_field_op(ZG_FIELD_FR, ZG_OP_ADD, w(a), w(b), w(results), n), "zg_field_op"); }
    static void batchSub(Fr *results, const Fr *a, const Fr *b, size_t n) { check(zg_field_op(ZG_FIELD_FR, ZG_OP_SUB, w(a), w(b), w(results), n), "zg_field_op"); }
    static void batchMul(Fr *results, const Fr *a, const Fr *b, size_t n) { check(zg_field_op(ZG_FIELD_FR, ZG_OP_MUL, w(a), w(b), w(results), n), "zg_field_op"); }
    static void batchMulScalar(Fr *results, const Fr *a, size_t n, const Fr &scalar) { check(zg_fr_scale(w(a), n, scalar.limbs, w(results)), "zg_fr_scale"); }
    static void batchSquare(Fr *results, const Fr *a, size_t n) { check(zg_field_op(ZG_FIELD_FR, ZG_OP_SQR, w(a), nullptr, w(results), n), "zg_field_op"); }
    static Fr innerProduct(const Fr *a, const Fr *b, size_t n) {
        Fr out;
        check(zg_field_inner_product(ZG_FIELD_FR, w(a), w(b), n, out.limbs), "zg_field_inner_product");
        return out;
    }
    static Fr hornerEval(const Fr *coeffs, size_t n, const Fr &x) {
        Fr out;
        check(zg_field_horner(ZG_FIELD_FR, w(coeffs), n, x.limbs, out.limbs), "zg_field_horner");
        return out;
    }
    // Element-wise: zero only where the input is zero. The reference zeroes EVERY output when a[0] is zero (:1241); on any other input
    // the two agree (zolt_gpu.h).
    static void batchInverse(Fr *results, const Fr *a, size_t n) { check(zg_field_batch_inverse(ZG_FIELD_FR, w(a), w(results), n), "zg_field_batch_inverse"); }
    static Fr multiScalarMulLinear(const Fr *scalars, const Fr *bases, size_t n) { return innerProduct(scalars, bases, n); }

    // the same over device pointers (n elements of four words): enqueued on `stream` (nullptr: the library's), the scalars waited for
    struct Dev {
        static void batchAdd(uint64_t *d_results, const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream = nullptr) {
            check(zg_field_op_dev(ZG_FIELD_FR, ZG_OP_ADD, d_a, d_b, d_results, n, stream), "zg_field_op_dev");
        }
        static void batchSub(uint64_t *d_results, const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream = nullptr) {
            check(zg_field_op_dev(ZG_FIELD_FR, ZG_OP_SUB, d_a, d_b, d_results, n, stream), "zg_field_op_dev");
        }
        static void batchMul(uint64_t *d_results, const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream = nullptr) {
            check(zg_field_op_dev(ZG_FIELD_FR, ZG_OP_MUL, d_a, d_b, d_results, n, stream), "zg_field_op_dev");
        }
        static void batchMulScalar(uint64_t *d_results, const uint64_t *d_a, size_t n, const Fr &scalar, void *stream = nullptr) {
            check(zg_field_scale_dev(ZG_FIELD_FR, d_a, n, scalar.limbs, d_results, stream), "zg_field_scale_dev");
        }
        static void batchSquare(uint64_t *d_results, const uint64_t *d_a, size_t n, void *stream = nullptr) {
            check(zg_field_op_dev(ZG_FIELD_FR, ZG_OP_SQR, d_a, nullptr, d_results, n, stream), "zg_field_op_dev");
        }
        static Fr innerProduct(const uint64_t *d_a, const uint64_t *d_b, size_t n, void *stream = nullptr) {
            Fr out;
            check(zg_field_inner_product_dev(ZG_FIELD_FR, d_a, d_b, n, stream, out.limbs), "zg_field_inner_product_dev");
            return out;
        }
        static Fr hornerEval(const uint64_t *d_coeffs, size_t n, const Fr &x, void *stream = nullptr) {
            Fr out;
            check(zg_field_horner_dev(ZG_FIELD_FR, d_coeffs, n, x.limbs, stream, out.limbs), "zg_field_horner_dev");
            return out;
        }
        static void batchInverse(uint64_t *d_results, const uint64_t *d_a, size_t n, void *stream = nullptr) {
            check(zg_field_batch_inverse_dev(ZG_FIELD_FR, d_a, d_results, n, stream), "zg_field_batch_inverse_dev");
        }
        static Fr multiScalarMulLinear(const uint64_t *d_scalars, const uint64_t *d_bases, size_t n, void *stream = nullptr) {
            return innerProduct(d_scalars, d_bases, n, stream);
        }
    };
};

}  // namespace zolt
