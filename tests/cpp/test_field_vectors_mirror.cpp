// test_field_vectors_mirror.cpp — zolt::BatchOps and zolt::BatchOps::Dev (zolt_amd/host/field_vectors.hpp) on the reference's known answers
// (src/field/mod.zig:1445-1494) and on a vector with zeros. tests/test_gpu_field_vectors.py builds it with g++ against libzolt_gpu.so,
// runs it and compares the printed words with what the Python mirror computes on the same vector.
//
// stdout: "known_answers ok", then "<host|dev>_<inverse|inner|horner|scaled|sum> <hex words>" lines.
#include <cstdio>

#include "zolt_host.hpp"

using zolt::BatchOps;
using zolt::Fr;

static void print(const char *name, const Fr *v, size_t n) {
    std::printf("%s ", name);
    for (size_t i = 0; i < n; i++)
        for (int l = 0; l < 4; l++) std::printf("%016llx", (unsigned long long)v[i].limbs[l]);
    std::printf("\n");
}

static bool knownAnswers() {
    Fr a[4], b[4], r[4];
    for (int i = 0; i < 4; i++) {
        a[i] = Fr::fromU64(i + 1);
        b[i] = Fr::fromU64(i + 5);
    }
    bool ok = true;
    BatchOps::batchAdd(r, a, b, 4);
    for (int i = 0; i < 4; i++) ok = ok && r[i].eql(Fr::fromU64(2 * i + 6));
    ok = ok && BatchOps::innerProduct(a, b, 4).eql(Fr::fromU64(70));
    ok = ok && BatchOps::multiScalarMulLinear(a, b, 4).eql(Fr::fromU64(70));
    ok = ok && BatchOps::hornerEval(a, 4, Fr::fromU64(2)).eql(Fr::fromU64(49));
    Fr c[8], d[8];
    for (int i = 0; i < 8; i++) {
        c[i] = Fr::fromU64(i + 1);
        d[i] = Fr::fromU64(i + 10);
    }
    ok = ok && BatchOps::innerProduct(c, d, 8).eql(Fr::fromU64(528));
    Fr nz[3] = {Fr::fromU64(2), Fr::fromU64(3), Fr::fromU64(5)}, inv[3];
    BatchOps::batchInverse(inv, nz, 3);
    for (int i = 0; i < 3; i++) ok = ok && nz[i].mul(inv[i]).eql(Fr::one());
    BatchOps::batchSquare(r, a, 4);
    for (int i = 0; i < 4; i++) ok = ok && r[i].eql(Fr::fromU64((i + 1) * (i + 1)));
    BatchOps::batchSub(r, b, a, 4);
    BatchOps::batchMul(inv, nz, nz, 3);
    ok = ok && r[2].eql(Fr::fromU64(4)) && inv[2].eql(Fr::fromU64(25));
    ok = ok && BatchOps::hornerEval(a, 0, Fr::fromU64(2)).isZero() && BatchOps::innerProduct(a, b, 0).isZero();
    return ok;
}

int main() {
    try {
        zolt::check(zg_init(0), "zg_init");
        std::printf("known_answers %s\n", knownAnswers() ? "ok" : "WRONG");
        const size_t n = 600;
        std::vector<Fr> v(n), w(n), out(n);
        for (size_t i = 0; i < n; i++) {
            v[i] = i % 7 == 3 ? Fr::zero() : Fr::fromU64(i * i + 3);
            w[i] = Fr::fromU64(2 * i + 1);
        }
        const Fr five = Fr::fromU64(5), eleven = Fr::fromU64(11);
        BatchOps::batchInverse(out.data(), v.data(), n);
        print("host_inverse", out.data(), n);
        Fr s = BatchOps::innerProduct(v.data(), w.data(), n);
        print("host_inner", &s, 1);
        s = BatchOps::hornerEval(v.data(), n, five);
        print("host_horner", &s, 1);
        BatchOps::batchMulScalar(out.data(), v.data(), n, eleven);
        print("host_scaled", out.data(), n);
        BatchOps::batchAdd(out.data(), v.data(), w.data(), n);
        print("host_sum", out.data(), n);

        zolt::DeviceMem dv(n * 32), dw(n * 32), dout(n * 32);
        zolt::check(zg_memcpy_h2d(dv.p, v.data(), n * 32), "zg_memcpy_h2d");
        zolt::check(zg_memcpy_h2d(dw.p, w.data(), n * 32), "zg_memcpy_h2d");
        auto fetch = [&](const char *name) {
            zolt::check(zg_memcpy_d2h(out.data(), dout.p, n * 32), "zg_memcpy_d2h");  // on the library's stream: behind the call
            print(name, out.data(), n);
        };
        BatchOps::Dev::batchInverse(dout.u64(), dv.u64(), n);
        fetch("dev_inverse");
        s = BatchOps::Dev::innerProduct(dv.u64(), dw.u64(), n);
        print("dev_inner", &s, 1);
        s = BatchOps::Dev::hornerEval(dv.u64(), n, five);
        print("dev_horner", &s, 1);
        BatchOps::Dev::batchMulScalar(dout.u64(), dv.u64(), n, eleven);
        fetch("dev_scaled");
        BatchOps::Dev::batchAdd(dout.u64(), dv.u64(), dw.u64(), n);
        fetch("dev_sum");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "test_field_vectors_mirror: %s\n", e.what());
        return 1;
    }
    return 0;
}
