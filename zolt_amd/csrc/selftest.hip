// selftest.hip — zg_selftest_lazy_g1 (include/zolt_gpu_internal.h): the MSM's lazy-limb arithmetic and group law on raw limbs, one
// record per lane (one per quad for the four-lane ops). The record format and the dispatch are lazy_selftest.hip.h, which the host harness
// of tests/test_lazy_group_law_host.py compiles too. This unit is built like msm.hip (no ZG_F29_SERIAL), so xyzz29_madd_nz runs the
// interleaved inline-assembly products here exactly as it does in the accumulate loop.
#include "common.hip.h"
#define ZG_LAZY_DEVICE_FORMS
#include "lazy_selftest.hip.h"

namespace zg {

__global__ void __launch_bounds__(64) lazy_g1_kernel(int op, const u32 *in, size_t n, u32 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lazy_record(op, in + ZG_LAZY_IN_WORDS * i, out + ZG_LAZY_OUT_WORDS * i);
}

// four adjacent lanes per record; a quad is either wholly inside n or wholly outside
__global__ void __launch_bounds__(64) lazy_g1_quad_kernel(int op, const u32 *in, size_t n, u32 *out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2;
    if (i >= n) return;
    u32 *o = out + ZG_LAZY_OUT_WORDS * i;
    const u32 bit = lazy_record4(op, in + ZG_LAZY_IN_WORDS * i, o, (u32)(t & 3));
    if (bit) atomicOr(&o[144], bit);  // the output buffer starts zeroed
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_selftest_lazy_g1(int op, const uint32_t *in, size_t n, uint32_t *out) {
    ZG_INIT();
    if (op < 0 || op >= LAZY_NOPS || !in || !out || n == 0 || n > (1u << 20))
        return invalid("zg_selftest_lazy_g1: invalid argument (op 0..9, 1 <= n <= 2^20, non-null records)");
    const size_t in_bytes = n * ZG_LAZY_IN_WORDS * sizeof(u32), out_bytes = n * ZG_LAZY_OUT_WORDS * sizeof(u32);
    Staging sg(lib_stream());
    const u32 *din = sg.in(in, in_bytes);
    u32 *dout = sg.out<u32>(out_bytes);
    if (sg.ok() && ZG_STAGE(sg, hipMemsetAsync(dout, 0, out_bytes, sg.st))) {
        if (op >= LAZY_MADD4)
            hipLaunchKernelGGL(lazy_g1_quad_kernel, dim3(div_up(4 * n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        else
            hipLaunchKernelGGL(lazy_g1_kernel, dim3(div_up(n, 64)), dim3(64), 0, sg.st, op, din, n, dout);
        sg.launched();
    }
    sg.fetch(out, dout, out_bytes);
    return sg.finish();
}

}  // extern "C"
