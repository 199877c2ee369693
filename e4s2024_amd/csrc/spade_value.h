// One element of a SPADE modulation, shared by csrc/spade.hip (e4s_spade_modulate) and csrc/vid2vid.hip (e4s_v2v_spade_norm): the two kernels give the same bits
// because they run this one function.
#pragma once
#include <hip/hip_runtime.h>

namespace e4s {

// Every rounding written out (no contraction left to the compiler): the difference, its product with rstd, 1 + gamma, the product, the sum with beta, and the
// activation's product.  slope 1 is the identity (v * 1 is v, bit for bit).
__device__ __forceinline__ float spade_value(float x, float m, float r, float gamma, float beta, bool modulated, float slope) {
#pragma clang fp contract(off)
    float v = (x - m) * r;
    if (modulated) {
        const float g = 1.f + gamma;
        v = v * g;
        v = v + beta;
    }
    return v > 0.f ? v : v * slope;
}

}  // namespace e4s
