// Row f12: what the GPEN generator (swap_face_fine/gpen/face_model/gpen_model.py: FullGenerator; face_gan.py: FaceGAN.img2tensor / tensor2img) needs beside
// the library's convolutions, modulated convolutions, FIR and linear kernels.  fp32 NCHW, no atomics, no host synchronisation, grids from the shapes alone: the
// same inputs give the same bits.
//   stem       : ecd0 = ConvLayer(3, C0, 1): the 1 x 1 EqualConv2d without bias and FusedLeakyReLU(C0) in one pass.  Three input channels would leave 29/32 of an
//                MFMA tile on zeros, so this is an exact-float32 VALU kernel: each output is bias[co], then one fused multiply-add per input channel in channel
//                order, then v > 0 ? v : 0.2 v, then * sqrt(2).  The weight [C0][3] carries the equalised-lr scale already.  The input is float [bs][3][H][W], or
//                uint8 [bs][H][W][3] (RGB) taken through FaceGAN.img2tensor first: v / 255 (a true division), - 0.5, / 0.5, each rounded on its own.
//   noise_half : the second half of a StyledConv's concatenated output (gpen_model.py:294-302, 350-356): out[b][C + c][p] = lrelu(fl(w f[b][c][p]) + bias[C + c])
//                * sqrt(2) with w the device scalar noise.weight; the product is rounded before the sum and the scale comes last, PyTorch's bits for
//                scale * F.leaky_relu(cat(out, w * noise) + bias).  One launch reads f once and serves the (up to) two layers of a resolution, each with its own
//                destination, w and bias; a destination is addressed by a batch stride, so it is planes [C, 2C) of a [bs][2C][h][w] buffer.
//   to_u8      : FaceGAN.tensor2img without the channel flip: float [bs][3][H][W] -> uint8 [bs][H][W][3] = uint8(clip(x * 0.5 + 0.5, 0, 1) * 255), every
//                operation rounded on its own, truncating.
// Every kernel moves 16 bytes per lane along a row (12 bytes of uint8 pixels) where the pointers and the row length allow and single elements otherwise, with
// the same expressions per element in both forms.
#include "common.h"

namespace e4s {

constexpr int GPEN_CPB = 16;                     // output channels of the stem per workgroup row (blockIdx.y)
constexpr float GPEN_SQRT2 = 1.41421356237309515f;

static inline bool gpen_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

// FaceGAN.img2tensor on one colour value, every rounding written out
__device__ __forceinline__ float gpen_unit(uint8_t v) {
#pragma clang fp contract(off)
    float a = (float)v / 255.f;
    a = a - 0.5f;
    return a / 0.5f;
}

__device__ __forceinline__ float gpen_lrelu(float v) {
#pragma clang fp contract(off)
    const float a = v > 0.f ? v : v * 0.2f;
    return a * GPEN_SQRT2;
}

// A group is V consecutive pixels of one image (V = 4: W % 4 == 0, so a group never leaves its row).  n: groups in all; hw: pixels of an image.
// blockIdx.y picks GPEN_CPB output channels.
template <int V, bool U8>
__global__ __launch_bounds__(256) void gpen_stem_kernel(float* __restrict__ out, const float* __restrict__ xf, const uint8_t* __restrict__ xu,
                                                        const float* __restrict__ weight, const float* __restrict__ bias, int64_t n, int64_t hw, int C0) {
    const int c_lo = blockIdx.y * GPEN_CPB;
    const int c_hi = c_lo + GPEN_CPB < C0 ? c_lo + GPEN_CPB : C0;
    const int64_t gpi = hw / V;                                                 // groups per image
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / gpi;
        const int64_t p = (g - b * gpi) * V;
        float x[3][V];
        if constexpr (U8) {
            const uint8_t* src = xu + (b * hw + p) * 3;
            if constexpr (V == 4) {
                const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);   // 12 bytes: the host checked the alignment
                const uint32_t q[3] = {s32[0], s32[1], s32[2]};
#pragma unroll
                for (int e = 0; e < 12; ++e) x[e % 3][e / 3] = gpen_unit((uint8_t)(q[e >> 2] >> (8 * (e & 3))));
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) x[c][0] = gpen_unit(src[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* src = xf + (b * 3 + c) * hw + p;
                if constexpr (V == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(src);
                    x[c][0] = q.x; x[c][1] = q.y; x[c][2] = q.z; x[c][3] = q.w;
                } else {
                    x[c][0] = src[0];
                }
            }
        }
        for (int co = c_lo; co < c_hi; ++co) {
            const float w0 = weight[co * 3], w1 = weight[co * 3 + 1], w2 = weight[co * 3 + 2], bi = bias[co];
            float r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float a = bi;
                a = __builtin_fmaf(w0, x[0][j], a);
                a = __builtin_fmaf(w1, x[1][j], a);
                a = __builtin_fmaf(w2, x[2][j], a);
                r[j] = gpen_lrelu(a);
            }
            float* op = out + (b * C0 + co) * hw + p;
            if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(r[0], r[1], r[2], r[3]);
            else op[0] = r[0];
        }
    }
}

__device__ __forceinline__ float gpen_noise_act(float f, float w, float bi) {
#pragma clang fp contract(off)
    const float t = w * f;
    return gpen_lrelu(t + bi);
}

// A group is V consecutive elements of one plane (V = 4: hw % 4 == 0).  n: groups in all.  out1 may be NULL.
template <int V>
__global__ __launch_bounds__(256) void gpen_noise_half_kernel(float* __restrict__ out0, float* __restrict__ out1, const float* __restrict__ f,
                                                              const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ bias0,
                                                              const float* __restrict__ bias1, int64_t n, int C, int64_t hw, int64_t stride_b) {
    const float wa = w0[0], wb = out1 ? w1[0] : 0.f;
    const int64_t gpp = hw / V;                                                 // groups per plane
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t plane = g / gpp;                                          // b * C + c
        const int64_t p = (g - plane * gpp) * V;
        const int64_t b = plane / C;
        const int c = (int)(plane - b * C);
        const int64_t dst = b * stride_b + (int64_t)c * hw + p;
        const float* src = f + plane * hw + p;
        const float ba = bias0[c];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            *reinterpret_cast<float4*>(out0 + dst) = make_float4(gpen_noise_act(q.x, wa, ba), gpen_noise_act(q.y, wa, ba), gpen_noise_act(q.z, wa, ba),
                                                                 gpen_noise_act(q.w, wa, ba));
            if (out1) {
                const float bb = bias1[c];
                *reinterpret_cast<float4*>(out1 + dst) = make_float4(gpen_noise_act(q.x, wb, bb), gpen_noise_act(q.y, wb, bb), gpen_noise_act(q.z, wb, bb),
                                                                     gpen_noise_act(q.w, wb, bb));
            }
        } else {
            const float q = src[0];
            out0[dst] = gpen_noise_act(q, wa, ba);
            if (out1) out1[dst] = gpen_noise_act(q, wb, bias1[c]);
        }
    }
}

// FaceGAN.tensor2img on one value, every rounding written out
__device__ __forceinline__ uint8_t gpen_level(float v) {
#pragma clang fp contract(off)
    float a = v * 0.5f;
    a = a + 0.5f;
    a = fminf(fmaxf(a, 0.f), 1.f);
    a = a * 255.f;
    return (uint8_t)a;
}

// A group is V consecutive pixels of one image (V = 4: W % 4 == 0).  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void gpen_to_u8_kernel(uint8_t* __restrict__ out, const float* __restrict__ x, int64_t n, int64_t hw) {
    const int64_t gpi = hw / V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / gpi;
        const int64_t p = (g - b * gpi) * V;
        uint8_t* dst = out + (b * hw + p) * 3;
        if constexpr (V == 4) {
            uint8_t u[12];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 q = *reinterpret_cast<const float4*>(x + (b * 3 + c) * hw + p);
                u[c] = gpen_level(q.x); u[3 + c] = gpen_level(q.y); u[6 + c] = gpen_level(q.z); u[9 + c] = gpen_level(q.w);
            }
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int k = 0; k < 3; ++k) d32[k] = (uint32_t)u[4 * k] | ((uint32_t)u[4 * k + 1] << 8) | ((uint32_t)u[4 * k + 2] << 16) | ((uint32_t)u[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = gpen_level(x[(b * 3 + c) * hw + p]);
        }
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_gpen_stem(float* out, const float* x, const uint8_t* x_u8, const float* weight, const float* bias, int bs, int C0, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && C0 >= 1 && C0 <= 65535 * GPEN_CPB && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "gpen_stem: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && weight && bias && ((x != nullptr) != (x_u8 != nullptr)), "gpen_stem: null tensor, or not exactly one of the float and the uint8 input");
    const int64_t hw = (int64_t)H * W, n = (int64_t)bs * hw;
    const int gy = cdiv(C0, GPEN_CPB);
    hipStream_t st = (hipStream_t)stream;
    if (x) {
        if (W % 4 == 0 && gpen_aligned16(out, x))
            hipLaunchKernelGGL((gpen_stem_kernel<4, false>), dim3(grid_1d(n / 4), gy), dim3(256), 0, st, out, x, x_u8, weight, bias, n / 4, hw, C0);
        else
            hipLaunchKernelGGL((gpen_stem_kernel<1, false>), dim3(grid_1d(n), gy), dim3(256), 0, st, out, x, x_u8, weight, bias, n, hw, C0);
    } else {
        if (W % 4 == 0 && gpen_aligned16(out) && (((uintptr_t)x_u8) & 3) == 0)
            hipLaunchKernelGGL((gpen_stem_kernel<4, true>), dim3(grid_1d(n / 4), gy), dim3(256), 0, st, out, x, x_u8, weight, bias, n / 4, hw, C0);
        else
            hipLaunchKernelGGL((gpen_stem_kernel<1, true>), dim3(grid_1d(n), gy), dim3(256), 0, st, out, x, x_u8, weight, bias, n, hw, C0);
    }
    return check_launch("gpen_stem");
}

extern "C" int e4s_gpen_noise_half(float* out0, float* out1, const float* f, const float* w0, const float* w1, const float* bias0, const float* bias1,
                                   int bs, int C, int hw, int64_t out_stride_b, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && hw >= 1 && out_stride_b >= (int64_t)C * hw, "gpen_noise_half: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out0 && f && w0 && bias0 && (!out1 || (w1 && bias1)), "gpen_noise_half: null tensor");
    const int64_t n = (int64_t)bs * C * hw;
    hipStream_t st = (hipStream_t)stream;
    if (hw % 4 == 0 && out_stride_b % 4 == 0 && gpen_aligned16(out0, out1, f))
        hipLaunchKernelGGL(gpen_noise_half_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, st, out0, out1, f, w0, w1, bias0, bias1, n / 4, C, (int64_t)hw, out_stride_b);
    else
        hipLaunchKernelGGL(gpen_noise_half_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, st, out0, out1, f, w0, w1, bias0, bias1, n, C, (int64_t)hw, out_stride_b);
    return check_launch("gpen_noise_half");
}

extern "C" int e4s_gpen_to_u8(uint8_t* out, const float* x, int bs, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "gpen_to_u8: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && x, "gpen_to_u8: null tensor");
    const int64_t hw = (int64_t)H * W, n = (int64_t)bs * hw;
    if (W % 4 == 0 && gpen_aligned16(x) && (((uintptr_t)out) & 3) == 0)
        hipLaunchKernelGGL(gpen_to_u8_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, out, x, n / 4, hw);
    else
        hipLaunchKernelGGL(gpen_to_u8_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, x, n, hw);
    return check_launch("gpen_to_u8");
}
