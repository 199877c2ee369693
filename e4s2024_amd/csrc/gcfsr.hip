// Row f25: face inpainting, stage 1 (e4s2024_amd/ops_inpaint.py) — what FaceInpaintingArch.forward (swap_face_fine/gcfsr_arch.py:1347-1540) and the two ends
// of inpainting() (swap_face_fine/face_inpainting.py:21-51) need beyond the kernels the library has: the caller's input (image / 255 outside the hole, the
// mask plane, the hole share), Norm2Scale of the two condition linears for every level at once, the scale-shift-activation epilogue of
// StyleConv_norm_scale_shift, the caller's uint8 tail, and the support of cv2.resize on the hole mask.  fp32 with the roundings written out (hipcc contracts by
// default), no atomics, no host synchronisation, grids from shapes alone: the same inputs give the same bits, and a sample of a batch gets the bits it gets alone.
#include <math.h>

#include "common.h"

using namespace e4s;

#define GCFSR_PARTS 64        // pieces a sample's pixels are counted in (the first level of the hole count)
#define GCFSR_MAX_LEVELS 8    // condition levels one launch covers: 16 .. 1024 are seven

// np.array(img) / 255. in float64, then .float()
__device__ __forceinline__ float gcfsr_unit(unsigned byte) { return (float)((double)byte / 255.0); }

// ------------------------------------------------------------------------------------ input
// x [bs][4][S][S]: planes 0..2 = fl32(double(byte) / 255.0) * (1 - m), plane 3 = m; part [bs][GCFSR_PARTS] = hole pixels of each piece.  A piece is `chunk`
// consecutive pixels; vec: chunk % 4 == 0, S * S % 4 == 0 and every pointer aligned, a lane then owns four pixels (12 image bytes, 4 mask bytes, four float4 stores).
__global__ __launch_bounds__(256) void gcfsr_input_kernel(float* __restrict__ x, int* __restrict__ part, const uint8_t* __restrict__ img,
                                                          const uint8_t* __restrict__ mask, int hw, int chunk, int vec) {
    __shared__ int wsum[4];
    const int b = blockIdx.y, piece = blockIdx.x;
    const int p0 = piece * chunk, p1 = min(p0 + chunk, hw);
    const uint8_t* ib = img + (int64_t)b * hw * 3;
    const uint8_t* mb = mask + (int64_t)b * hw;
    float* xb = x + (int64_t)b * 4 * hw;
    int n = 0;
    if (vec) {
        for (int p = p0 + threadIdx.x * 4; p < p1; p += 1024) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(mb + p);
            const uint32_t* ip = reinterpret_cast<const uint32_t*>(ib + (int64_t)p * 3);
            const uint32_t w0 = ip[0], w1 = ip[1], w2 = ip[2];
            const unsigned by[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255, (w1 >> 16) & 255, w1 >> 24,
                                     w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
            float v[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool m = ((m4 >> (8 * j)) & 255) != 0;
                n += m;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = m ? 0.f : gcfsr_unit(by[3 * j + c]);
                v[3][j] = m ? 1.f : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<float4*>(xb + (int64_t)c * hw + p) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
    } else {
        for (int p = p0 + threadIdx.x; p < p1; p += 256) {
            const bool m = mb[p] != 0;
            n += m;
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[(int64_t)c * hw + p] = m ? 0.f : gcfsr_unit(ib[(int64_t)p * 3 + c]);
            xb[(int64_t)3 * hw + p] = m ? 1.f : 0.f;
        }
    }
    // integer sums: any order gives the same count
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part[b * GCFSR_PARTS + piece] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// count [bs] = the sum of a sample's pieces; in_size [bs] = float(count) / float(S * S), one correctly rounded division (exact operands up to 4096 x 4096)
__global__ __launch_bounds__(64) void gcfsr_count_kernel(int* __restrict__ count, float* __restrict__ in_size, const int* __restrict__ part, int hw) {
    int n = part[blockIdx.x * GCFSR_PARTS + threadIdx.x];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (threadIdx.x == 0) {
        count[blockIdx.x] = n;
        in_size[blockIdx.x] = (float)n / (float)hw;
    }
}

extern "C" int e4s_gcfsr_input(float* x, int* count, float* in_size, int* part, const uint8_t* img, const uint8_t* mask, int bs, int S, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && S >= 1 && S <= 4096, "gcfsr_input: bad size (bs <= 65535, 1 <= S <= 4096)");
    if (bs == 0) return 0;
    E4S_REQUIRE(x && count && in_size && part && img && mask, "gcfsr_input: null tensor");
    const int hw = S * S;
    int chunk = cdiv(hw, GCFSR_PARTS);
    const int aligned = (((uintptr_t)x & 15) | ((uintptr_t)img & 3) | ((uintptr_t)mask & 3)) == 0 && (hw & 3) == 0;
    if (aligned) chunk = cdiv(chunk, 4) * 4;
    hipLaunchKernelGGL(gcfsr_input_kernel, dim3(GCFSR_PARTS, bs), dim3(256), 0, (hipStream_t)stream, x, part, img, mask, hw, chunk, aligned);
    hipLaunchKernelGGL(gcfsr_count_kernel, dim3(bs), dim3(64), 0, (hipStream_t)stream, count, in_size, (const int*)part, hw);
    return check_launch("gcfsr_input");
}

// ------------------------------------------------------------------------------------ condition: two EqualLinear(1, C) and Norm2Scale, every level at once
struct GcfsrLevels {
    const float* w1[GCFSR_MAX_LEVELS];
    const float* b1[GCFSR_MAX_LEVELS];
    const float* w2[GCFSR_MAX_LEVELS];
    const float* b2[GCFSR_MAX_LEVELS];
    int begin[GCFSR_MAX_LEVELS + 1];     // channel offsets of the levels in a table row
    int n;
};

__global__ __launch_bounds__(256) void gcfsr_condition_kernel(float* __restrict__ s1n, float* __restrict__ s2n, const float* __restrict__ in_size,
                                                              GcfsrLevels L, int total) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= total) return;
    int l = 0;
    while (l + 1 < L.n && i >= L.begin[l + 1]) ++l;
    const int c = i - L.begin[l];
    const float v = in_size[b];
    float s1 = L.w1[l][c] * v;
    s1 = s1 + L.b1[l][c];
    float s2 = L.w2[l][c] * v;
    s2 = s2 + L.b2[l][c];
    const float q1 = s1 * s1, q2 = s2 * s2;
    float n = q1 + q2;
    n = n + 1e-8f;
    const float r = 1.0f / sqrtf(n);                 // IEEE square root and division (hipcc's defaults for float32)
    s1n[(int64_t)b * total + i] = s1 * r;
    s2n[(int64_t)b * total + i] = s2 * r;
}

extern "C" int e4s_gcfsr_condition(float* s1n, float* s2n, const float* in_size, const float* const* w1, const float* const* b1, const float* const* w2,
                                   const float* const* b2, const int* channels, int levels, int bs, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && levels >= 1 && levels <= GCFSR_MAX_LEVELS, "gcfsr_condition: bad size (bs <= 65535, 1 .. %d levels)", GCFSR_MAX_LEVELS);
    E4S_REQUIRE(w1 && b1 && w2 && b2 && channels, "gcfsr_condition: null table");
    GcfsrLevels L;
    memset(&L, 0, sizeof(L));
    L.n = levels;
    int64_t total = 0;
    for (int l = 0; l < levels; ++l) {
        E4S_REQUIRE(channels[l] >= 1 && w1[l] && b1[l] && w2[l] && b2[l], "gcfsr_condition: level %d: null weights or no channels", l);
        L.w1[l] = w1[l], L.b1[l] = b1[l], L.w2[l] = w2[l], L.b2[l] = b2[l];
        L.begin[l] = (int)total;
        total += channels[l];
        E4S_REQUIRE(total <= (1 << 24), "gcfsr_condition: too many channels");
    }
    L.begin[levels] = (int)total;
    if (bs == 0) return 0;
    E4S_REQUIRE(s1n && s2n && in_size, "gcfsr_condition: null tensor");
    hipLaunchKernelGGL(gcfsr_condition_kernel, dim3(cdiv((int)total, 256), bs), dim3(256), 0, (hipStream_t)stream, s1n, s2n, in_size, L, (int)total);
    return check_launch("gcfsr_condition");
}

// ------------------------------------------------------------------------------------ scale, shift, bias, activation: the epilogue of StyleConv_norm_scale_shift
// y <- lrelu(((y * s1) + (shift * s2)) + bias, 0.2) * sqrt(2), every operation rounded on its own: out * scale1 + shift * scale2, then FusedLeakyReLU.
__device__ __forceinline__ float gcfsr_ssa_value(float y, float sh, float s1, float s2, float bias) {
#pragma clang fp contract(off)
    const float a = y * s1, c = sh * s2;
    float t = a + c;
    t = t + bias;
    t = t < 0.f ? t * 0.2f : t;
    return t * 1.41421354f;                          // float32(2 ** 0.5)
}

// One workgroup owns up to 4096 consecutive elements of one plane (b, c): the plane's three scalars have workgroup-uniform addresses (scalar loads).
__global__ __launch_bounds__(256) void gcfsr_ssa_kernel(float* __restrict__ y, const float* __restrict__ shift, const float* __restrict__ s1n,
                                                        const float* __restrict__ s2n, const float* __restrict__ bias, int C, int hw, int64_t table_stride,
                                                        int vec) {
    const int c = blockIdx.y, b = blockIdx.z;
    const float s1 = s1n[b * table_stride + c], s2 = s2n[b * table_stride + c], bi = bias[c];
    const int64_t base = ((int64_t)b * C + c) * hw;
    const int p0 = blockIdx.x * 4096, p1 = min(p0 + 4096, hw);
    if (vec) {
        for (int p = p0 + threadIdx.x * 4; p < p1; p += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(y + base + p), s = *reinterpret_cast<const float4*>(shift + base + p);
            *reinterpret_cast<float4*>(y + base + p) = make_float4(gcfsr_ssa_value(v.x, s.x, s1, s2, bi), gcfsr_ssa_value(v.y, s.y, s1, s2, bi),
                                                                   gcfsr_ssa_value(v.z, s.z, s1, s2, bi), gcfsr_ssa_value(v.w, s.w, s1, s2, bi));
        }
    } else {
        for (int p = p0 + threadIdx.x; p < p1; p += 256) y[base + p] = gcfsr_ssa_value(y[base + p], shift[base + p], s1, s2, bi);
    }
}

extern "C" int e4s_gcfsr_scale_shift_act(float* y, const float* shift, const float* s1n, const float* s2n, const float* bias, int bs, int C, int hw,
                                         int64_t table_stride, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && C <= 65535 && hw >= 1 && table_stride >= C, "gcfsr_scale_shift_act: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(y && shift && s1n && s2n && bias, "gcfsr_scale_shift_act: null tensor");
    const int vec = (hw & 3) == 0 && (((uintptr_t)y | (uintptr_t)shift) & 15) == 0;
    hipLaunchKernelGGL(gcfsr_ssa_kernel, dim3(cdiv(hw, 4096), C, bs), dim3(256), 0, (hipStream_t)stream, y, shift, s1n, s2n, bias, C, hw, table_stride, vec);
    return check_launch("gcfsr_scale_shift_act");
}

// ------------------------------------------------------------------------------------ tail
// out uint8 [bs][S][S][3] = rint((x * (1 - m) + clamp(img, 0, 1) * m) * 255.0f), half to even; with m in {0, 1} the sum is x or the clamped value exactly.
__device__ __forceinline__ unsigned gcfsr_tail_value(float o, unsigned byte, bool m) {
#pragma clang fp contract(off)
    const float v = m ? fminf(fmaxf(o, 0.f), 1.f) : gcfsr_unit(byte);
    return (unsigned)rintf(v * 255.0f);
}

__global__ __launch_bounds__(256) void gcfsr_tail_kernel(uint8_t* __restrict__ out, const float* __restrict__ img, const uint8_t* __restrict__ in_u8,
                                                         const uint8_t* __restrict__ mask, int hw, int vec) {
    const int b = blockIdx.y;
    const float* ib = img + (int64_t)b * 3 * hw;
    const uint8_t* ub = in_u8 + (int64_t)b * hw * 3;
    const uint8_t* mb = mask + (int64_t)b * hw;
    uint8_t* ob = out + (int64_t)b * hw * 3;
    if (vec) {
        for (int p = (blockIdx.x * 256 + threadIdx.x) * 4; p < hw; p += gridDim.x * 1024) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(mb + p);
            const uint32_t* up = reinterpret_cast<const uint32_t*>(ub + (int64_t)p * 3);
            const uint32_t w[3] = {up[0], up[1], up[2]};
            const float4 r = *reinterpret_cast<const float4*>(ib + p), g = *reinterpret_cast<const float4*>(ib + hw + p),
                         bl = *reinterpret_cast<const float4*>(ib + 2 * (int64_t)hw + p);
            const float o[12] = {r.x, g.x, bl.x, r.y, g.y, bl.y, r.z, g.z, bl.z, r.w, g.w, bl.w};
            uint32_t q[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const bool m = ((m4 >> (8 * (k / 3))) & 255) != 0;
                q[k >> 2] |= gcfsr_tail_value(o[k], (w[k >> 2] >> (8 * (k & 3))) & 255, m) << (8 * (k & 3));
            }
            uint32_t* op = reinterpret_cast<uint32_t*>(ob + (int64_t)p * 3);
            op[0] = q[0], op[1] = q[1], op[2] = q[2];
        }
    } else {
        for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
            const bool m = mb[p] != 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) ob[(int64_t)p * 3 + c] = (uint8_t)gcfsr_tail_value(ib[(int64_t)c * hw + p], ub[(int64_t)p * 3 + c], m);
        }
    }
}

extern "C" int e4s_gcfsr_tail(uint8_t* out, const float* img, const uint8_t* in_u8, const uint8_t* mask, int bs, int S, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && S >= 1 && S <= 4096, "gcfsr_tail: bad size (bs <= 65535, 1 <= S <= 4096)");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img && in_u8 && mask, "gcfsr_tail: null tensor");
    const int hw = S * S;
    const int vec = (hw & 3) == 0 && (((uintptr_t)img & 15) | ((uintptr_t)out & 3) | ((uintptr_t)in_u8 & 3) | ((uintptr_t)mask & 3)) == 0;
    const int blocks = min(cdiv(vec ? hw / 4 : hw, 256), 1024);
    hipLaunchKernelGGL(gcfsr_tail_kernel, dim3(blocks, bs), dim3(256), 0, (hipStream_t)stream, out, img, in_u8, mask, hw, vec);
    return check_launch("gcfsr_tail");
}

// ------------------------------------------------------------------------------------ the support of cv2.resize on a non-negative mask
// out [bs][S][S] = 1 where any source pixel of rows ystart[y] .. + ycount[y] - 1, columns xstart[x] .. + xcount[x] - 1 is > 0.  The tables are clamped here: no
// table content makes an access leave the mask.
template <class T>
__global__ __launch_bounds__(256) void cv_mask_support_kernel(uint8_t* __restrict__ out, const T* __restrict__ mask, const int* __restrict__ ystart,
                                                              const int* __restrict__ ycount, const int* __restrict__ xstart, const int* __restrict__ xcount,
                                                              int64_t n, int H, int W, int S) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % S), y = (int)((i / S) % S);
        const int64_t b = i / ((int64_t)S * S);
        const int y0 = min(max(ystart[y], 0), H - 1), x0 = min(max(xstart[x], 0), W - 1);
        const int y1 = min(y0 + min(max(ycount[y], 1), 2), H), x1 = min(x0 + min(max(xcount[x], 1), 2), W);
        const T* mb = mask + b * H * W;
        bool any = false;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) any = any || (mb[(int64_t)yy * W + xx] > (T)0);
        out[i] = any ? 1 : 0;
    }
}

extern "C" int e4s_cv_mask_support(uint8_t* out, const void* mask, int is_f32, const int* ystart, const int* ycount, const int* xstart, const int* xcount, int bs,
                                   int H, int W, int S, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && S >= 1 && H <= 16384 && W <= 16384 && S <= 16384, "cv_mask_support: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && mask && ystart && ycount && xstart && xcount, "cv_mask_support: null tensor");
    const int64_t n = (int64_t)bs * S * S;
    if (is_f32)
        hipLaunchKernelGGL(cv_mask_support_kernel<float>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, (const float*)mask, ystart, ycount, xstart,
                           xcount, n, H, W, S);
    else
        hipLaunchKernelGGL(cv_mask_support_kernel<uint8_t>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, (const uint8_t*)mask, ystart, ycount, xstart,
                           xcount, n, H, W, S);
    return check_launch("cv_mask_support");
}
