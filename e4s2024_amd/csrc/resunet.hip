// Row f9: the glue of the Blender recolouring network's Res-U-Net (swap_face_fine/Blender/model_center/res_u_net.py) between its convolutions, which run
// on conv.hip (e4s_conv2d_sb3).  Three streaming kernels, fp32 NCHW, no atomics, no host synchronisation; the same inputs give the same bits.
//   preact        : act = max(x * scale[c] + shift[c], 0)              the bn1 -> relu at the head of a ResBlock; the shortcut still needs x itself
//   up_cat_preact : u = bilinear x2 (align_corners) of low; act = relu(bn(cat(u, skip))); u is written too when the caller asks for it
//   head          : out = sigmoid(W[3, C] . x + b)                      the 1x1 output convolution: three outputs would waste conv.hip's 32-output tile
// Every kernel moves 16 bytes per lane along the pixel axis when the pointers are 16-byte aligned (and, for preact / head, the plane is a multiple of four
// pixels, so that the four share a channel and every plane starts aligned); otherwise one element per lane.  Both forms use the same expressions per element.
// e4s_id_affine with a zero slope is NOT the pre-activation bit for bit: it writes v * 0 = -0.0 for a negative v where max(v, 0) writes +0.0.
#include "common.h"

namespace e4s {

static inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

__device__ __forceinline__ float bn_relu(float v, float s, float t) { return fmaxf(fmaf(v, s, t), 0.f); }

// n: elements (V = 1) or groups of four along hw (V = 4, hw % 4 == 0)
template <int V>
__global__ __launch_bounds__(256) void resunet_preact_kernel(float* __restrict__ act, const float* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int64_t n, int C, int hwv) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = (int)((e / hwv) % C);
        const float s = scale[c], t = shift[c];
        if constexpr (V == 4) {
            const float4 v = reinterpret_cast<const float4*>(x)[e];
            reinterpret_cast<float4*>(act)[e] = make_float4(bn_relu(v.x, s, t), bn_relu(v.y, s, t), bn_relu(v.z, s, t), bn_relu(v.w, s, t));
        } else {
            act[e] = bn_relu(x[e], s, t);
        }
    }
}

// one output value of the x2 upsampling: e4s_bilinear_resize's coordinates and blend (bilinear_coord, bilinear_blend of common.h): the same bits
__device__ __forceinline__ float up2_sample(const float* __restrict__ p, int iw, int y0, int y1, float ly, int x, float sx) {
    int x0, x1;
    float lx;
    bilinear_coord(x, sx, 1, iw, x0, x1, lx);
    return bilinear_blend(p[(size_t)y0 * iw + x0], p[(size_t)y0 * iw + x1], p[(size_t)y1 * iw + x0], p[(size_t)y1 * iw + x1], ly, lx);
}

// A group is V consecutive elements of one output plane (2h x 2w = 4 h w elements: always a multiple of four, so with V = 4 no group straddles two planes
// and every plane starts 16-byte aligned when the tensor does; a group may run over a row end when 2w is not a multiple of four).  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void resunet_up_cat_preact_kernel(float* __restrict__ act, float* __restrict__ up, const float* __restrict__ low,
                                                                    const float* __restrict__ skip, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, int64_t n, int c_low, int c_skip, int h, int w,
                                                                    float sy, float sx) {
    const int C = c_low + c_skip, ow = 2 * w;
    const int64_t gpp = (int64_t)4 * h * w / V;                            // groups per plane
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t plane = g / gpp;
        const int i0 = (int)(g - plane * gpp) * V;                          // first element of the group within its plane
        const int b = (int)(plane / C), c = (int)(plane - (int64_t)b * C);
        const float s = scale[c], t = shift[c];
        float* dst = act + plane * gpp * V + i0;
        float v[V];
        if (c < c_low) {
            const int64_t lp = (int64_t)b * c_low + c;
            const float* p = low + lp * h * w;
            int y = i0 / ow, x = i0 - y * ow;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                int y0, y1;
                float ly;
                bilinear_coord(y, sy, 1, h, y0, y1, ly);
                v[j] = up2_sample(p, w, y0, y1, ly, x, sx);
                if (++x == ow) { x = 0; ++y; }
            }
            if (up) {
                float* ud = up + lp * gpp * V + i0;
                if constexpr (V == 4) *reinterpret_cast<float4*>(ud) = make_float4(v[0], v[1], v[2], v[3]);
                else ud[0] = v[0];
            }
        } else {
            const float* sp = skip + ((int64_t)b * c_skip + (c - c_low)) * gpp * V + i0;
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(sp);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = sp[0];
            }
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(bn_relu(v[0], s, t), bn_relu(v[1], s, t), bn_relu(v[2], s, t), bn_relu(v[3], s, t));
        else dst[0] = bn_relu(v[0], s, t);
    }
}

// n: pixels (V = 1) or groups of four pixels (V = 4, hw % 4 == 0) over the batch; the channel sum runs in channel order in both forms
template <int V>
__global__ __launch_bounds__(256) void resunet_head_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ wgt,
                                                           const float* __restrict__ bias, int64_t n, int C, int hwv) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / hwv;
        const int64_t p = (e - b * hwv) * V;
        const int64_t hw = (int64_t)hwv * V;
        const float* xp = x + b * C * hw + p;
        float acc[3][V];
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) acc[o][j] = bias[o];
        for (int c = 0; c < C; ++c) {
            float v[V];
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(xp + c * hw);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = xp[c * hw];
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const float wv = wgt[o * C + c];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[o][j] = fmaf(wv, v[j], acc[o][j]);
            }
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) r[j] = 1.f / (1.f + expf(-acc[o][j]));       // expf: the full-precision exponential
            float* op = out + (b * 3 + o) * hw + p;
            if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(r[0], r[1], r[2], r[3]);
            else op[0] = r[0];
        }
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_resunet_preact(float* act, const float* x, const float* scale, const float* shift, int bs, int C, int hw, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && hw >= 1, "resunet_preact: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(act && x && scale && shift, "resunet_preact: null tensor");
    const int64_t n = (int64_t)bs * C * hw;
    if (hw % 4 == 0 && aligned16(act, x))
        hipLaunchKernelGGL(resunet_preact_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, act, x, scale, shift, n / 4, C, hw / 4);
    else
        hipLaunchKernelGGL(resunet_preact_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, act, x, scale, shift, n, C, hw);
    return check_launch("resunet_preact");
}

extern "C" int e4s_resunet_up_cat_preact(float* act, float* up, const float* low, const float* skip, const float* scale, const float* shift, int bs,
                                         int c_low, int c_skip, int h, int w, void* stream) {
    E4S_REQUIRE(bs >= 0 && c_low >= 1 && c_skip >= 1 && h >= 1 && w >= 1 && h <= 8192 && w <= 8192, "resunet_up_cat_preact: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(act && low && skip && scale && shift, "resunet_up_cat_preact: null tensor");
    // F.upsample_bilinear: align_corners=True, (in - 1) / (out - 1) as e4s_bilinear_resize forms it; 0 / 1 = 0 when h == 1
    const float sy = (float)(h - 1) / (float)(2 * h - 1), sx = (float)(w - 1) / (float)(2 * w - 1);
    const int64_t n = (int64_t)bs * (c_low + c_skip) * 4 * h * w;
    if (aligned16(act, up, skip))
        hipLaunchKernelGGL(resunet_up_cat_preact_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, act, up, low, skip, scale, shift,
                           n / 4, c_low, c_skip, h, w, sy, sx);
    else
        hipLaunchKernelGGL(resunet_up_cat_preact_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, act, up, low, skip, scale, shift, n,
                           c_low, c_skip, h, w, sy, sx);
    return check_launch("resunet_up_cat_preact");
}

extern "C" int e4s_resunet_head(float* out, const float* x, const float* w, const float* b, int bs, int C, int hw, void* stream) {
    E4S_REQUIRE(bs >= 0 && hw >= 1, "resunet_head: bad size");
    E4S_REQUIRE(C == 64 || C == 16, "resunet_head: %d channels (64, or 16 for the small network)", C);
    if (bs == 0) return 0;
    E4S_REQUIRE(out && x && w && b, "resunet_head: null tensor");
    const int64_t n = (int64_t)bs * hw;
    if (hw % 4 == 0 && aligned16(out, x))
        hipLaunchKernelGGL(resunet_head_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, out, x, w, b, n / 4, C, hw / 4);
    else
        hipLaunchKernelGGL(resunet_head_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, x, w, b, n, C, hw);
    return check_launch("resunet_head");
}
