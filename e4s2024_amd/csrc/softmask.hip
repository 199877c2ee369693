// f6 (the two-image caller): the soft paste masks and the uint8 blends of Face_swap_with_two_imgs.py's paste-back, on the device.
//   e4s_soft_erosion : SoftErosion.forward (utils/paste_back_tricks.py:17-43) per plane — a k x k cone-weighted convolution (zero padding k/2),
//                      `iterations - 1` times x = min(x, conv(x)), then c = conv(x); hard = c >= threshold; soft = 1 where hard, else c / max(c over
//                      the not-hard pixels of the plane).  The maximum never leaves the device: every workgroup of the last convolution writes the
//                      maximum of its own tile into scratch, and the normalising pass reduces its plane's partials again (in a fixed order, for any input).
//   e4s_blend_u8     : Trick.blending_two_images_with_mask (:131-147) on uint8 frames, in numpy's float32 arithmetic (no FMA contraction).
// The stencil is LDS-bound, not HBM-bound (k = 15: 225 multiply-adds per 4 bytes in and 4 out): a 64 x 32 output tile with its k/2 halo lies in LDS, one wave
// per 64-pixel row segment so that every ds_read_b32 of a wave covers 64 consecutive dwords (conflict-free), and each thread carries SE_R = 8 vertically
// adjacent outputs: one LDS read feeds up to 8 multiply-adds (k + 7 reads per 8 k of them), the weights of a kernel column sit in scalar registers.
#include <math.h>

#include "common.h"

using namespace e4s;

namespace {

constexpr int SE_TW = 64;                  // tile width  = the wave
constexpr int SE_R = 8;                    // outputs per thread (vertical)
constexpr int SE_TH = 4 * SE_R;            // tile height = 4 waves x SE_R rows
constexpr int SE_MAXK = 33;

// LAST = false: out = min(x, conv(x)).  LAST = true: out = conv(x), hard = out >= threshold, partial[plane][tile] = max(out over the tile's not-hard pixels)
// (-inf for a tile that has none).  wt: the weights TRANSPOSED, wt[kx * K + ky].
template <int K, bool LAST>
__global__ __launch_bounds__(256) void soft_erosion_conv_kernel(float* __restrict__ out, uint8_t* __restrict__ hard, float* __restrict__ partial,
                                                                const float* __restrict__ x, const float* __restrict__ wt, int h, int w, float threshold) {
    constexpr int P = K / 2;
    constexpr int LW = SE_TW + K - 1, LH = SE_TH + K - 1;
    __shared__ float tile[LH * LW];
    __shared__ float wave_part[4];
    const int plane = blockIdx.z;
    const int x0 = blockIdx.x * SE_TW, y0 = blockIdx.y * SE_TH;
    const float* __restrict__ src = x + (size_t)plane * h * w;
    for (int e = threadIdx.x; e < LH * LW; e += 256) {
        const int py = e / LW, px = e - py * LW;
        const int gy = y0 - P + py, gx = x0 - P + px;
        tile[e] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? src[(size_t)gy * w + gx] : 0.f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * SE_R;
    float acc[SE_R];
#pragma unroll
    for (int r = 0; r < SE_R; ++r) acc[r] = 0.f;
    const float* col = tile + ty * LW + tx;
#pragma unroll 1          // (unrolled over kx as well, k = 7 .. 11 take 106 .. 207 VGPRs: 2 to 4 waves per SIMD instead of 8)
    for (int kx = 0; kx < K; ++kx) {
        const float* __restrict__ wk = wt + kx * K;
#pragma unroll
        for (int j = 0; j < K + SE_R - 1; ++j) {
            const float v = col[j * LW + kx];
#pragma unroll
            for (int r = 0; r < SE_R; ++r) {
                const int ky = j - r;
                if (ky >= 0 && ky < K) acc[r] = fmaf(v, wk[ky], acc[r]);
            }
        }
    }
    const int gx = x0 + tx;
    float below = -INFINITY;
#pragma unroll
    for (int r = 0; r < SE_R; ++r) {
        const int gy = y0 + ty + r;
        if (gx < w && gy < h) {
            const size_t o = ((size_t)plane * h + gy) * w + gx;
            if (LAST) {
                const bool hd = acc[r] >= threshold;
                out[o] = acc[r];
                if (hard) hard[o] = hd ? 1 : 0;
                if (!hd) below = fmaxf(below, acc[r]);
            } else {
                out[o] = fminf(tile[(ty + r + P) * LW + tx + P], acc[r]);
            }
        }
    }
    if (LAST) {
        below = wave_max(below);
        if (tx == 0) wave_part[threadIdx.x >> 6] = below;
        __syncthreads();
        if (threadIdx.x == 0)
            partial[(size_t)plane * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] =
                fmaxf(fmaxf(wave_part[0], wave_part[1]), fmaxf(wave_part[2], wave_part[3]));
    }
}

// soft (holding c) -> 1 where c >= threshold, else c / m with m = the plane's maximum over its below-threshold pixels; m == 0 -> 0 (the reference: NaN).
// A plane without a below-threshold pixel has m = -inf and no pixel that would use it.
constexpr int SE_NORM_PER_BLOCK = 256 * 8;
__global__ __launch_bounds__(256) void soft_erosion_normalise_kernel(float* __restrict__ soft, const float* __restrict__ partial, int tiles, int hw,
                                                                     float threshold) {
    __shared__ float wave_part[4];
    const int plane = blockIdx.y;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < tiles; i += 256) m = fmaxf(m, partial[(size_t)plane * tiles + i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wave_part[0], wave_part[1]), fmaxf(wave_part[2], wave_part[3]));
    float* __restrict__ p = soft + (size_t)plane * hw;
    const int base = blockIdx.x * SE_NORM_PER_BLOCK;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < hw) {
            const float c = p[i];
            p[i] = c >= threshold ? 1.f : (m == 0.f ? 0.f : c / m);
        }
    }
}

template <int K>
void launch_conv(bool last, dim3 grid, hipStream_t st, float* out, uint8_t* hard, float* partial, const float* x, const float* wt, int h, int w,
                 float threshold) {
    if (last)
        hipLaunchKernelGGL((soft_erosion_conv_kernel<K, true>), grid, dim3(256), 0, st, out, hard, partial, x, wt, h, w, threshold);
    else
        hipLaunchKernelGGL((soft_erosion_conv_kernel<K, false>), grid, dim3(256), 0, st, out, hard, partial, x, wt, h, w, threshold);
}

void launch_conv_k(int k, bool last, dim3 grid, hipStream_t st, float* out, uint8_t* hard, float* partial, const float* x, const float* wt, int h, int w,
                   float threshold) {
    switch (k) {
#define SE_CASE(K) case K: launch_conv<K>(last, grid, st, out, hard, partial, x, wt, h, w, threshold); break;
        SE_CASE(3) SE_CASE(5) SE_CASE(7) SE_CASE(9) SE_CASE(11) SE_CASE(13) SE_CASE(15) SE_CASE(17) SE_CASE(19) SE_CASE(21) SE_CASE(23) SE_CASE(25)
        SE_CASE(27) SE_CASE(29) SE_CASE(31) SE_CASE(33)
#undef SE_CASE
    }
}

int64_t partial_floats(int planes, int h, int w) { return (int64_t)planes * cdiv(w, SE_TW) * cdiv(h, SE_TH); }
int64_t partial_floats_aligned(int planes, int h, int w) { return (partial_floats(planes, h, w) + 63) / 64 * 64; }

// numpy's float32 arithmetic: every product and sum rounded on its own.  hipcc contracts a * b + c into an FMA by default, and its __fmul_rn / __fadd_rn are
// plain operators that do not stop it: contraction is switched off for this kernel's body.
__global__ __launch_bounds__(256) void blend_u8_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ bottom, const uint8_t* __restrict__ up,
                                                       const float* __restrict__ mask, float up_ratio, int hw, int mask_channels) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int b = blockIdx.y;
    const size_t px = ((size_t)b * hw + i) * 3;
    const float* __restrict__ mp = mask + (size_t)b * mask_channels * hw + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float m = mp[mask_channels == 3 ? (size_t)c * hw : 0];
        if (m != m) m = 0.f;
        m = m * up_ratio;
        const float lo = (float)bottom[px + c] * (1.f - m), hi = (float)up[px + c] * m;
        const float s = lo + hi;
        out[px + c] = (uint8_t)fminf(fmaxf(s, 0.f), 255.f);
    }
}

}  // namespace

extern "C" int e4s_soft_erosion_scratch_bytes(int planes, int h, int w, int iterations, int64_t* bytes) {
    E4S_REQUIRE(bytes, "soft_erosion_scratch_bytes: null result");
    E4S_REQUIRE(planes >= 0 && planes <= 65535 && h >= 1 && w >= 1 && iterations >= 1, "soft_erosion_scratch_bytes: bad size");
    const int bufs = iterations >= 3 ? 2 : iterations - 1;
    *bytes = 4 * (partial_floats_aligned(planes, h, w) + (int64_t)bufs * planes * h * w);
    return 0;
}

extern "C" int e4s_soft_erosion(float* soft, uint8_t* hard, const float* x, const float* weights_t, float* scratch, int planes, int h, int w,
                                int kernel_size, float threshold, int iterations, void* stream) {
    E4S_REQUIRE(planes >= 0 && planes <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "soft_erosion: bad size (planes 0..65535, h * w <= 2^28)");
    E4S_REQUIRE(kernel_size >= 3 && kernel_size <= SE_MAXK && (kernel_size & 1), "soft_erosion: kernel_size %d is not an odd number in 3..%d", kernel_size,
                SE_MAXK);
    E4S_REQUIRE(iterations >= 1, "soft_erosion: iterations %d < 1", iterations);
    if (planes == 0) return 0;
    E4S_REQUIRE(soft && x && weights_t && scratch, "soft_erosion: null tensor");
    E4S_REQUIRE(cdiv(h, SE_TH) <= 65535, "soft_erosion: h too large");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(w, SE_TW), cdiv(h, SE_TH), planes);
    const size_t n = (size_t)planes * h * w;
    float* buf[2] = {scratch + partial_floats_aligned(planes, h, w), scratch + partial_floats_aligned(planes, h, w) + n};
    const float* cur = x;
    for (int it = 0; it + 1 < iterations; ++it) {          // x = min(x, conv(x))
        float* dst = buf[it & 1];
        launch_conv_k(kernel_size, false, grid, st, dst, nullptr, nullptr, cur, weights_t, h, w, threshold);
        cur = dst;
    }
    launch_conv_k(kernel_size, true, grid, st, soft, hard, scratch, cur, weights_t, h, w, threshold);
    const int hw = h * w;
    hipLaunchKernelGGL(soft_erosion_normalise_kernel, dim3(cdiv(hw, SE_NORM_PER_BLOCK), planes), dim3(256), 0, st, soft, scratch, (int)(grid.x * grid.y), hw,
                       threshold);
    return check_launch("soft_erosion");
}

extern "C" int e4s_blend_u8(uint8_t* out, const uint8_t* bottom, const uint8_t* up, const float* mask, float up_ratio, int n, int h, int w,
                            int mask_channels, void* stream) {
    E4S_REQUIRE(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "blend_u8: bad size (n 0..65535, h * w <= 2^28)");
    E4S_REQUIRE(mask_channels == 1 || mask_channels == 3, "blend_u8: mask_channels %d is not 1 or 3", mask_channels);
    E4S_REQUIRE(up_ratio >= 0.f && up_ratio <= 1.f, "blend_u8: up_ratio %g is not in [0, 1]", (double)up_ratio);
    if (n == 0) return 0;
    E4S_REQUIRE(out && bottom && up && mask, "blend_u8: null tensor");
    const int hw = h * w;
    hipLaunchKernelGGL(blend_u8_kernel, dim3(cdiv(hw, 256), n), dim3(256), 0, (hipStream_t)stream, out, bottom, up, mask, up_ratio, hw, mask_channels);
    return check_launch("blend_u8");
}
