// LPIPS-AlexNet (criteria/lpips: lpips.py:28-34, networks.py:47-56 + 76-84, utils.py:6-9) — the parts of its forward pass and of its gradient with respect
// to the input image that conv.hip's split-bf16 convolutions do not cover:
//   conv1      Conv2d(3, 64, 11, stride 4, pad 2) + ReLU on the z-scored image (z = (x - mean) / std), optionally of its exact f x f box mean (f = 1, 2, 4:
//              the reference's adaptive_avg_pool2d to 1024 / 2^i); fp32 FMAs, one workgroup = 16 x 16 output pixels x all 64 channels
//   conv1 dgrad the stride-4 transposed convolution of conv1's (ReLU-masked) output gradient down to the three image channels, with the z-score and box-mean
//              backward fused: the gradient lands on the full-resolution image
//   maxpool    MaxPool2d(3, 2) without padding (floor mode); its backward is a GATHER (every input pixel collects from the <= 4 windows that chose it, the first
//              maximum in row-major window order as in PyTorch) fused with the tap's head gradient and the producing ReLU's mask
//   head       per tap: f / (sqrt(sum_c f^2 + 1e-16) + 1e-10) for x and y, the lin-weighted squared difference, mean over pixels, sum over the batch / batch size —
//              per-workgroup partial sums in a fixed order, summed by one workgroup (no float atomics: same inputs, same bits); the backward gives d/dfx (and d/dfy)
//   relu mask  g *= (a > 0) after a data-gradient convolution
// Convolutions 2 - 5 and their data gradients run on conv.hip (e4s_conv2d_sb3 forward, e4s_conv2d_sb on the flipped, transposed weights backward).
#include "common.h"
#include "targets.h"

using namespace e4s;

namespace {

constexpr int C1_K = 11, C1_S = 4, C1_P = 2, C1_CO = 64;
constexpr int C1_T = 16;                                                              // output tile side
constexpr int C1_PATCH = (C1_T - 1) * C1_S + C1_K;                                    // 71
constexpr int C1_PS = 72;                                                             // patch row stride

// z-scored value of scaled-image pixel (zy, zx) of channel c: the f x f box mean of x, then (v - mean) / std; 0 outside (the convolution's zero padding)
__device__ __forceinline__ float zval(const float* __restrict__ xc, int zy, int zx, int hs, int ws, int f, int w, float mu, float sd) {
    if (zy < 0 || zy >= hs || zx < 0 || zx >= ws) return 0.f;
    float s = 0.f;
    const float* r = xc + (size_t)zy * f * w + (size_t)zx * f;
    for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) s += r[(size_t)dy * w + dx];
    return (s / (float)(f * f) - mu) / sd;
}

// wt: [c][ky][kx][co] (363 x 64), the same for every workgroup; indices are wave-uniform so the weights come through the scalar cache
__global__ __launch_bounds__(256) void lpips_conv1_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, const float* __restrict__ wt, const float* __restrict__ bias,
                                                          int h, int w, int f, int ho, int wo, int tiles_x) {
    __shared__ float patch[3][C1_PATCH][C1_PS];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int oy0 = (blockIdx.x / tiles_x) * C1_T, ox0 = (blockIdx.x % tiles_x) * C1_T;
    const int hs = h / f, ws = w / f;
    const int zy0 = oy0 * C1_S - C1_P, zx0 = ox0 * C1_S - C1_P;
    for (int e = tid; e < 3 * C1_PATCH * C1_PATCH; e += 256) {
        const int c = e / (C1_PATCH * C1_PATCH), r = e - c * C1_PATCH * C1_PATCH;
        const int py = r / C1_PATCH, px = r - py * C1_PATCH;
        patch[c][py][px] = zval(x + ((size_t)b * 3 + c) * h * w, zy0 + py, zx0 + px, hs, ws, f, w, mean[c], stdv[c]);
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    float acc[C1_CO];
#pragma unroll
    for (int co = 0; co < C1_CO; ++co) acc[co] = 0.f;
    for (int c = 0; c < 3; ++c)
        for (int ky = 0; ky < C1_K; ++ky) {
            const float* prow = &patch[c][ty * C1_S + ky][tx * C1_S];
            const float* wr = wt + (size_t)((c * C1_K + ky) * C1_K) * C1_CO;
            for (int kx = 0; kx < C1_K; ++kx) {
                const float v = prow[kx];
#pragma unroll
                for (int co = 0; co < C1_CO; ++co) acc[co] = fmaf(v, wr[kx * C1_CO + co], acc[co]);
            }
        }
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy < ho && ox < wo) {
        float* o = out + (size_t)b * C1_CO * ho * wo + (size_t)oy * wo + ox;
#pragma unroll
        for (int co = 0; co < C1_CO; ++co) o[(size_t)co * ho * wo] = fmaxf(acc[co] + bias[co], 0.f);
    }
}

// Data gradient of conv1 down to the image.  Workgroup = 32 x 32 scaled-image pixels; wave wv takes the four stride phases (py, px) = p / 4, p % 4 for
// p = 4 wv .. 4 wv + 3, lane l the pixel (zy0 + py + 4 (l / 8), zx0 + px + 4 (l % 8)): within a phase every lane meets the same (ky, kx) set, ky = (py + 2) mod 4 + 4 i.
// g1: [bs][64][ho][wo], the ReLU-masked gradient of conv1's output.  gx [bs][3][h][w] = (dL/dz)[zy][zx] / (f^2 std[c]) over the f x f block (written, not added).
constexpr int D1_T = 32;
constexpr int D1_G = D1_T / C1_S + 3;     // 11 rows / cols of g1 reach a 32-pixel tile
__global__ __launch_bounds__(256) void lpips_conv1_dgrad_kernel(float* __restrict__ gx, const float* __restrict__ g1, const float* __restrict__ stdv,
                                                                const float* __restrict__ wt, int h, int w, int f, int ho, int wo, int tiles_x) {
    __shared__ float gt[C1_CO][D1_G][D1_G + 1];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int zy0 = (blockIdx.x / tiles_x) * D1_T, zx0 = (blockIdx.x % tiles_x) * D1_T;
    const int gy0 = zy0 / C1_S - 2, gx0 = zx0 / C1_S - 2;      // g1 row of tile row 0: (zy + 2 - ky) / 4 >= (zy0 + 2 - 10) / 4 = zy0 / 4 - 2
    const float* gb = g1 + (size_t)b * C1_CO * ho * wo;
    for (int e = tid; e < C1_CO * D1_G * D1_G; e += 256) {
        const int co = e / (D1_G * D1_G), r = e - co * D1_G * D1_G;
        const int ly = r / D1_G, lx = r - ly * D1_G;
        const int oy = gy0 + ly, ox = gx0 + lx;
        gt[co][ly][lx] = (oy >= 0 && oy < ho && ox >= 0 && ox < wo) ? gb[(size_t)co * ho * wo + (size_t)oy * wo + ox] : 0.f;
    }
    __syncthreads();
    const int hs = h / f, ws = w / f;
    const int lane = tid & 63, wv = tid >> 6;
    const float inv = 1.f / (float)(f * f);
    for (int q = 0; q < 4; ++q) {
        const int ph = wv * 4 + q;
        const int py = ph >> 2, px = ph & 3;
        const int zy = zy0 + py + 4 * (lane >> 3), zx = zx0 + px + 4 * (lane & 7);
        const int ky0 = (py + C1_P) & 3, kx0 = (px + C1_P) & 3;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int co = 0; co < C1_CO; ++co) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int ky = ky0 + 4 * i;
                if (ky >= C1_K) continue;
                const int ly = (zy + C1_P - ky) / C1_S - gy0;             // zy + 2 - ky is a multiple of 4 (phase): exact; 0 <= ly <= 10
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int kx = kx0 + 4 * j;
                    if (kx >= C1_K) continue;
                    const int lx = (zx + C1_P - kx) / C1_S - gx0;
                    const float g = gt[co][ly][lx];
                    const size_t k = (size_t)(ky * C1_K + kx) * C1_CO + co;
                    a0 = fmaf(g, wt[k], a0);
                    a1 = fmaf(g, wt[(size_t)C1_K * C1_K * C1_CO + k], a1);
                    a2 = fmaf(g, wt[(size_t)2 * C1_K * C1_K * C1_CO + k], a2);
                }
            }
        }
        if (zy < hs && zx < ws) {
            const float v[3] = {a0, a1, a2};
            for (int c = 0; c < 3; ++c) {
                const float g = v[c] * inv / stdv[c];
                float* o = gx + ((size_t)b * 3 + c) * h * w + (size_t)zy * f * w + (size_t)zx * f;
                for (int dy = 0; dy < f; ++dy)
                    for (int dx = 0; dx < f; ++dx) o[(size_t)dy * w + dx] = g;
            }
        }
    }
}

// MaxPool2d(3, stride 2), no padding
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(float* __restrict__ out, const float* __restrict__ a, int64_t n, int h, int w, int ho, int wo) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % wo);
        const int64_t r = i / wo;
        const int oy = (int)(r % ho);
        const int64_t pl = r / ho;
        const float* p = a + pl * h * w + (size_t)(2 * oy) * w + 2 * ox;
        float m = p[0];
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, p[(size_t)dy * w + dx]);
        out[i] = m;
    }
}

// g = ((add ? add : 0) + sum of gpool over the windows whose first maximum is this pixel) * (a > 0)
__global__ __launch_bounds__(256) void lpips_maxpool_bwd_kernel(float* __restrict__ g, const float* __restrict__ gpool, const float* __restrict__ add,
                                                                const float* __restrict__ a, int64_t n, int h, int w, int ho, int wo) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % w);
        const int64_t r = i / w;
        const int y = (int)(r % h);
        const int64_t pl = r / h;
        const float* ap = a + pl * h * w;
        float s = add ? add[i] : 0.f;
        const int oy_lo = y >= 2 ? (y - 1) / 2 : 0, oy_hi = min(y / 2, ho - 1);
        const int ox_lo = x >= 2 ? (x - 1) / 2 : 0, ox_hi = min(x / 2, wo - 1);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const float* p = ap + (size_t)(2 * oy) * w + 2 * ox;
                int best = 0;
                float m = p[0];
                for (int k = 1; k < 9; ++k) {
                    const float v = p[(size_t)(k / 3) * w + k % 3];
                    if (v > m) { m = v; best = k; }      // strict: the first maximum in row-major order keeps the window
                }
                if (2 * oy + best / 3 == y && 2 * ox + best % 3 == x) s += gpool[(pl * ho + oy) * wo + ox];
            }
        g[i] = ap[(size_t)y * w + x] > 0.f ? s : 0.f;
    }
}

// The head kernels: one workgroup = HP pixels x HS channel slices (lane group q = tid / HP sums channels q, q + HS, ...), the slices' partial sums
// combined in LDS in slice order — every thread of a pixel gets the same bits.  (One thread per pixel over all channels left the 63 x 63 taps
// with 16 workgroups and made the head the largest cost of the term.)
constexpr int HP = 32, HS = 8;

// sum over the HS slices of v, in slice order, for pixel column tid % HP (buf: HS x HP floats); ends with a barrier
__device__ __forceinline__ float slice_sum(float v, float* buf) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    float s = 0.f;
    for (int q = 0; q < HS; ++q) s += buf[q * HP + (tid % HP)];
    __syncthreads();
    return s;
}

// block sum of 256 values in a fixed order (LDS tree)
__device__ __forceinline__ float block_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// partial[b * gridDim.x + blockIdx.x] = scale * sum over the block's HP pixels of sum_c lin_c (fx_c / nx - fy_c / ny)^2
__global__ __launch_bounds__(256) void lpips_head_kernel(float* __restrict__ partial, const float* __restrict__ fx, const float* __restrict__ fy,
                                                         const float* __restrict__ lin, int c, int hw, float scale) {
#pragma clang fp contract(off)      // u nx - v ny must not become fma(u, nx, -v ny): x == y gives exactly 0
    __shared__ float buf[256];
    const int b = blockIdx.y, q = threadIdx.x / HP;
    const int p = blockIdx.x * HP + threadIdx.x % HP;
    const bool on = p < hw;
    const float* xp = fx + (size_t)b * c * hw + (on ? p : 0);
    const float* yp = fy + (size_t)b * c * hw + (on ? p : 0);
    float sx = 0.f, sy = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw], v = yp[(size_t)k * hw];
        sx = fmaf(u, u, sx);
        sy = fmaf(v, v, sy);
    }
    sx = slice_sum(sx, buf);
    sy = slice_sum(sy, buf);
    const float nx = 1.f / (sqrtf(sx + 1e-16f) + 1e-10f), ny = 1.f / (sqrtf(sy + 1e-16f) + 1e-10f);
    float d = 0.f;
    for (int k = q; k < c; k += HS) {
        const float t = xp[(size_t)k * hw] * nx - yp[(size_t)k * hw] * ny;
        d = fmaf(lin[k] * t, t, d);
    }
    d = slice_sum(d, buf);
    const float s = block_sum256(on && q == 0 ? d * scale : 0.f, buf);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void lpips_sum_kernel(float* __restrict__ loss, const float* __restrict__ partial, int n) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) loss[0] = s;
}

// d/dfx of scale * gout * sum_c lin_c (u_c - v_c)^2, u = fx / (r + 1e-10), r = sqrt(sum fx^2 + 1e-16):
//   gfx_k = a_k / n - fx_k / (n^2 r) sum_c a_c fx_c,  a_c = 2 scale gout lin_c (u_c - v_c);  gfy likewise with -a
__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(float* __restrict__ gx, float* __restrict__ gy, const float* __restrict__ fx,
                                                             const float* __restrict__ fy, const float* __restrict__ lin, const float* __restrict__ gout,
                                                             int c, int hw, float scale) {
#pragma clang fp contract(off)      // as in lpips_head_kernel: equal features give a = 0 exactly
    __shared__ float buf[256];
    const int b = blockIdx.y, q = threadIdx.x / HP;
    const int p = blockIdx.x * HP + threadIdx.x % HP;
    const bool on = p < hw;
    const size_t base = (size_t)b * c * hw + (on ? p : 0);
    const float* xp = fx + base;
    const float* yp = fy + base;
    float sx = 0.f, sy = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw], v = yp[(size_t)k * hw];
        sx = fmaf(u, u, sx);
        sy = fmaf(v, v, sy);
    }
    sx = slice_sum(sx, buf);
    sy = slice_sum(sy, buf);
    const float rx = sqrtf(sx + 1e-16f), ry = sqrtf(sy + 1e-16f);
    const float nx = 1.f / (rx + 1e-10f), ny = 1.f / (ry + 1e-10f);
    const float s2 = 2.f * scale * gout[0];
    float dx = 0.f, dy = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw], v = yp[(size_t)k * hw];
        const float a = s2 * lin[k] * (u * nx - v * ny);
        dx = fmaf(a, u, dx);
        dy = fmaf(a, v, dy);
    }
    dx = slice_sum(dx, buf);
    dy = slice_sum(dy, buf);
    if (!on) return;
    const float cx = dx * nx * nx / rx, cy = dy * ny * ny / ry;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw], v = yp[(size_t)k * hw];
        const float a = s2 * lin[k] * (u * nx - v * ny);
        gx[base + (size_t)k * hw] = a * nx - u * cx;
        if (gy) gy[base + (size_t)k * hw] = -a * ny + v * cy;
    }
}

// The multi-target heads: one read of fx against k targets (targets.h), target j weighted by w_j.  With k = 1 and w = 1 they give the single head's bits.
// partial[b * gridDim.x + blockIdx.x] = scale * sum over the block's HP pixels of sum_j w_j sum_c lin_c (fx_c / nx - fy_jc / ny_j)^2
__global__ __launch_bounds__(256) void lpips_head_multi_kernel(float* __restrict__ partial, const float* __restrict__ fx, const Targets tg,
                                                               const float* __restrict__ lin, int c, int hw, float scale) {
#pragma clang fp contract(off)      // as in lpips_head_kernel: x == y_j gives exactly 0 for that target
    __shared__ float buf[256];
    const int b = blockIdx.y, q = threadIdx.x / HP;
    const int p = blockIdx.x * HP + threadIdx.x % HP;
    const bool on = p < hw;
    const size_t off = (size_t)b * c * hw + (on ? p : 0);
    const float* xp = fx + off;
    float sx = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw];
        sx = fmaf(u, u, sx);
    }
    sx = slice_sum(sx, buf);
    const float nx = 1.f / (sqrtf(sx + 1e-16f) + 1e-10f);
    float tot = 0.f;
    for (int j = 0; j < tg.k; ++j) {
        const float* yp = target_base(tg, j) + off;
        float sy = 0.f;
        for (int k = q; k < c; k += HS) {
            const float v = yp[(size_t)k * hw];
            sy = fmaf(v, v, sy);
        }
        sy = slice_sum(sy, buf);
        const float ny = 1.f / (sqrtf(sy + 1e-16f) + 1e-10f);
        float d = 0.f;
        for (int k = q; k < c; k += HS) {
            const float t = xp[(size_t)k * hw] * nx - yp[(size_t)k * hw] * ny;
            d = fmaf(lin[k] * t, t, d);
        }
        d = slice_sum(d, buf);
        tot += tg.w[j] * d;
    }
    const float s = block_sum256(on && q == 0 ? tot * scale : 0.f, buf);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// gx = d/dfx of scale gout sum_j w_j sum_c lin_c (u_c - v_jc)^2 in one pass: with A_c = sum_j a_jc, a_jc = 2 scale gout w_j lin_c (u_c - v_jc),
//   gfx_c = A_c nx - fx_c nx^2 / rx sum_c' A_c' fx_c'   (the single head's formula is linear in a)
__global__ __launch_bounds__(256) void lpips_head_multi_bwd_kernel(float* __restrict__ gx, const float* __restrict__ fx, const Targets tg,
                                                                   const float* __restrict__ lin, const float* __restrict__ gout, int c, int hw, float scale) {
#pragma clang fp contract(off)
    __shared__ float buf[256];
    const int b = blockIdx.y, q = threadIdx.x / HP;
    const int p = blockIdx.x * HP + threadIdx.x % HP;
    const bool on = p < hw;
    const size_t off = (size_t)b * c * hw + (on ? p : 0);
    const float* xp = fx + off;
    float sx = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw];
        sx = fmaf(u, u, sx);
    }
    sx = slice_sum(sx, buf);
    const float rx = sqrtf(sx + 1e-16f);
    const float nx = 1.f / (rx + 1e-10f);
    const float s2 = 2.f * scale * gout[0];
    const float* yp[MAX_TARGETS];
    float ny[MAX_TARGETS], sw[MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < MAX_TARGETS; ++j) {
        yp[j] = xp;
        ny[j] = 0.f;
        sw[j] = 0.f;
        if (j < tg.k) {
            yp[j] = target_base(tg, j) + off;
            float sy = 0.f;
            for (int k = q; k < c; k += HS) {
                const float v = yp[j][(size_t)k * hw];
                sy = fmaf(v, v, sy);
            }
            sy = slice_sum(sy, buf);
            ny[j] = 1.f / (sqrtf(sy + 1e-16f) + 1e-10f);
            sw[j] = s2 * tg.w[j];
        }
    }
    const int nt = tg.k;
    auto A = [&](int k, float u) {
        float a = sw[0] * lin[k] * (u * nx - yp[0][(size_t)k * hw] * ny[0]);
#pragma unroll
        for (int j = 1; j < MAX_TARGETS; ++j)
            if (j < nt) a += sw[j] * lin[k] * (u * nx - yp[j][(size_t)k * hw] * ny[j]);
        return a;
    };
    float dx = 0.f;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw];
        dx = fmaf(A(k, u), u, dx);
    }
    dx = slice_sum(dx, buf);
    if (!on) return;
    const float cx = dx * nx * nx / rx;
    for (int k = q; k < c; k += HS) {
        const float u = xp[(size_t)k * hw];
        gx[off + (size_t)k * hw] = A(k, u) * nx - u * cx;
    }
}

__global__ __launch_bounds__(256) void lpips_relu_mask_kernel(float* __restrict__ g, const float* __restrict__ a, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (!(a[i] > 0.f)) g[i] = 0.f;
}

int grid_for(int64_t n) { return (int)(cdiv64(n, 256) < 65536 ? cdiv64(n, 256) : 65536); }

int conv1_out(int side) { return (side + 2 * C1_P - C1_K) / C1_S + 1; }

}  // namespace

extern "C" int e4s_lpips_conv1(float* out, const float* x, const float* mean, const float* stdv, const float* wt, const float* bias, int bs, int h, int w,
                               int f, void* stream) {
    E4S_REQUIRE(out && x && mean && stdv && wt && bias, "lpips_conv1: null tensor");
    E4S_REQUIRE(f == 1 || f == 2 || f == 4, "lpips_conv1: box factor %d (1, 2 or 4)", f);
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && h % f == 0 && w % f == 0, "lpips_conv1: bad size");
    const int hs = h / f, ws = w / f;
    E4S_REQUIRE(hs + 2 * C1_P >= C1_K && ws + 2 * C1_P >= C1_K, "lpips_conv1: image smaller than the kernel");
    if (bs == 0) return 0;
    const int ho = conv1_out(hs), wo = conv1_out(ws);
    const int tx = cdiv(wo, C1_T), ty = cdiv(ho, C1_T);
    hipLaunchKernelGGL(lpips_conv1_kernel, dim3(tx * ty, 1, bs), dim3(256), 0, (hipStream_t)stream, out, x, mean, stdv, wt, bias, h, w, f, ho, wo, tx);
    return check_launch("lpips_conv1");
}

extern "C" int e4s_lpips_conv1_dgrad(float* gx, const float* g1, const float* stdv, const float* wt, int bs, int h, int w, int f, void* stream) {
    E4S_REQUIRE(gx && g1 && stdv && wt, "lpips_conv1_dgrad: null tensor");
    E4S_REQUIRE(f == 1 || f == 2 || f == 4, "lpips_conv1_dgrad: box factor %d (1, 2 or 4)", f);
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && h % f == 0 && w % f == 0, "lpips_conv1_dgrad: bad size");
    const int hs = h / f, ws = w / f;
    E4S_REQUIRE(hs + 2 * C1_P >= C1_K && ws + 2 * C1_P >= C1_K, "lpips_conv1_dgrad: image smaller than the kernel");
    if (bs == 0) return 0;
    const int ho = conv1_out(hs), wo = conv1_out(ws);
    const int tx = cdiv(ws, D1_T), ty = cdiv(hs, D1_T);
    hipLaunchKernelGGL(lpips_conv1_dgrad_kernel, dim3(tx * ty, 1, bs), dim3(256), 0, (hipStream_t)stream, gx, g1, stdv, wt, h, w, f, ho, wo, tx);
    return check_launch("lpips_conv1_dgrad");
}

extern "C" int e4s_lpips_maxpool(float* out, const float* a, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(out && a, "lpips_maxpool: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 3 && w >= 3, "lpips_maxpool: bad size (at least 3 x 3)");
    const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
    const int64_t n = (int64_t)planes * ho * wo;
    if (n == 0) return 0;
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, a, n, h, w, ho, wo);
    return check_launch("lpips_maxpool");
}

extern "C" int e4s_lpips_maxpool_bwd_relu(float* g, const float* gpool, const float* add, const float* a, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(g && gpool && a, "lpips_maxpool_bwd_relu: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 3 && w >= 3, "lpips_maxpool_bwd_relu: bad size (at least 3 x 3)");
    const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
    const int64_t n = (int64_t)planes * h * w;
    if (n == 0) return 0;
    hipLaunchKernelGGL(lpips_maxpool_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, gpool, add, a, n, h, w, ho, wo);
    return check_launch("lpips_maxpool_bwd_relu");
}

extern "C" int e4s_lpips_head(float* partial, const float* fx, const float* fy, const float* lin, int bs, int c, int hw, float scale, void* stream) {
    E4S_REQUIRE(partial && fx && fy && lin, "lpips_head: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && c >= 1 && hw >= 1, "lpips_head: bad size");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(lpips_head_kernel, dim3(cdiv(hw, HP), bs), dim3(256), 0, (hipStream_t)stream, partial, fx, fy, lin, c, hw, scale);
    return check_launch("lpips_head");
}

extern "C" int e4s_lpips_sum(float* loss, const float* partial, int n, void* stream) {
    E4S_REQUIRE(loss && partial && n >= 1, "lpips_sum: bad arguments");
    hipLaunchKernelGGL(lpips_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, partial, n);
    return check_launch("lpips_sum");
}

extern "C" int e4s_lpips_head_bwd(float* gx, float* gy, const float* fx, const float* fy, const float* lin, const float* gout, int bs, int c, int hw,
                                  float scale, void* stream) {
    E4S_REQUIRE(gx && fx && fy && lin && gout, "lpips_head_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && c >= 1 && hw >= 1, "lpips_head_bwd: bad size");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3(cdiv(hw, HP), bs), dim3(256), 0, (hipStream_t)stream, gx, gy, fx, fy, lin, gout, c, hw, scale);
    return check_launch("lpips_head_bwd");
}

extern "C" int e4s_lpips_head_multi(float* partial, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                    const float* lin, int bs, int c, int hw, float scale, void* stream) {
    E4S_REQUIRE(partial && fx && lin, "lpips_head_multi: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && c >= 1 && hw >= 1, "lpips_head_multi: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "lpips_head_multi")) return st;
    if (bs == 0) return 0;
    hipLaunchKernelGGL(lpips_head_multi_kernel, dim3(cdiv(hw, HP), bs), dim3(256), 0, (hipStream_t)stream, partial, fx, tg, lin, c, hw, scale);
    return check_launch("lpips_head_multi");
}

extern "C" int e4s_lpips_head_multi_bwd(float* gx, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                        const float* lin, const float* gout, int bs, int c, int hw, float scale, void* stream) {
    E4S_REQUIRE(gx && fx && lin && gout, "lpips_head_multi_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && c >= 1 && hw >= 1, "lpips_head_multi_bwd: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "lpips_head_multi_bwd")) return st;
    if (bs == 0) return 0;
    hipLaunchKernelGGL(lpips_head_multi_bwd_kernel, dim3(cdiv(hw, HP), bs), dim3(256), 0, (hipStream_t)stream, gx, fx, tg, lin, gout, c, hw, scale);
    return check_launch("lpips_head_multi_bwd");
}

extern "C" int e4s_lpips_relu_mask(float* g, const float* a, int64_t n, void* stream) {
    E4S_REQUIRE(g && a && n >= 0, "lpips_relu_mask: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(lpips_relu_mask_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, a, n);
    return check_launch("lpips_relu_mask");
}
