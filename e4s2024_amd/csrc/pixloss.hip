// The pixel term of calc_loss (training/video_swap_ft_coach.py:196-199, mse_loss of the foreground-weighted images) against k <= 4 targets at once
// (targets.h): sum_j w_j mean((x fg - y_j)^2), the targets y_j already weighted by the foreground (y fg), and its gradient with respect to x.
//   forward   one partial per PX_CHUNK pixels of a plane, in a fixed order; e4s_lpips_sum adds them up (no float atomics: same inputs, same bits)
//   backward  gx = gout 2 / n sum_j w_j (x fg - y_j) fg
#include "common.h"
#include "targets.h"

using namespace e4s;

namespace {

constexpr int PX_CHUNK = 4096;                  // elements of one plane per forward workgroup

// grid (ceil(hw / PX_CHUNK), bs C): workgroup (chunk, plane) sums its chunk of plane p = b C + c; x, y_j [bs C][hw], fg [bs][hw] or NULL (1)
__global__ __launch_bounds__(256) void pix_mse_multi_kernel(float* __restrict__ partial, const float* __restrict__ x, const float* __restrict__ fg,
                                                            const Targets tg, int C, int64_t hw, float inv_n) {
    __shared__ float red[256];
    const int64_t plane = blockIdx.y;
    const int64_t e0 = (int64_t)blockIdx.x * PX_CHUNK, e1 = min<int64_t>(hw, e0 + PX_CHUNK);
    const size_t base = (size_t)plane * hw;
    const float* mp = fg ? fg + (size_t)(plane / C) * hw : nullptr;
    const float* yp[MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < MAX_TARGETS; ++j) yp[j] = (j < tg.k ? target_base(tg, j) : x) + base;
    const int nt = tg.k;
    float s = 0.f;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const float a = x[base + e] * (mp ? mp[e] : 1.f);
#pragma unroll
        for (int j = 0; j < MAX_TARGETS; ++j)
            if (j < nt) {
                const float d = a - yp[j][e];
                s = fmaf(tg.w[j] * d, d, s);
            }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)plane * gridDim.x + blockIdx.x] = red[0] * inv_n;
}

// grid (x, bs C): plane p = blockIdx.y, its pixels strided over the x workgroups
__global__ __launch_bounds__(256) void pix_mse_multi_bwd_kernel(float* __restrict__ gx, const float* __restrict__ x, const float* __restrict__ fg,
                                                                const Targets tg, const float* __restrict__ gout, int C, int64_t hw, float inv_n) {
    const int64_t plane = blockIdx.y;
    const size_t base = (size_t)plane * hw;
    const float* mp = fg ? fg + (size_t)(plane / C) * hw : nullptr;
    const float* yp[MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < MAX_TARGETS; ++j) yp[j] = (j < tg.k ? target_base(tg, j) : x) + base;
    const int nt = tg.k;
    const float k2 = 2.f * gout[0] * inv_n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < hw; e += (int64_t)gridDim.x * 256) {
        const float m = mp ? mp[e] : 1.f;
        const float a = x[base + e] * m;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MAX_TARGETS; ++j)
            if (j < nt) s = fmaf(tg.w[j], a - yp[j][e], s);
        gx[base + e] = k2 * s * m;
    }
}

}  // namespace

extern "C" int e4s_pix_mse_multi(float* partial, const float* x, const float* fg, const float* const* ys, const float* tw, int k, const int* frame,
                                 int64_t fstride, int nframes, int bs, int C, int64_t hw, void* stream) {
    E4S_REQUIRE(partial && x, "pix_mse_multi: null tensor");
    E4S_REQUIRE(bs >= 1 && C >= 1 && (int64_t)bs * C <= 65535 && hw >= 1 && cdiv64(hw, PX_CHUNK) < (1 << 30), "pix_mse_multi: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "pix_mse_multi")) return st;
    const int64_t n = (int64_t)bs * C * hw;
    hipLaunchKernelGGL(pix_mse_multi_kernel, dim3((unsigned)cdiv64(hw, PX_CHUNK), bs * C), dim3(256), 0, (hipStream_t)stream, partial, x, fg, tg, C, hw,
                       (float)(1.0 / (double)n));
    return check_launch("pix_mse_multi");
}

extern "C" int e4s_pix_mse_multi_bwd(float* gx, const float* x, const float* fg, const float* const* ys, const float* tw, int k, const int* frame,
                                     int64_t fstride, int nframes, const float* gout, int bs, int C, int64_t hw, void* stream) {
    E4S_REQUIRE(gx && x && gout, "pix_mse_multi_bwd: null tensor");
    E4S_REQUIRE(bs >= 1 && C >= 1 && (int64_t)bs * C <= 65535 && hw >= 1, "pix_mse_multi_bwd: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "pix_mse_multi_bwd")) return st;
    const int64_t n = (int64_t)bs * C * hw;
    const int grid = (int)(cdiv64(hw, 256) < 1024 ? cdiv64(hw, 256) : 1024);
    hipLaunchKernelGGL(pix_mse_multi_bwd_kernel, dim3(grid, bs * C), dim3(256), 0, (hipStream_t)stream, gx, x, fg, tg, gout, C, hw, (float)(1.0 / (double)n));
    return check_launch("pix_mse_multi_bwd");
}
