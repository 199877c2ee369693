// Face-parsing feature loss (criteria/face_parsing/face_parsing_loss.py on criteria/face_parsing/unet.py::unet(feature_scale=4).extract_feats) —
// the parts of its forward pass and of its gradient with respect to the input image that the existing kernels do not cover:
//   maxpool    MaxPool2d(2) between the encoder blocks, over planes of even size
//   tap bwd    one pass per block output c (= ReLU(BN(conv)), also the tap's feature): the tap's head gradient
//              -gout scale (fy / |y| - cos fx / |x|) / |x| (stats from e4s_id_head_sum), plus the gradient of the next block's input routed through the
//              2 x 2 max pool to the FIRST maximum of each window in row-major order (PyTorch's tie rule), times the ReLU mask (fx > 0) — the gradient at
//              the pre-activation of the block's second convolution, in one read of fx / fy / gpool and one write
// No float atomics: the same inputs give the same bits.  The input pooling (AdaptiveAvgPool2d(512)) and its adjoint run on idloss.hip's banded
// resampler, the heads on e4s_id_head_partial / e4s_id_head_sum, the convolutions on conv.hip (e4s_conv2d for the 3-channel input, e4s_conv2d_sb3
// forward, e4s_conv2d_sb data gradients on flipped, transposed weights) and the first convolution's ReLU mask on e4s_lpips_relu_mask.
#include "common.h"
#include "targets.h"

using namespace e4s;

namespace {

int grid_for(int64_t n) { return (int)(cdiv64(n, 256) < 65536 ? cdiv64(n, 256) : 65536); }

// out[p, i, j] = max of a[p, 2i .. 2i + 1, 2j .. 2j + 1]; one thread per output, two float2 loads
__global__ __launch_bounds__(256) void fp_maxpool2_kernel(float* __restrict__ out, const float* __restrict__ a, int64_t n, int w, int ho, int wo) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % wo), i = (int)((e / wo) % ho);
        const int64_t p = e / ((int64_t)ho * wo);
        const float* r0 = a + ((size_t)p * 2 * ho + 2 * i) * w + 2 * j;
        const float2 u = *reinterpret_cast<const float2*>(r0);
        const float2 v = *reinterpret_cast<const float2*>(r0 + w);
        out[e] = fmaxf(fmaxf(u.x, u.y), fmaxf(v.x, v.y));
    }
}

// One thread per 2 x 2 window (i, j) of plane p of sample b: g = (head gradient + [gpool routed to the window's first maximum]) * (fx > 0).
// fx, fy, g [bs][D] with D = C h w; gpool [bs][C][h / 2][w / 2] or NULL; stats (|x|, |y|, cos) [bs][3] of this tap.
__global__ __launch_bounds__(256) void fp_tap_bwd_kernel(float* __restrict__ g, const float* __restrict__ fx, const float* __restrict__ fy,
                                                         const float* __restrict__ stats, const float* __restrict__ gout, const float* __restrict__ gpool,
                                                         int64_t nwin, int h, int w, float scale) {
    const int b = blockIdx.y;
    const float nx = stats[(size_t)b * 3], ny = stats[(size_t)b * 3 + 1], c = stats[(size_t)b * 3 + 2];
    const float k = -gout[0] * scale / nx;
    const float ix = c / nx, iy = 1.f / ny;
    const int hw2 = w >> 1;
    const size_t base = (size_t)b * nwin * 4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nwin; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % hw2);
        const int64_t r = e / hw2;                       // plane * (h / 2) + window row
        const int i = (int)(r % (h >> 1));
        const int64_t p = r / (h >> 1);
        const size_t o0 = base + ((size_t)p * h + 2 * i) * w + 2 * j, o1 = o0 + w;
        const float2 x0 = *reinterpret_cast<const float2*>(fx + o0), x1 = *reinterpret_cast<const float2*>(fx + o1);
        const float2 y0 = *reinterpret_cast<const float2*>(fy + o0), y1 = *reinterpret_cast<const float2*>(fy + o1);
        float v[4] = {k * (y0.x * iy - x0.x * ix), k * (y0.y * iy - x0.y * ix), k * (y1.x * iy - x1.x * ix), k * (y1.y * iy - x1.y * ix)};
        const float xs[4] = {x0.x, x0.y, x1.x, x1.y};
        if (gpool) {
            int m = 0;                                   // first maximum in row-major order: a later element wins only if strictly larger
            float best = xs[0];
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (xs[q] > best) {
                    best = xs[q];
                    m = q;
                }
            const float gp = gpool[(size_t)b * nwin + e];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == m) v[q] += gp;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!(xs[q] > 0.f)) v[q] = 0.f;
        *reinterpret_cast<float2*>(g + o0) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(g + o1) = make_float2(v[2], v[3]);
    }
}

// fp_tap_bwd_kernel with the head gradient summed over k targets (targets.h): -gout scale sum_j w_j (fy_j / |y_j| - cos_j fx / |x|) / |x|, stats
// [bs][1 + 2 MAX_TARGETS] = (|x|, then |y_j|, cos_j per target) of this tap (e4s_id_head_sum_multi).
__global__ __launch_bounds__(256) void fp_tap_bwd_multi_kernel(float* __restrict__ g, const float* __restrict__ fx, const Targets tg,
                                                               const float* __restrict__ stats, const float* __restrict__ gout,
                                                               const float* __restrict__ gpool, int64_t nwin, int h, int w, float scale) {
    constexpr int MS = 1 + 2 * MAX_TARGETS;
    const int b = blockIdx.y;
    const float* st = stats + (size_t)b * MS;
    const float nx = st[0];
    const size_t base = (size_t)b * nwin * 4;
    const float* yp[MAX_TARGETS];
    float kk[MAX_TARGETS], ix[MAX_TARGETS], iy[MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < MAX_TARGETS; ++j) {
        const bool on = j < tg.k;
        yp[j] = on ? target_base(tg, j) + base : fx + base;
        kk[j] = on ? -gout[0] * scale * tg.w[j] / nx : 0.f;
        ix[j] = on ? st[2 + 2 * j] / nx : 0.f;
        iy[j] = on ? 1.f / st[1 + 2 * j] : 0.f;
    }
    const int nt = tg.k;
    const int hw2 = w >> 1;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nwin; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % hw2);
        const int64_t r = e / hw2;
        const int i = (int)(r % (h >> 1));
        const int64_t p = r / (h >> 1);
        const size_t o0 = ((size_t)p * h + 2 * i) * w + 2 * j, o1 = o0 + w;      // offsets within sample b
        const float2 x0 = *reinterpret_cast<const float2*>(fx + base + o0), x1 = *reinterpret_cast<const float2*>(fx + base + o1);
        const float xs[4] = {x0.x, x0.y, x1.x, x1.y};
        float v[4];
        {
            const float2 y0 = *reinterpret_cast<const float2*>(yp[0] + o0), y1 = *reinterpret_cast<const float2*>(yp[0] + o1);
            const float ys[4] = {y0.x, y0.y, y1.x, y1.y};
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = kk[0] * (ys[q] * iy[0] - xs[q] * ix[0]);
        }
#pragma unroll
        for (int t = 1; t < MAX_TARGETS; ++t)
            if (t < nt) {
                const float2 y0 = *reinterpret_cast<const float2*>(yp[t] + o0), y1 = *reinterpret_cast<const float2*>(yp[t] + o1);
                const float ys[4] = {y0.x, y0.y, y1.x, y1.y};
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] += kk[t] * (ys[q] * iy[t] - xs[q] * ix[t]);
            }
        if (gpool) {
            int m = 0;                                   // first maximum in row-major order, as in fp_tap_bwd_kernel
            float best = xs[0];
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (xs[q] > best) {
                    best = xs[q];
                    m = q;
                }
            const float gp = gpool[(size_t)b * nwin + e];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == m) v[q] += gp;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!(xs[q] > 0.f)) v[q] = 0.f;
        *reinterpret_cast<float2*>(g + base + o0) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(g + base + o1) = make_float2(v[2], v[3]);
    }
}

}  // namespace

extern "C" int e4s_fp_tap_bwd_multi(float* g, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                    const float* stats, const float* gout, const float* gpool, int bs, int C, int h, int w, float scale, void* stream) {
    E4S_REQUIRE(g && fx && stats && gout, "fp_tap_bwd_multi: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "fp_tap_bwd_multi: bad size (h, w even, >= 2)");
    E4S_REQUIRE((((uintptr_t)g | (uintptr_t)fx) & 7) == 0 && (fstride & 1) == 0, "fp_tap_bwd_multi: g, fx must be 8-byte aligned, the frame stride even");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "fp_tap_bwd_multi")) return st;
    for (int j = 0; j < k; ++j) E4S_REQUIRE((((uintptr_t)ys[j]) & 7) == 0, "fp_tap_bwd_multi: target %d must be 8-byte aligned", j);
    if (bs == 0) return 0;
    const int64_t nwin = (int64_t)C * (h / 2) * (w / 2);
    const int gx = (int)(cdiv64(nwin, 256) < 4096 ? cdiv64(nwin, 256) : 4096);
    hipLaunchKernelGGL(fp_tap_bwd_multi_kernel, dim3(gx, bs), dim3(256), 0, (hipStream_t)stream, g, fx, tg, stats, gout, gpool, nwin, h, w, scale);
    return check_launch("fp_tap_bwd_multi");
}

extern "C" int e4s_fp_maxpool2(float* out, const float* a, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(out && a, "fp_maxpool2: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "fp_maxpool2: bad size (h, w even, >= 2)");
    E4S_REQUIRE((((uintptr_t)a) & 7) == 0, "fp_maxpool2: the input must be 8-byte aligned");
    const int ho = h / 2, wo = w / 2;
    const int64_t n = (int64_t)planes * ho * wo;
    if (n == 0) return 0;
    hipLaunchKernelGGL(fp_maxpool2_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, a, n, w, ho, wo);
    return check_launch("fp_maxpool2");
}

extern "C" int e4s_fp_tap_bwd(float* g, const float* fx, const float* fy, const float* stats, const float* gout, const float* gpool, int bs, int C, int h,
                              int w, float scale, void* stream) {
    E4S_REQUIRE(g && fx && fy && stats && gout, "fp_tap_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "fp_tap_bwd: bad size (h, w even, >= 2)");
    E4S_REQUIRE((((uintptr_t)g | (uintptr_t)fx | (uintptr_t)fy) & 7) == 0, "fp_tap_bwd: g, fx, fy must be 8-byte aligned");
    if (bs == 0) return 0;
    const int64_t nwin = (int64_t)C * (h / 2) * (w / 2);
    const int gx = (int)(cdiv64(nwin, 256) < 4096 ? cdiv64(nwin, 256) : 4096);
    hipLaunchKernelGGL(fp_tap_bwd_kernel, dim3(gx, bs), dim3(256), 0, (hipStream_t)stream, g, fx, fy, stats, gout, gpool, nwin, h, w, scale);
    return check_launch("fp_tap_bwd");
}
