// Row f10: the glue of the Blender recolouring network's feature network (swap_face_fine/Blender/model_center/backbone.py, AdaptiveFeatureGenerator with its
// SPADE residual blocks, cmodules/architecture.py and cmodules/normalization.py) between its convolutions, which run on conv.hip (e4s_conv2d_sb3).  conv.hip
// pads with zeros only; the network's 3x3 convolutions inside the SPADE blocks see reflection padding, so both kernels here can WRITE reflection-padded planes
// [C][h + 2][w + 2] and the convolution then runs on those with pad = 0.  fp32 NCHW, no atomics, no host synchronisation, grids from the shapes alone: the same
// inputs give the same bits.
//   shared   : the first layer of every SPADE norm of a call in one launch (they all read the same image): nearest-neighbour pick of the image at h x w
//              (F.interpolate mode='nearest': floor(dst * (H / h)) in float32), reflection pad 1, 3 -> 128 N 3x3 convolution + bias, ReLU, written padded.
//              27 multiply-adds per output: a VALU kernel; a lane owns one padded position and walks a chunk of output channels whose weights are the same in
//              every lane.  A border position computes the interior position it mirrors, from the same inputs in the same order: the same bits.
//   modulate : out = act((x - mean) * rstd * (1 + gamma) + beta), gamma | beta the two halves [2C] of one convolution's output, or without them the plain
//              InstanceNorm; act = leaky 0.2 or identity; the output unpadded or reflection-padded by 1.  Every value is computed once, by the lane that owns
//              the interior element, and stored to every padded cell that mirrors it (up to nine for a corner's neighbour when h or w is 2 or 3).
//              Four elements of a row per lane with 16-byte loads when w % 4 == 0 and the pointers allow, one otherwise: the same expressions per element.
#include "common.h"
#include "spade_value.h"

namespace e4s {

static inline bool spade_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

// ReflectionPad2d(1): index -1 is 1, index n is n - 2 (n >= 2; with n == 2 the two sides read 1 and 0)
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

constexpr int SPADE_HIDDEN = 128;       // SPADE's nhidden (normalization.py: "Yes, hardcoded")
constexpr int SPADE_CHUNK = 32;         // output channels per workgroup

// grid (ceil((h + 2)(w + 2) / 256), N * 128 / 32, bs); actv [N][bs][128][h + 2][w + 2]: the slice of one norm is a contiguous batch for the convolution after it
__global__ __launch_bounds__(256) void spade_shared_kernel(float* __restrict__ actv, const float* __restrict__ img, const float* __restrict__ wgt,
                                                           const float* __restrict__ bias, int bs, int H, int W, int h, int w, float sy, float sx) {
    const int hp = h + 2, wp = w + 2;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hp * wp) return;
    const int b = blockIdx.z;
    const int y = reflect1(p / wp - 1, h), x = reflect1(p % wp - 1, w);
    float in[27];
    int rows[3], cols[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rows[k] = nearest_src(reflect1(y + k - 1, h), sy, H);
        cols[k] = nearest_src(reflect1(x + k - 1, w), sx, W);
    }
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) in[(ci * 3 + ky) * 3 + kx] = img[((size_t)(b * 3 + ci) * H + rows[ky]) * W + cols[kx]];
    const int co0 = blockIdx.y * SPADE_CHUNK;                                   // a chunk never straddles two norms: 128 % 32 == 0
    const int n = co0 / SPADE_HIDDEN, c0 = co0 % SPADE_HIDDEN;
    float* op = actv + (((size_t)n * bs + b) * SPADE_HIDDEN + c0) * hp * wp + p;
    for (int cc = 0; cc < SPADE_CHUNK; ++cc) {
        const float* wr = wgt + (size_t)(co0 + cc) * 27;                        // the same address in every lane
        float acc = bias[co0 + cc];
#pragma unroll
        for (int t = 0; t < 27; ++t) acc = fmaf(wr[t], in[t], acc);             // input channel, then row, then column: one definite order
        op[(size_t)cc * hp * wp] = fmaxf(acc, 0.f);
    }
}

// One element of the modulation is spade_value (spade_value.h), every rounding written out.

// A group is V consecutive elements of one row (V = 4: w % 4 == 0).  n: groups in all.  gb [bs][2C][h][w] or null.
template <int V, bool PAD>
__global__ __launch_bounds__(256) void spade_modulate_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gb, int64_t n, int C, int h, int w,
                                                             float slope) {
    const int hw = h * w, gpp = hw / V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t plane = g / gpp;
        const int i0 = (int)(g - plane * gpp) * V;
        const float m = mean[plane], r = rstd[plane];
        const float* xp = x + plane * hw + i0;
        float xv[V], ga[V], be[V], v[V];
        const float *gp = nullptr, *bp = nullptr;
        if (gb) {
            const int64_t b = plane / C, c = plane - b * C;
            gp = gb + ((b * 2 * C + c) * hw + i0);
            bp = gp + (int64_t)C * hw;
        }
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(xp);
            xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
            if (gb) {
                const float4 a = *reinterpret_cast<const float4*>(gp), c4 = *reinterpret_cast<const float4*>(bp);
                ga[0] = a.x; ga[1] = a.y; ga[2] = a.z; ga[3] = a.w;
                be[0] = c4.x; be[1] = c4.y; be[2] = c4.z; be[3] = c4.w;
            }
        } else {
            xv[0] = xp[0];
            if (gb) { ga[0] = gp[0]; be[0] = bp[0]; }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = spade_value(xv[j], m, r, gb ? ga[j] : 0.f, gb ? be[j] : 0.f, gb != nullptr, slope);
        if constexpr (!PAD) {
            float* op = out + plane * hw + i0;
            if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            else op[0] = v[0];
        } else {
            const int wp = w + 2;
            const int y = i0 / w, x0 = i0 - y * w;
            float* op = out + plane * (int64_t)(h + 2) * wp;
            // the padded rows that hold interior row y: its own, row 0 when y == 1, row h + 1 when y == h - 2 (both when h == 3 and y == 1; h == 2: 1 -> 0, 0 -> 3)
            int rows[3] = {y + 1, y == 1 ? 0 : -1, y == h - 2 ? h + 1 : -1};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (rows[k] < 0) continue;
                float* rp = op + (int64_t)rows[k] * wp;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int xx = x0 + j;
                    rp[xx + 1] = v[j];
                    if (xx == 1) rp[0] = v[j];
                    if (xx == w - 2) rp[w + 1] = v[j];
                }
            }
        }
    }
}

template <int V>
static void launch_modulate(bool pad, hipStream_t st, float* out, const float* x, const float* mean, const float* rstd, const float* gb, int64_t n, int C, int h,
                            int w, float slope) {
    if (pad) hipLaunchKernelGGL((spade_modulate_kernel<V, true>), dim3(grid_1d(n)), dim3(256), 0, st, out, x, mean, rstd, gb, n, C, h, w, slope);
    else hipLaunchKernelGGL((spade_modulate_kernel<V, false>), dim3(grid_1d(n)), dim3(256), 0, st, out, x, mean, rstd, gb, n, C, h, w, slope);
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_spade_shared(float* actv, const float* img, const float* weight, const float* bias, int bs, int nnorms, int H, int W, int h, int w,
                                void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && nnorms >= 1 && nnorms <= 64, "spade_shared: bad batch or number of norms");
    E4S_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "spade_shared: bad image size");
    E4S_REQUIRE(h >= 2 && w >= 2 && h <= 4096 && w <= 4096, "spade_shared: a %d x %d map: reflection padding needs at least 2 x 2 (at most 4096 x 4096)", h, w);
    if (bs == 0) return 0;
    E4S_REQUIRE(actv && img && weight && bias, "spade_shared: null tensor");
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;               // ATen compute_scales_value without a scale factor: in / out in float32
    const dim3 grid(cdiv((h + 2) * (w + 2), 256), nnorms * SPADE_HIDDEN / SPADE_CHUNK, bs);
    hipLaunchKernelGGL(spade_shared_kernel, grid, dim3(256), 0, (hipStream_t)stream, actv, img, weight, bias, bs, H, W, h, w, sy, sx);
    return check_launch("spade_shared");
}

extern "C" int e4s_spade_modulate(float* out, const float* x, const float* mean, const float* rstd, const float* gamma_beta, int bs, int C, int h, int w,
                                  int leaky, int padded, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "spade_modulate: bad size");
    E4S_REQUIRE(!padded || (h >= 2 && w >= 2), "spade_modulate: a %d x %d map: reflection padding needs at least 2 x 2", h, w);
    E4S_REQUIRE((leaky == 0 || leaky == 1) && (padded == 0 || padded == 1), "spade_modulate: leaky and padded are 0 or 1");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && x && mean && rstd, "spade_modulate: null tensor");
    const int64_t n = (int64_t)bs * C * h * w;
    const float slope = leaky ? 0.2f : 1.f;
    // the padded output is never read or written 16 bytes at a time (its rows start one element in), so its alignment does not matter
    if (w % 4 == 0 && spade_aligned16(x, gamma_beta, padded ? nullptr : out))
        launch_modulate<4>(padded != 0, (hipStream_t)stream, out, x, mean, rstd, gamma_beta, n / 4, C, h, w, slope);
    else
        launch_modulate<1>(padded != 0, (hipStream_t)stream, out, x, mean, rstd, gamma_beta, n, C, h, w, slope);
    return check_launch("spade_modulate");
}
