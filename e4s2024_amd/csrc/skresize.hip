// Row f24: the two ends of the whole-clip reenactment chain (face_swap_video_pipeline.py:248-253): skimage.transform.resize on a float64 image in front of
// make_animation, and (pred * 255).astype(np.uint8) behind it.  No atomics, no host synchronisation, no scratch memory, grids from the shapes alone: the same
// inputs give the same bits, and the calls can be captured in a graph.
//   minmax : the byte minimum and maximum of every sample in SK_PARTS pieces (skimage clips the result to the input image's own range, all channels together;
//            v -> v / 255.0 is monotonic, so the range is taken on the bytes).  The resize kernel merges the pieces.
//   resize : out = float32(clip(sum_y wy sum_x wx (double(byte) / 255.0))) on composite tables made on the host per axis (start int32 [dst], count int32 [dst],
//            weight float64 [dst][T]: the product of scipy.ndimage.zoom's order-1 'mirror' grid-mode matrix and gaussian_filter's mirror-folded, truncated,
//            normalised matrix).  Everything is float64 with one rounding per product and per sum (no contraction), summed in ascending source index from 0.0:
//            first along x, then along y.  A workgroup owns 16 x 32 output pixels.
//            LDS plan: the tile's source rows, at most SK_ROWS = 80 (at 16 output rows and 4f composite taps that is a shrink of up to about 4.2 : 1 per
//            axis, the 1024 -> 256 of the workload with its 14 taps; any enlargement), are each filtered along x ONCE into float64 [row][3][32] in LDS (60 KB),
//            and the y pass reads that.  The division by 255.0 is a 256-entry table in LDS, filled by the IEEE division itself.
//            Direct form: a tile whose rows do not fit is formed pixel by pixel from global memory, the x sum of every source row first and in the same order:
//            both forms give the same bits.  Limits: sides up to 16384, up to E4S_SK_MAX_TAPS = 1024 composite taps per axis (a shrink of about 255 : 1).
//            start and count are clamped to the source on the device: no table content makes an access leave a tensor.
//   frames : out uint8 [n][H][W][3] = (uint8)trunc(p * 255.0f) of float32 [n][3][H][W], the float32 product truncated toward zero and clamped to 0 .. 255 (a NaN
//            gives 0); `flip` stores the channels reversed.  Four pixels a lane (three 16-byte loads, three dword stores) where H W % 4 == 0 and the pointers
//            allow it, one pixel a lane otherwise.
#include "common.h"

namespace e4s {

constexpr int SK_PARTS = 64;                     // pieces of a sample's bytes in the range pass
constexpr int SK_TH = 16, SK_TW = 32;            // output pixels of a workgroup
constexpr int SK_ROWS = 80;                      // source rows of a tile the LDS plan holds: 15 * 4 + 14 = 74 at 1024 -> 256

// grid (SK_PARTS, bs): part[b][p] = (min, max) of bytes [p * per, (p + 1) * per) of sample b; an empty piece gives (255, 0)
__global__ __launch_bounds__(256) void sk_minmax_kernel(uint8_t* __restrict__ part, const uint8_t* __restrict__ img, int64_t n) {
    __shared__ int red[8];
    const int tid = threadIdx.x;
    const int64_t per = (n + SK_PARTS - 1) / SK_PARTS;
    const int64_t lo = min(n, (int64_t)blockIdx.x * per), hi = min(n, lo + per);
    const uint8_t* p = img + (int64_t)blockIdx.y * n + lo;
    const int64_t len = hi - lo;
    int mn = 255, mx = 0;
    const int64_t head = min(len, (int64_t)((4 - ((uintptr_t)p & 3)) & 3));                   // bytes in front of the first aligned dword
    if (tid < head) { mn = p[tid]; mx = p[tid]; }
    const uint8_t* q = p + head;
    const int64_t nd = (len - head) >> 2;
    for (int64_t i = tid; i < nd; i += 256) {
        const uint32_t u = reinterpret_cast<const uint32_t*>(q)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = (int)((u >> (8 * k)) & 0xffu);
            mn = min(mn, v);
            mx = max(mx, v);
        }
    }
    const int64_t rest = len - head - 4 * nd;
    if (tid < rest) {
        const int v = q[4 * nd + tid];
        mn = min(mn, v);
        mx = max(mx, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = min(mn, __shfl_xor(mn, m));
        mx = max(mx, __shfl_xor(mx, m));
    }
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = mn; red[2 * (tid >> 6) + 1] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { mn = min(mn, red[2 * w]); mx = max(mx, red[2 * w + 1]); }
        uint8_t* o = part + ((int64_t)blockIdx.y * SK_PARTS + blockIdx.x) * 2;
        o[0] = (uint8_t)mn;
        o[1] = (uint8_t)mx;
    }
}

// one rounding for the product, one for the sum: what numpy does, and what makes the two forms of the kernel agree
__device__ __forceinline__ double sk_mad(double acc, double w, double v) {
#pragma clang fp contract(off)
    const double p = w * v;
    return acc + p;
}

__device__ __forceinline__ int sk_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the taps of destination index d, cut to the source: [s, s + n), n <= T
__device__ __forceinline__ void sk_taps(const int* __restrict__ start, const int* __restrict__ count, int d, int src, int T, int& s, int& n) {
    s = sk_clampi(start[d], 0, src - 1);
    n = sk_clampi(count[d], 0, min(T, src - s));
}

// grid (ceil(Wo / 32), ceil(Ho / 16), bs)
__global__ __launch_bounds__(256) void sk_resize_u8_kernel(float* __restrict__ out, const uint8_t* __restrict__ img, const uint8_t* __restrict__ part,
                                                           const int* __restrict__ ystart, const int* __restrict__ ycount, const double* __restrict__ yw, int Ty,
                                                           const int* __restrict__ xstart, const int* __restrict__ xcount, const double* __restrict__ xw, int Tx,
                                                           int H, int W, int Ho, int Wo, int chw) {
    __shared__ double tmp[SK_ROWS * 3 * SK_TW];
    __shared__ double lut[256];
    __shared__ int range[2];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * SK_TW, ty0 = blockIdx.y * SK_TH;
    const int64_t b = blockIdx.z;
    const int ny = min(SK_TH, Ho - ty0), nx = min(SK_TW, Wo - tx0);
    const uint8_t* src = img + b * H * W * 3;

    lut[tid] = (double)tid / 255.0;
    if (tid < 64) {                                                             // the sample's byte range from its SK_PARTS pieces
        const uint8_t* pp = part + (b * SK_PARTS + tid) * 2;
        int mn = pp[0], mx = pp[1];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            mn = min(mn, __shfl_xor(mn, m));
            mx = max(mx, __shfl_xor(mx, m));
        }
        if (tid == 0) { range[0] = mn; range[1] = mx; }
    }
    // the tile's source rows [rmin, rmax): from the (clamped) tables, whatever they hold
    int rmin = H, rmax = 0;
    for (int y = 0; y < ny; ++y) {
        int s, n;
        sk_taps(ystart, ycount, ty0 + y, H, Ty, s, n);
        rmin = min(rmin, s);
        rmax = max(rmax, s + n);
    }
    const int nr = rmax - rmin;                                                 // (<= 0: every count of the tile is 0, the sums are 0.0)
    __syncthreads();
    const double lo = lut[range[0]], hi = lut[range[1]];
    const int x = tid & 31;

    if (nr > SK_ROWS) {                                                         // the rows do not fit: every pixel on its own (uniform over the workgroup)
        if (x >= nx) return;
        int xs, xn;
        sk_taps(xstart, xcount, tx0 + x, W, Tx, xs, xn);
        const double* wx = xw + (int64_t)(tx0 + x) * Tx;
        for (int y = tid >> 5; y < ny; y += 8) {
            int ys, yn;
            sk_taps(ystart, ycount, ty0 + y, H, Ty, ys, yn);
            const double* wy = yw + (int64_t)(ty0 + y) * Ty;
            double v[3] = {0.0, 0.0, 0.0};
            for (int ky = 0; ky < yn; ++ky) {
                const uint8_t* rp = src + ((int64_t)(ys + ky) * W + xs) * 3;
                double h[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < xn; ++k) {
                    const double w = wx[k];
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[c] = sk_mad(h[c], w, lut[rp[k * 3 + c]]);
                }
                const double w = wy[ky];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = sk_mad(v[c], w, h[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double r = fmin(fmax(v[c], lo), hi);
                const int64_t o = chw ? ((b * 3 + c) * Ho + ty0 + y) * (int64_t)Wo + tx0 + x : ((b * Ho + ty0 + y) * (int64_t)Wo + tx0 + x) * 3 + c;
                out[o] = (float)r;
            }
        }
        return;
    }

    // along x: tmp[r][c][x] = sum_k wx[k] v[rmin + r][xs + k][c].  A lane keeps its column (256 is a multiple of 32).
    if (x < nx) {
        int xs, xn;
        sk_taps(xstart, xcount, tx0 + x, W, Tx, xs, xn);
        const double* wx = xw + (int64_t)(tx0 + x) * Tx;
        for (int r = tid >> 5; r < nr; r += 8) {
            const uint8_t* rp = src + ((int64_t)(rmin + r) * W + xs) * 3;
            double h[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < xn; ++k) {
                const double w = wx[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) h[c] = sk_mad(h[c], w, lut[rp[k * 3 + c]]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) tmp[(r * 3 + c) * SK_TW + x] = h[c];
        }
    }
    __syncthreads();

    // along y: a lane owns column x of rows y and y + 8
    if (x >= nx) return;
    for (int y = tid >> 5; y < ny; y += 8) {
        int ys, yn;
        sk_taps(ystart, ycount, ty0 + y, H, Ty, ys, yn);
        const double* wy = yw + (int64_t)(ty0 + y) * Ty;
        double v[3] = {0.0, 0.0, 0.0};
        for (int ky = 0; ky < yn; ++ky) {
            const double w = wy[ky];
            const double* tp = tmp + (ys + ky - rmin) * 3 * SK_TW + x;          // rmin <= ys and ys + yn <= rmax: inside the staged rows
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = sk_mad(v[c], w, tp[c * SK_TW]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double r = fmin(fmax(v[c], lo), hi);
            const int64_t o = chw ? ((b * 3 + c) * Ho + ty0 + y) * (int64_t)Wo + tx0 + x : ((b * Ho + ty0 + y) * (int64_t)Wo + tx0 + x) * 3 + c;
            out[o] = (float)r;
        }
    }
}

__device__ __forceinline__ uint32_t fr_u8(float p) {
    const float t = p * 255.0f;
    if (!(t > 0.f)) return 0u;                                                  // negatives, -0, NaN
    return t >= 255.f ? 255u : (uint32_t)(int)t;                                // truncation toward zero
}

// one pixel a lane: e over n * hw pixels
__global__ __launch_bounds__(256) void frames_u8_kernel(uint8_t* __restrict__ out, const float* __restrict__ x, int64_t pixels, int64_t hw, int flip) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < pixels; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / hw, i = e - b * hw;
        const float* xp = x + b * 3 * hw + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[e * 3 + (flip ? 2 - c : c)] = (uint8_t)fr_u8(xp[c * hw]);
    }
}

// four pixels a lane: hw % 4 == 0, x 16-byte and out 4-byte aligned
__global__ __launch_bounds__(256) void frames_u8_x4_kernel(uint8_t* __restrict__ out, const float* __restrict__ x, int64_t quads, int64_t hw, int flip) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < quads; e += (int64_t)gridDim.x * 256) {
        const int64_t p0 = e * 4;
        const int64_t b = p0 / hw, i = p0 - b * hw;
        const float* xp = x + b * 3 * hw + i;
        uint32_t u[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 q = *reinterpret_cast<const float4*>(xp + c * hw);
            const int o = flip ? 2 - c : c;
            u[o] = fr_u8(q.x); u[3 + o] = fr_u8(q.y); u[6 + o] = fr_u8(q.z); u[9 + o] = fr_u8(q.w);
        }
        uint32_t* op = reinterpret_cast<uint32_t*>(out + p0 * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) op[k] = u[4 * k] | (u[4 * k + 1] << 8) | (u[4 * k + 2] << 16) | (u[4 * k + 3] << 24);
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_sk_resize_u8(float* out, uint8_t* part, const uint8_t* img, const int* ystart, const int* ycount, const void* yweight, int Ty,
                                const int* xstart, const int* xcount, const void* xweight, int Tx, int bs, int H, int W, int Ho, int Wo, int chw, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && H <= 16384 && W <= 16384 && Ho <= 16384 && Wo <= 16384, "sk_resize_u8: bad size");
    E4S_REQUIRE(Ty >= 1 && Tx >= 1 && Ty <= E4S_SK_MAX_TAPS && Tx <= E4S_SK_MAX_TAPS, "sk_resize_u8: a table holds 1 .. %d taps per destination index, got %d and %d",
                E4S_SK_MAX_TAPS, Ty, Tx);
    if (bs == 0) return 0;
    E4S_REQUIRE(out && part && img && ystart && ycount && yweight && xstart && xcount && xweight, "sk_resize_u8: null tensor");
    E4S_REQUIRE(((((uintptr_t)yweight) | ((uintptr_t)xweight)) & 7) == 0 && ((((uintptr_t)ystart) | ((uintptr_t)ycount) | ((uintptr_t)xstart) | ((uintptr_t)xcount)) & 3) == 0,
                "sk_resize_u8: unaligned table");
    hipLaunchKernelGGL(sk_minmax_kernel, dim3(SK_PARTS, bs), dim3(256), 0, (hipStream_t)stream, part, img, (int64_t)H * W * 3);
    const dim3 grid(cdiv(Wo, SK_TW), cdiv(Ho, SK_TH), bs);
    hipLaunchKernelGGL(sk_resize_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, img, part, ystart, ycount, static_cast<const double*>(yweight), Ty, xstart, xcount,
                       static_cast<const double*>(xweight), Tx, H, W, Ho, Wo, chw ? 1 : 0);
    return check_launch("sk_resize_u8");
}

extern "C" int e4s_frames_u8(uint8_t* out, const float* x, int n, int H, int W, int flip, void* stream) {
    E4S_REQUIRE(n >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "frames_u8: bad size");
    if (n == 0) return 0;
    E4S_REQUIRE(out && x, "frames_u8: null tensor");
    const int64_t hw = (int64_t)H * W, pixels = (int64_t)n * hw;
    if (hw % 4 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 3) == 0)
        hipLaunchKernelGGL(frames_u8_x4_kernel, dim3(grid_1d(pixels / 4)), dim3(256), 0, (hipStream_t)stream, out, x, pixels / 4, hw, flip ? 1 : 0);
    else
        hipLaunchKernelGGL(frames_u8_kernel, dim3(grid_1d(pixels)), dim3(256), 0, (hipStream_t)stream, out, x, pixels, hw, flip ? 1 : 0);
    return check_launch("frames_u8");
}
