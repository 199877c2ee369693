// Row f5: the geometry around the swap — crop-and-align of a video frame to the 1024^2 face crop, and the paste of the blended crop
// back into the frame (utils/alignment.py:101-147 `crop_image`, face_swap_video_pipeline.py:474-483).  Both are Pillow's
// Image.transform(..., BILINEAR) on 8-bit RGB (src/libImaging/Geometry.c: quad_transform / perspective_transform + bilinear_filter32RGB),
// reproduced bit for bit: the coordinate and weight arithmetic is plain double, evaluated in Pillow's order, never contracted into FMAs.
#include <math.h>

#include "common.h"

// An FMA rounds once where Pillow rounds twice: a contracted a*b+c moves the bounds test and the truncated bytes away from the library's.
#pragma clang fp contract(off)

using namespace e4s;

namespace {

constexpr int kAlignChunk = 32;        // frames per launch: their windows travel in the kernel arguments (32 x 16 B)
constexpr int kPxPerThread = 4;        // 4 RGB pixels = 12 bytes = three aligned dword stores
constexpr int kBlockX = 64, kBlockY = 4;

struct Windows {
    int4 b[kAlignChunk];               // (x0, y0, x1, y1) per frame of the chunk
};

// bilinear_filter32RGB on a source window of bw x bh pixels whose row r starts at src + r * row_stride (3 bytes per pixel).
// Returns false (Pillow: "not sampled", the caller fills) when (xi, yi) is outside [0, bw) x [0, bh) — written so that a NaN fails too.
__device__ __forceinline__ bool sample_bilinear(const uint8_t* __restrict__ src, size_t row_stride, int bw, int bh, double xi, double yi,
                                                uint8_t* px) {
    if (!(xi >= 0.0 && xi < (double)bw && yi >= 0.0 && yi < (double)bh)) return false;
    xi -= 0.5;
    yi -= 0.5;
    const int x = (int)floor(xi), y = (int)floor(yi);          // >= -1: xi, yi >= -0.5 here
    const double dx = xi - x, dy = yi - y;
    const int yc = y < 0 ? 0 : (y >= bh ? bh - 1 : y);
    const int x0 = x < 0 ? 0 : (x >= bw ? bw - 1 : x);
    const int x1 = x + 1 < 0 ? 0 : (x + 1 >= bw ? bw - 1 : x + 1);
    const bool second = y + 1 >= 0 && y + 1 < bh;
    const uint8_t* r0 = src + (size_t)yc * row_stride;
    const uint8_t* r1 = src + (size_t)(second ? y + 1 : yc) * row_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a0 = r0[x0 * 3 + c], b0 = r0[x1 * 3 + c];
        double v1 = a0 + (b0 - a0) * dx;
        double v2 = v1;
        if (second) {
            const int a1 = r1[x0 * 3 + c], b1 = r1[x1 * 3 + c];
            v2 = a1 + (b1 - a1) * dx;
        }
        v1 = v1 + (v2 - v1) * dy;
        px[c] = (uint8_t)(int)v1;                                // truncated, like the library's (UINT8) cast
    }
    return true;
}

// 12 bytes of 4 pixels: three dword stores when the address allows, else byte stores of the pixels in `mask`.
__device__ __forceinline__ void store_px4(uint8_t* dst, const uint8_t (&px)[12], unsigned mask) {
    if (mask == 0xFu && ((uintptr_t)dst & 3u) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
        return;
    }
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k)
        if (mask & (1u << k)) {
            dst[3 * k] = px[3 * k];
            dst[3 * k + 1] = px[3 * k + 1];
            dst[3 * k + 2] = px[3 * k + 2];
        }
}

// QUAD warp: out[f] (size x size) pixel (x, y) samples the window of frame f at
//   xi = a0 + a1*x' + a2*y' + a3*x'*y',  yi = a4 + a5*x' + a6*y' + a7*x'*y',  (x', y') = (x + 0.5, y + 0.5);  fill 0.
__global__ __launch_bounds__(kBlockX* kBlockY) void warp_quad_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ frames,
                                                                     const double* __restrict__ coeffs, Windows win, int h, int w, int size) {
    const int f = blockIdx.z;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    const int x4 = (blockIdx.x * kBlockX + threadIdx.x) * kPxPerThread;
    if (y >= size || x4 >= size) return;
    const int4 bx = win.b[f];
    const double* a = coeffs + (size_t)f * 8;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    const size_t rs = (size_t)w * 3;
    const uint8_t* src = frames + (size_t)f * h * rs + (size_t)bx.y * rs + (size_t)bx.x * 3;
    const int bw = bx.z - bx.x, bh = bx.w - bx.y;
    const double yin = y + 0.5;
    uint8_t px[12];
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) {
        const int x = x4 + k;
        if (x >= size) break;
        mask |= 1u << k;
        const double xin = x + 0.5;
        const double xi = a0 + a1 * xin + a2 * yin + a3 * xin * yin;
        const double yi = a4 + a5 * xin + a6 * yin + a7 * xin * yin;
        if (!sample_bilinear(src, rs, bw, bh, xi, yi, px + 3 * k)) px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = 0;
    }
    store_px4(out + ((size_t)f * size * size + (size_t)y * size + x4) * 3, px, mask);
}

// PERSPECTIVE paste: frame pixel (x, y) inside the frame's paste box samples face f at
//   xi = (a0*x' + a1*y' + a2) / (a6*x' + a7*y' + 1),  yi = (a3*x' + a4*y' + a5) / (a6*x' + a7*y' + 1);
// a sampled pixel replaces the frame's, an unsampled one is left alone (the opaque face over alpha_composite).  Threads cover the box
// from its column rounded down to a multiple of 4, so that whole-pixel quadruples of a frame with w % 4 == 0 are dword aligned.
__global__ __launch_bounds__(kBlockX* kBlockY) void warp_perspective_paste_kernel(uint8_t* __restrict__ frames, const uint8_t* __restrict__ faces,
                                                                                  const double* __restrict__ coeffs, Windows win, int h, int w,
                                                                                  int size) {
    const int f = blockIdx.z;
    const int4 bx = win.b[f];
    const int y = bx.y + (int)(blockIdx.y * kBlockY + threadIdx.y);
    const int x4 = (bx.x & ~(kPxPerThread - 1)) + (int)(blockIdx.x * kBlockX + threadIdx.x) * kPxPerThread;
    if (y >= bx.w || x4 >= bx.z) return;
    const double* a = coeffs + (size_t)f * 8;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    const uint8_t* src = faces + (size_t)f * size * size * 3;
    const double yin = y + 0.5;
    uint8_t px[12];
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) {
        const int x = x4 + k;
        if (x < bx.x || x >= bx.z) continue;
        const double xin = x + 0.5;
        const double den = a6 * xin + a7 * yin + 1;
        const double xi = (a0 * xin + a1 * yin + a2) / den;
        const double yi = (a3 * xin + a4 * yin + a5) / den;
        if (sample_bilinear(src, (size_t)size * 3, size, size, xi, yi, px + 3 * k)) mask |= 1u << k;
    }
    if (mask) store_px4(frames + ((size_t)f * h * w + (size_t)y * w + x4) * 3, px, mask);
}

int check_boxes(const char* what, const int32_t* boxes, int n, int h, int w) {
    for (int i = 0; i < n; ++i) {
        const int32_t* b = boxes + 4 * i;
        E4S_REQUIRE(b[0] >= 0 && b[1] >= 0 && b[0] <= b[2] && b[1] <= b[3] && b[2] <= w && b[3] <= h,
                    "%s: box %d = (%d, %d, %d, %d) is not inside the %dx%d frame", what, i, b[0], b[1], b[2], b[3], w, h);
    }
    return 0;
}

int check_sizes(const char* what, int n, int h, int w, int size) {
    E4S_REQUIRE(n >= 1, "%s: n = %d frames (must be >= 1)", what, n);
    E4S_REQUIRE(h >= 1 && w >= 1 && h <= 65536 && w <= 65536, "%s: bad frame size %dx%d", what, w, h);
    E4S_REQUIRE(size >= 1 && size <= 16384, "%s: bad output size %d", what, size);
    return 0;
}

}  // namespace

extern "C" int e4s_warp_quad_u8(uint8_t* out, const uint8_t* frames, const int32_t* windows, const void* coeffs, int n, int h, int w, int size,
                                void* stream) {
    E4S_REQUIRE(out && frames && windows && coeffs, "warp_quad_u8: null pointer");
    if (int st = check_sizes("warp_quad_u8", n, h, w, size)) return st;
    if (int st = check_boxes("warp_quad_u8", windows, n, h, w)) return st;
    const size_t frame_bytes = (size_t)h * w * 3, crop_bytes = (size_t)size * size * 3;
    const dim3 block(kBlockX, kBlockY);
    for (int first = 0; first < n; first += kAlignChunk) {
        const int nf = n - first < kAlignChunk ? n - first : kAlignChunk;
        Windows win;
        for (int i = 0; i < nf; ++i)
            win.b[i] = make_int4(windows[4 * (first + i)], windows[4 * (first + i) + 1], windows[4 * (first + i) + 2], windows[4 * (first + i) + 3]);
        const dim3 grid(cdiv(size, kBlockX * kPxPerThread), cdiv(size, kBlockY), nf);
        hipLaunchKernelGGL(warp_quad_kernel, grid, block, 0, (hipStream_t)stream, out + first * crop_bytes, frames + first * frame_bytes,
                           static_cast<const double*>(coeffs) + (size_t)first * 8, win, h, w, size);
        if (int st = check_launch("warp_quad_u8")) return st;
    }
    return 0;
}

extern "C" int e4s_warp_perspective_paste_u8(uint8_t* frames, const uint8_t* faces, const int32_t* boxes, const void* coeffs, int n, int h, int w,
                                             int size, void* stream) {
    E4S_REQUIRE(frames && faces && boxes && coeffs, "warp_perspective_paste_u8: null pointer");
    if (int st = check_sizes("warp_perspective_paste_u8", n, h, w, size)) return st;
    if (int st = check_boxes("warp_perspective_paste_u8", boxes, n, h, w)) return st;
    const size_t frame_bytes = (size_t)h * w * 3, crop_bytes = (size_t)size * size * 3;
    const dim3 block(kBlockX, kBlockY);
    for (int first = 0; first < n; first += kAlignChunk) {
        const int nf = n - first < kAlignChunk ? n - first : kAlignChunk;
        Windows win;
        int span_x = 0, span_y = 0;
        for (int i = 0; i < nf; ++i) {
            const int32_t* b = boxes + 4 * (first + i);
            win.b[i] = make_int4(b[0], b[1], b[2], b[3]);
            if (b[2] > b[0] && b[3] > b[1]) {
                span_x = b[2] - (b[0] & ~(kPxPerThread - 1)) > span_x ? b[2] - (b[0] & ~(kPxPerThread - 1)) : span_x;
                span_y = b[3] - b[1] > span_y ? b[3] - b[1] : span_y;
            }
        }
        if (span_x == 0 || span_y == 0) continue;               // no frame of the chunk has a pixel to paste
        const dim3 grid(cdiv(span_x, kBlockX * kPxPerThread), cdiv(span_y, kBlockY), nf);
        hipLaunchKernelGGL(warp_perspective_paste_kernel, grid, block, 0, (hipStream_t)stream, frames + first * frame_bytes,
                           faces + first * crop_bytes, static_cast<const double*>(coeffs) + (size_t)first * 8, win, h, w, size);
        if (int st = check_launch("warp_perspective_paste_u8")) return st;
    }
    return 0;
}
